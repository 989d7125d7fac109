"""A plain-Python index-pack, written from git's description of the pack and idx formats (gitformat-pack) and from what
include/mdeflate.h says of md_pack_index_build: no idx is given, the objects are found by walking the zlib streams from byte
12 with zlib's own decoder, their names are resolved to a fixpoint in generations, and the idx version 2 is written.  It
shares no code with the library; from the tests' reader (pack_model.py) it takes the status numbers and the delta
instructions.

  BuildModel(pack, check_trailer)   rc, bad_offset, bad_status, n, offsets, status, idx, generations, candidates, objects
  candidate_positions(pack)         every z of [12, len - 26] whose two bytes pass the decoder's test of a zlib header
  candidate_table(pack)             [(z, consumed, out_len, status)] as the size query answers for each of them
"""
import hashlib
import struct
import zlib

from tests import pack_model as pm

OK = pm.OK
NO_OFFSET = (1 << 64) - 1
TYPE_NAMES = {1: b"commit", 2: b"tree", 3: b"blob", 4: b"tag"}
_PAIRS = frozenset((c, f) for c in range(256) for f in range(256) if (c & 15) == 8 and ((c << 8) + f) % 31 == 0)


def candidate_positions(pack):
    hi = len(pack) - 20 - 6
    return [z for z in range(12, hi + 1) if (pack[z], pack[z + 1]) in _PAIRS]


def count_stream(pack, z):
    """the zlib stream at pack[z:len - 20] as the size query sees it -> (status, consumed, inflated bytes, the Adler-32
    holds); the query does not compare the checksum, it only needs its four bytes to be there"""
    end = len(pack) - 20
    if pack[z + 1] & 0x20:
        return pm.DECODER_ERROR, 0, b"", False  # (a preset dictionary: no case builds one)
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(pack[z + 2:end])
    except zlib.error:
        return pm.DECODER_ERROR, 0, b"", False
    if not d.eof or len(d.unused_data) < 4:
        return pm.END_OF_INPUT, 0, b"", False
    consumed = end - z - len(d.unused_data) + 4
    return OK, consumed, out, d.unused_data[:4] == struct.pack(">I", zlib.adler32(out))


def candidate_table(pack):
    out = []
    for z in candidate_positions(pack):
        st, consumed, data, _ = count_stream(pack, z)
        out.append((z, consumed, len(data), st))
    return out


def parse_header(pack, at, end):
    """-> (type, size, z, link) or None; link: an OFS_DELTA's distance, a REF_DELTA's 20 bytes"""
    p = at
    if p >= end:
        return None
    c = pack[p]
    p += 1
    t, size, shift = (c >> 4) & 7, c & 15, 4
    while c & 0x80:
        if p >= end:
            return None
        c = pack[p]
        p += 1
        size |= (c & 0x7f) << shift
        shift += 7
        if size >> 64:
            return None
    if t in (0, 5):
        return None
    link = None
    if t == 6:
        v, first = 0, True
        while True:
            if p >= end or v >> 56:
                return None
            c = pack[p]
            p += 1
            v = ((0 if first else v + 1) << 7) | (c & 0x7f)
            first = False
            if not c & 0x80:
                break
        link = v
    elif t == 7:
        if end - p < 20:
            return None
        link = bytes(pack[p:p + 20])
        p += 20
    return t, size, p, link


def write_idx(entries, pack_checksum):
    """[(name, offset, crc)] in any order -> the idx version 2"""
    entries = sorted(entries)
    fan = [0] * 256
    for name, _, _ in entries:
        fan[name[0]] += 1
    for b in range(1, 256):
        fan[b] += fan[b - 1]
    out = bytearray(b"\xfftOc" + struct.pack(">I", 2) + struct.pack(">256I", *fan))
    out += b"".join(name for name, _, _ in entries)
    out += b"".join(struct.pack(">I", crc) for _, _, crc in entries)
    big = bytearray()
    for _, off, _ in entries:
        if off > 0x7fffffff:
            out += struct.pack(">I", 0x80000000 | len(big) // 8)
            big += struct.pack(">Q", off)
        else:
            out += struct.pack(">I", off)
    out += big + pack_checksum
    return bytes(out) + hashlib.sha1(bytes(out)).digest()


class BuildModel:
    def __init__(self, pack, check_trailer=True):
        self.pack = pack
        self.rc, self.bad_offset, self.bad_status = OK, NO_OFFSET, OK
        self.n, self.offsets, self.status, self.idx, self.generations, self.candidates, self.objects = 0, [], [], b"", 0, 0, []
        if len(pack) < 32 or pack[:4] != b"PACK":
            self.rc = pm.INVALID_PACK
            return
        if struct.unpack_from(">I", pack, 4)[0] not in (2, 3):
            self.rc = pm.UNSUPPORTED
            return
        end = len(pack) - 20
        self.candidates = len(candidate_positions(pack))
        if check_trailer and hashlib.sha1(pack[:end]).digest() != pack[end:]:
            self.rc, self.bad_offset = pm.INVALID_CHECKSUM, end
            return
        if not self._walk(end):
            self.rc = pm.INVALID_PACK
            return
        self.n = len(self.objs)
        self.offsets = [o["off"] for o in self.objs]
        self._resolve()
        self.status = [o["final"] for o in self.objs]
        bad = [i for i, st in enumerate(self.status) if st != OK]
        if bad:
            self.rc, self.bad_offset = self.status[bad[0]], self.objs[bad[0]]["off"]
            return
        self.objects = [(o["root_type"], o["data"]) for o in self.objs]
        self.idx = write_idx([(o["name"], o["off"], zlib.crc32(pack[o["off"]:o["end"]])) for o in self.objs], pack[end:])

    def _walk(self, end):
        pack, at, count = self.pack, 12, struct.unpack_from(">I", self.pack, 8)[0]
        cand = set(candidate_positions(pack))
        self.objs = []
        while at < end:
            self.bad_offset = at
            if len(self.objs) == count:
                return False
            h = parse_header(pack, at, end)
            if h is None or h[2] not in cand:
                return False
            t, size, z, link = h
            st, consumed, raw, adler = count_stream(pack, z)
            if st != OK:
                self.bad_status = st
                return False
            self.objs.append({"off": at, "type": t, "hsize": size, "z": z, "link": link, "raw": raw, "adler": adler, "end": z + consumed})
            at = z + consumed
        self.bad_offset = end
        if len(self.objs) != count:
            return False
        self.bad_offset = NO_OFFSET
        return True

    def _table(self, known):
        """what the table of a generation says with the names in `known` (name -> object): status, base, size per object"""
        objs, n = self.objs, len(self.objs)
        at_off = {o["off"]: i for i, o in enumerate(objs)}
        st, base = [OK] * n, [None] * n
        for i, o in enumerate(objs):
            if o["type"] == 6:
                v = o["link"]
                if v == 0 or v > o["off"] or o["off"] - v not in at_off:
                    st[i] = pm.INVALID_PACK
                else:
                    base[i] = at_off[o["off"] - v]
            elif o["type"] == 7:
                if o["link"] in known:
                    base[i] = known[o["link"]]
                else:
                    st[i] = pm.MISSING_BASE
        depth, root = [0] * n, list(range(n))
        for i in range(n):
            j, steps = i, 0
            while base[j] is not None:
                j, steps = base[j], steps + 1
                assert steps <= n  # (a base has a name, so it was decoded, so its chain ends)
            depth[i], root[i] = steps, j
        bs, rs = [0] * n, [0] * n
        for i, o in enumerate(objs):
            if st[i] == OK and (o["end"] - o["z"] > pm.MAX_INFLATE_IN or o["hsize"] > pm.MAX_STREAM):
                st[i] = pm.E_INVALID_ARGUMENT
            if st[i] == OK and base[i] is not None:
                own = self._own(o)
                a = pm._leb(o["raw"], 0) if own == OK else None
                b = pm._leb(o["raw"], a[1]) if a else None
                if own != OK:
                    st[i] = own
                elif not b:
                    st[i] = pm.INVALID_DELTA
                else:
                    bs[i], rs[i] = a[0], b[0]
                    if b[0] > pm.MAX_STREAM:
                        st[i] = pm.E_INVALID_ARGUMENT
        size = [0] * n
        for i in sorted(range(n), key=lambda i: depth[i]):
            linked = base[i] is not None
            size[i] = rs[i] if linked else objs[i]["hsize"]
            if linked and st[i] == OK:
                if st[base[i]] != OK:
                    st[i] = pm.INVALID_PACK_BASE
                elif bs[i] != size[base[i]]:
                    st[i] = pm.INVALID_DELTA
            if st[i] != OK:
                size[i] = 0
        return st, base, size, root

    @staticmethod
    def _own(o):
        """the stream's own verdict: the size its header states, then the Adler-32"""
        if len(o["raw"]) != o["hsize"]:
            return pm.INVALID_SIZE
        return OK if o["adler"] else pm.INVALID_CHECKSUM

    def _resolve(self):
        objs, n = self.objs, len(self.objs)
        verdict, known = [None] * n, {}
        for o in objs:
            o["data"] = o["name"] = o["root_type"] = None
        table = [OK] * n
        while True:
            table, base, size, root = self._table(known)
            sel = [i for i in range(n) if table[i] == OK and verdict[i] is None]
            if not sel:
                break
            self.generations += 1
            memo = {}

            def decode(i):
                if i not in memo:
                    o = objs[i]
                    st, got = self._own(o), o["raw"]
                    if st == OK and base[i] is not None:
                        bst, bdata = decode(base[i])
                        st, got = (pm.INVALID_PACK_BASE, b"") if bst != OK else pm.Model._apply(None, {"size": size[i]}, got, bdata)
                    memo[i] = (st, got if st == OK else b"")
                return memo[i]

            import sys
            sys.setrecursionlimit(max(sys.getrecursionlimit(), 10 * n + 1000))
            fresh = 0
            for i in sel:
                verdict[i], data = decode(i)
                if verdict[i] == OK:
                    t = objs[root[i]]["type"]
                    o = objs[i]
                    o["data"], o["root_type"] = data, t
                    o["name"] = hashlib.sha1(TYPE_NAMES[t] + b" %d\0" % len(data) + data).digest()
                    known.setdefault(o["name"], i)
                    fresh += 1
            waiting = any(verdict[i] is None and table[i] in (pm.MISSING_BASE, pm.INVALID_PACK_BASE) for i in range(n))
            if not fresh or not waiting:
                break
        for i, o in enumerate(objs):
            if verdict[i] is not None:
                o["final"] = verdict[i]
            else:
                o["final"] = pm.INVALID_SIZE if len(o["raw"]) != o["hsize"] else table[i]
        seen = set()
        for o in objs:  # pack order: the later of two objects with one name
            if o["final"] == OK:
                if o["name"] in seen:
                    o["final"] = pm.INVALID_PACK
                seen.add(o["name"])
