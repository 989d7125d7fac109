"""A reader of git packfiles written from the format's description (gitformat-pack), plain Python: the idx version 2, the
object headers, how a delta finds its base, depth, the delta instructions, and the statuses in the order include/mdeflate.h
gives them for md_pack_index / md_pack_open / md_pack_read.  It shares no code with the writer of the tests."""
import zlib

OK = 0
END_OF_INPUT, END_OF_OUTPUT, INVALID_CHECKSUM, INVALID_SIZE, INVALID_INDEX = 1, 2, 9, 12, 21
INVALID_PACK, INVALID_DELTA, INVALID_PACK_BASE, MISSING_BASE, UNSUPPORTED = 22, 23, 24, 25, 26
E_INVALID_ARGUMENT, E_OUT_OF_MEMORY = -1, -4
MAX_INFLATE_IN, MAX_STREAM = 0x1ffffff0, 0xfffffff0
DECODER_ERROR = 1000  # a zlib stream broken in a way the cases do not build: the library reports one of its decoder's statuses


def _be(b, at, n):
    return int.from_bytes(b[at:at + n], "big")


def read_idx(idx):
    """-> (status, entries, info): entries [(name, offset, crc)] ascending by name; info: n, has64, pack_checksum"""
    if len(idx) < 8:
        return INVALID_INDEX, None, None
    if idx[:4] != b"\xfftOc" or _be(idx, 4, 4) != 2:
        return UNSUPPORTED, None, None
    if len(idx) < 8 + 1024 + 40:
        return INVALID_INDEX, None, None
    fan = [_be(idx, 8 + 4 * b, 4) for b in range(256)]
    if any(fan[b] < fan[b - 1] for b in range(1, 256)):
        return INVALID_INDEX, None, None
    n = fan[255]
    room = len(idx) - (8 + 1024 + 40)
    if n * 28 > room:
        return INVALID_INDEX, None, None
    names_at, crc_at, off_at = 1032, 1032 + 20 * n, 1032 + 24 * n
    big_at = 1032 + 28 * n
    words = [_be(idx, off_at + 4 * i, 4) for i in range(n)]
    m = sum(w >> 31 for w in words)
    if room - 28 * n != 8 * m:
        return INVALID_INDEX, None, None
    names = [idx[names_at + 20 * i:names_at + 20 * i + 20] for i in range(n)]
    for i, nm in enumerate(names):
        if i and names[i - 1] >= nm:
            return INVALID_INDEX, None, None
        lo = fan[nm[0] - 1] if nm[0] else 0
        if not lo <= i < fan[nm[0]]:
            return INVALID_INDEX, None, None
    entries = []
    for i, w in enumerate(words):
        if w >> 31:
            if (w & 0x7fffffff) >= m:
                return INVALID_INDEX, None, None
            w = _be(idx, big_at + 8 * (w & 0x7fffffff), 8)
        entries.append((names[i], w, _be(idx, crc_at + 4 * i, 4)))
    return OK, entries, {"n": n, "has64": int(m != 0), "pack_checksum": idx[big_at + 8 * m:big_at + 8 * m + 20]}


def _leb(b, at):
    """LEB128 at b[at:] -> (value, next) or None: it passes the end or does not fit 64 bits"""
    v = shift = 0
    while True:
        if at >= len(b):
            return None
        c = b[at]
        at += 1
        v |= (c & 0x7f) << shift
        shift += 7
        if v >> 64:
            return None
        if not c & 0x80:
            return v, at


def _inflate(stream, size):
    """the zlib stream that fills `stream` into exactly `size` bytes -> (status, bytes)"""
    d = zlib.decompressobj()
    try:
        out = d.decompress(stream, size + 1)
    except zlib.error as e:
        return (INVALID_CHECKSUM if "incorrect data check" in str(e) else DECODER_ERROR), b""
    if len(out) > size:
        return INVALID_SIZE, b""
    if not d.eof:
        return (END_OF_INPUT if not d.unconsumed_tail else DECODER_ERROR), b""
    if d.unused_data or len(out) != size:
        return INVALID_SIZE, b""
    return OK, out


class Model:
    """md_pack_open's table (self.rc: the call's return value; self.objects in idx order) and md_pack_read"""

    def __init__(self, pack, idx):
        self.pack, self.objects = pack, []
        self.rc, ent, info = read_idx(idx)
        if self.rc != OK:
            return
        if len(pack) < 32 or pack[:4] != b"PACK":
            self.rc = INVALID_PACK
        elif _be(pack, 4, 4) not in (2, 3):
            self.rc = UNSUPPORTED
        elif _be(pack, 8, 4) != info["n"] or pack[-20:] != info["pack_checksum"]:
            self.rc = INVALID_INDEX
        elif any(off < 12 or off >= len(pack) - 20 for _, off, _ in ent) or len({off for _, off, _ in ent}) != len(ent):
            self.rc = INVALID_INDEX
        if self.rc != OK:
            return
        n = len(ent)
        by_off = sorted(range(n), key=lambda i: ent[i][1])
        end = {}
        for s, i in enumerate(by_off):
            end[i] = ent[by_off[s + 1]][1] if s + 1 < n else len(pack) - 20
        at_off = {ent[i][1]: i for i in range(n)}
        by_name = {ent[i][0]: i for i in range(n)}
        objs = [self._header(i, ent[i], end[i], at_off, by_name) for i in range(n)]
        # depth and root: follow the links; what comes back to itself, or never ends, is on a cycle or hangs off one
        for i, o in enumerate(objs):
            j, steps = i, 0
            while objs[j]["link"] and steps <= n:
                j, steps = objs[j]["base"], steps + 1
            o["cycle"] = steps > n
            o["depth"], o["root"] = (0, i) if o["cycle"] else (steps, j)
        for o in objs:
            if o["cycle"]:
                if o["status"] == OK:
                    o["status"] = INVALID_PACK
                o["link"] = False
        # the deltas' own sizes
        for o in objs:
            o["result_size"] = o["base_size"] = 0
            if o["status"] == OK and (o["end"] - o["zoff"] > MAX_INFLATE_IN or o["hsize"] > MAX_STREAM):
                o["status"] = E_INVALID_ARGUMENT
            if o["status"] == OK and o["link"]:
                st, payload = _inflate(pack[o["zoff"]:o["end"]], o["hsize"])
                a = _leb(payload, 0) if st == OK else None
                b = _leb(payload, a[1]) if a else None
                if st != OK:
                    o["status"] = st
                elif not b:
                    o["status"] = INVALID_DELTA
                else:
                    o["base_size"], o["result_size"] = a[0], b[0]
                    if b[0] > MAX_STREAM:
                        o["status"] = E_INVALID_ARGUMENT
        for i in sorted(range(n), key=lambda i: objs[i]["depth"]):
            o = objs[i]
            o["size"] = o["result_size"] if o["link"] else o["hsize"]
            if o["link"] and o["status"] == OK:
                b = objs[o["base"]]
                if b["status"] != OK:
                    o["status"] = INVALID_PACK_BASE
                elif o["base_size"] != b["size"]:
                    o["status"] = INVALID_DELTA
            if o["status"] != OK:
                o["size"] = 0
        for o in objs:
            t = objs[o["root"]]["own_type"]
            o["type"] = t if 1 <= t <= 4 else 0
        self.objects = objs
        self.info = {"n": n, "deltas": sum(o["link"] for o in objs), "max_depth": max([o["depth"] for o in objs] or [0]),
                     "total_size": sum(o["size"] for o in objs), "failed": sum(o["status"] != OK for o in objs)}

    def _header(self, i, entry, end, at_off, by_name):
        name, off, crc = entry
        pack = self.pack
        o = {"name": name, "offset": off, "end": end, "packed_len": end - off, "crc": crc, "base": None, "status": OK, "link": False,
             "own_type": 0, "hsize": 0, "zoff": off}
        p = off
        c = pack[p]
        p += 1
        o["own_type"], size, shift = (c >> 4) & 7, c & 15, 4
        while c & 0x80:
            if p >= end:
                o["status"] = INVALID_PACK
                return o
            c = pack[p]
            p += 1
            size |= (c & 0x7f) << shift
            shift += 7
        if size >> 64 or o["own_type"] in (0, 5):
            o["status"] = INVALID_PACK
            return o
        o["hsize"] = size
        if o["own_type"] == 6:
            v, first = 0, True
            while True:
                if p >= end or v >> 56:
                    o["status"] = INVALID_PACK
                    return o
                c = pack[p]
                p += 1
                v = ((0 if first else v + 1) << 7) | (c & 0x7f)
                first = False
                if not c & 0x80:
                    break
            if v == 0 or v > off or off - v not in at_off:
                o["status"] = INVALID_PACK
                return o
            o["base"] = at_off[off - v]
        elif o["own_type"] == 7:
            if end - p < 20:
                o["status"] = INVALID_PACK
                return o
            want = pack[p:p + 20]
            p += 20
            if want not in by_name:
                o["status"] = MISSING_BASE
            else:
                o["base"] = by_name[want]
                if o["base"] == i:
                    o["status"] = INVALID_PACK
        o["zoff"] = p
        o["link"] = o["status"] == OK and o["base"] is not None
        return o

    def _apply(self, o, payload, base):
        a = _leb(payload, 0)
        b = _leb(payload, a[1]) if a else None
        if not b or a[0] != len(base) or b[0] != o["size"]:
            return INVALID_DELTA, b""
        p, out, want = b[1], bytearray(), o["size"]
        while p < len(payload):
            op = payload[p]
            p += 1
            if op == 0:
                return INVALID_DELTA, b""
            if op & 0x80:
                off = size = 0
                for k in range(7):
                    if op >> k & 1:
                        if p >= len(payload):
                            return INVALID_DELTA, b""
                        if k < 4:
                            off |= payload[p] << (8 * k)
                        else:
                            size |= payload[p] << (8 * (k - 4))
                        p += 1
                size = size or 0x10000
                if off + size > len(base) or len(out) + size > want:
                    return INVALID_DELTA, b""
                out += base[off:off + size]
            else:
                if p + op > len(payload) or len(out) + op > want:
                    return INVALID_DELTA, b""
                out += payload[p:p + op]
                p += op
        return (OK, bytes(out)) if len(out) == want else (INVALID_DELTA, b"")

    def _decode(self, i, verify, memo):
        if i in memo:
            return memo[i]
        o = self.objects[i]
        st, got = _inflate(self.pack[o["zoff"]:o["end"]], o["hsize"])
        if st == OK and verify and zlib.crc32(self.pack[o["offset"]:o["end"]]) != o["crc"]:
            st = INVALID_CHECKSUM
        if st == OK and o["link"]:
            bst, base = self._decode(o["base"], verify, memo)
            st, got = (INVALID_PACK_BASE, b"") if bst != OK else self._apply(o, got, base)
        memo[i] = (st, got if st == OK else b"")
        return memo[i]

    def read(self, select=None, verify=False):
        """-> [(status, bytes)] for the objects `select` (idx order; None: all)"""
        memo = {}
        out = []
        for i in (range(len(self.objects)) if select is None else select):
            o = self.objects[i]
            out.append((o["status"], b"") if o["status"] != OK else self._decode(i, verify, memo))
        return out

    def closure(self, select):
        """the objects a read of `select` decodes: the sound ones and their chains of bases, each once"""
        need = set()
        for i in select:
            while self.objects[i]["status"] == OK and i not in need:
                need.add(i)
                if not self.objects[i]["link"]:
                    break
                i = self.objects[i]["base"]
        return need
