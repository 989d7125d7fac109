"""The delta of a target against a base as md_pack_delta_batch_* defines it (include/mdeflate.h), in plain
Python: the index of the base's 16-byte blocks, the greedy parse and the encoding, with a trace of every match and every op.
The bytes are a pure function of base and target, so the kernel is held to them byte for byte.  Nothing here touches the
code under test; numpy only looks every target position up in the index at once."""
import functools
import struct

import numpy as np

BLOCK = 16
MUL = 0x9E3779B1
MIN_BITS = 10
EMPTY = 0xFFFFFFFF
MAX_INSERT = 127
MAX_COPY = 0x10000
MD_OK, MD_UNEXPECTED_END_OF_OUTPUT = 0, 2


def block_hash(b16):
    x = 0
    for w in struct.unpack("<4I", b16):
        x = ((x + w) * MUL) & 0xFFFFFFFF
    return x


def table_bits(nblocks):
    k = MIN_BITS
    while (1 << k) < 2 * nblocks:
        k += 1
    return k


def slot_of(b16, k):
    return block_hash(b16) >> (32 - k)


def base_index(base):
    """(k, table): table[slot] = the lowest block index that maps to the slot, EMPTY where none does"""
    nblocks = len(base) // BLOCK
    k = table_bits(nblocks)
    table = np.full(1 << k, EMPTY, dtype=np.uint32)
    if nblocks > 4096:  # (a long base: every block's hash at once, the same arithmetic)
        words = np.frombuffer(base, dtype="<u4", count=4 * nblocks).reshape(-1, 4).astype(np.uint64)
        x = np.zeros(nblocks, dtype=np.uint64)
        for w in range(4):
            x = ((x + words[:, w]) * np.uint64(MUL)) & np.uint64(0xFFFFFFFF)
        np.minimum.at(table, (x >> np.uint64(32 - k)).astype(np.int64), np.arange(nblocks, dtype=np.uint32))
        return k, table
    for j in range(nblocks - 1, -1, -1):  # (descending: the lowest is written last)
        table[slot_of(base[BLOCK * j:BLOCK * j + BLOCK], k)] = j
    return k, table


def _hits(base, target, k, table):
    """per target position p with p + 16 <= nt: the block its slot holds if that block's bytes are the target's, else -1"""
    nt = len(target)
    if nt < BLOCK:
        return np.zeros(0, dtype=np.int64)
    t = np.frombuffer(target, dtype=np.uint8).astype(np.uint64)
    npos = nt - BLOCK + 1
    x = np.zeros(npos, dtype=np.uint64)
    for w in range(4):
        word = sum(t[4 * w + b:4 * w + b + npos] << np.uint64(8 * b) for b in range(4))
        x = ((x + word) * np.uint64(MUL)) & np.uint64(0xFFFFFFFF)
    j = table[(x >> np.uint64(32 - k)).astype(np.int64)].astype(np.int64)
    out = np.full(npos, -1, dtype=np.int64)
    cand = np.nonzero(j != EMPTY)[0]
    if cand.size:
        blocks = np.frombuffer(base, dtype=np.uint8)[:len(base) // BLOCK * BLOCK].reshape(-1, BLOCK)
        windows = np.lib.stride_tricks.sliding_window_view(np.frombuffer(target, dtype=np.uint8), BLOCK)
        same = (windows[cand] == blocks[j[cand]]).all(axis=1)
        out[cand[same]] = j[cand[same]]
    return out


def _common_prefix(a, ai, b, bi):
    n = min(len(a) - ai, len(b) - bi)
    k = 0
    while k < n and a[ai + k:ai + k + 4096] == b[bi + k:bi + k + 4096]:
        k += 4096
    k = min(k, n)
    while k < n and a[ai + k] == b[bi + k]:
        k += 1
    return k


def _common_suffix(a, ai, b, bi, limit):
    """the bytes in front of a[ai] and b[bi] that are equal, at most limit"""
    e = 0
    while e < limit and a[ai - e - 1] == b[bi - e - 1]:
        e += 1
    return e


def varint(v):
    out = bytearray()
    while True:
        out.append((v & 0x7F) | (0x80 if v > 0x7F else 0))
        v >>= 7
        if not v:
            return bytes(out)


def insert_ops(data):
    """[("insert", bytes)] of 1 .. 127 bytes: 127s with the rest last"""
    return [("insert", data[i:i + MAX_INSERT]) for i in range(0, len(data), MAX_INSERT)]


def copy_ops(off, size):
    """[("copy", off, size)] of 1 .. 0x10000 bytes: 0x10000s with the rest last"""
    return [("copy", off + i, min(MAX_COPY, size - i)) for i in range(0, size, MAX_COPY)]


def encode_op(op):
    if op[0] == "insert":
        return bytes([len(op[1])]) + op[1]
    _, off, size = op
    cmd, tail = 0x80, bytearray()
    for i in range(4):
        if (off >> (8 * i)) & 0xFF:
            cmd |= 1 << i
            tail.append((off >> (8 * i)) & 0xFF)
    if size != MAX_COPY:
        for i in range(2):
            if (size >> (8 * i)) & 0xFF:
                cmd |= 0x10 << i
                tail.append((size >> (8 * i)) & 0xFF)
    return bytes([cmd]) + bytes(tail)


@functools.lru_cache(maxsize=8192)
def make_delta(base, target):
    """-> (delta bytes, trace): trace["matches"] = [{p, j, L, e, lit}], trace["ops"] = the ops in order, trace["k"], and
    trace["scan_steps"] = per match (and once for the tail) the steps of 64 positions the scan took without a hit.
    base and target are bytes (the results are kept: the tests ask for the same pairs again)"""
    nb, nt = len(base), len(target)
    k, table = base_index(base)
    hits = _hits(base, target, k, table)
    where = np.nonzero(hits >= 0)[0]
    matches, ops, steps = [], [], []
    lit = 0
    while True:
        at = int(np.searchsorted(where, lit))
        if at >= where.size:
            last = max(nt - BLOCK + 1, lit)
            steps.append(-(-(last - lit) // 64))
            break
        p = int(where[at])
        j = int(hits[p])
        steps.append((p - lit) // 64)
        L = BLOCK + _common_prefix(base, BLOCK * j + BLOCK, target, p + BLOCK)
        e = _common_suffix(base, BLOCK * j, target, p, min(p - lit, BLOCK * j))
        matches.append({"p": p, "j": j, "L": L, "e": e, "lit": lit})
        ops += insert_ops(target[lit:p - e]) + copy_ops(BLOCK * j - e, L + e)
        lit = p + L
    ops += insert_ops(target[lit:nt])
    delta = varint(nb) + varint(nt) + b"".join(encode_op(op) for op in ops)
    return delta, {"matches": matches, "ops": ops, "k": k, "scan_steps": steps}


def delta_result(base, target, out_cap):
    """what md_pack_delta_batch_* reports for one pair: (status, out_len, bytes)"""
    delta, _ = make_delta(base, target)
    if len(delta) > out_cap:
        return MD_UNEXPECTED_END_OF_OUTPUT, 0, b""
    return MD_OK, len(delta), delta


def apply_delta(base, delta):
    """a reader of git's delta format written for this file alone (tests also use tests/pack_model.py's applier)"""
    def rd(p):
        v = s = 0
        while True:
            c = delta[p]
            p += 1
            v |= (c & 0x7F) << s
            s += 7
            if not c & 0x80:
                return v, p
    nb, p = rd(0)
    nt, p = rd(p)
    assert nb == len(base)
    out = bytearray()
    while p < len(delta):
        c = delta[p]
        p += 1
        assert c != 0
        if c & 0x80:
            off = size = 0
            for i in range(4):
                if c & (1 << i):
                    off |= delta[p] << (8 * i)
                    p += 1
            for i in range(3):
                if c & (0x10 << i):
                    size |= delta[p] << (8 * i)
                    p += 1
            size = size or MAX_COPY
            assert off + size <= len(base)
            out += base[off:off + size]
        else:
            out += delta[p:p + c]
            p += c
    assert len(out) == nt
    return bytes(out)


# ---- the whole pack as md_pack_write writes it (mdeflate.h) ----------------------------------------------------------------
DELTA_MIN_TARGET, DELTA_SLACK, HEADER_MAX = 64, 20, 16


def delta_tried(nb, nt):
    return nt >= DELTA_MIN_TARGET and nb >= BLOCK


def delta_cap(nt):
    return nt // 2 - DELTA_SLACK


def stream_room(n):
    return n + n // 8 + 256


def write_bound(lens):
    return 32 + sum(HEADER_MAX + stream_room(n) for n in lens)


def keep_rule(bases, tried, fitted, max_depth):
    """-> (keep, depth, counts): in index order; a dropped delta is whole and counts as depth 0 for what hangs off it"""
    n = len(bases)
    keep, depth = [False] * n, [0] * n
    counts = {"kept": 0, "dropped_size": 0, "dropped_depth": 0}
    for i in range(n):
        if not tried[i]:
            continue
        if not fitted[i]:
            counts["dropped_size"] += 1
            continue
        d = depth[bases[i]] + 1
        if max_depth and d > max_depth:
            counts["dropped_depth"] += 1
            continue
        keep[i], depth[i] = True, d
        counts["kept"] += 1
    return keep, depth, counts


def _zl(payload, level):
    from tests import oracle_lib
    return oracle_lib.load().zl_deflate(payload, level, 4096, True)


def write_pack(objects, bases=None, level=6, max_depth=50, deltas=True, deflate=_zl):
    """objects = [(type 1 .. 4, bytes)], bases[i] = an earlier index or None -> a dict: pack, idx, entries (name, offset,
    crc32 in input order), keep, depth, payloads, and `last`, what md_pack_write_last counts but launches and time.
    deflate(payload, level) -> the zlib stream (the oracle's Zl with the parameters md_zip_compress derives from level)"""
    import hashlib
    import zlib

    from tests import pack_writer as pw
    n = len(objects)
    bases = [None] * n if bases is None or not deltas else list(bases)
    for i, b in enumerate(bases):
        assert b is None or (0 <= b < i and objects[b][0] == objects[i][0])
    tried = [b is not None and delta_tried(len(objects[b][1]), len(objects[i][1])) for i, b in enumerate(bases)]
    made = [delta_result(objects[bases[i]][1], objects[i][1], delta_cap(len(objects[i][1]))) if tried[i] else None for i in range(n)]
    keep, depth, counts = keep_rule(bases, tried, [m is not None and m[0] == MD_OK for m in made], max_depth)
    payloads = [made[i][2] if keep[i] else bytes(objects[i][1]) for i in range(n)]
    body = bytearray(b"PACK" + struct.pack(">II", 2, n))
    layout = []
    for i in range(n):
        off = len(body)
        body += pw.object_header(pw.OFS_DELTA if keep[i] else objects[i][0], len(payloads[i]))
        if keep[i]:
            body += pw.ofs_varint(off - layout[bases[i]]["offset"])
        body += deflate(payloads[i], level)
        layout.append({"name": pw.object_name(objects[i][0], bytes(objects[i][1])), "offset": off, "packed_len": len(body) - off})
    pack = bytes(body) + hashlib.sha1(bytes(body)).digest()
    entries = [{"name": o["name"], "offset": o["offset"], "crc32": zlib.crc32(pack[o["offset"]:o["offset"] + o["packed_len"]])} for o in layout]
    names = [o["name"] for o in layout]
    idx = pw.write_idx(pack, layout) if len(set(names)) == n else None  # (two objects with one name: md_pack_index_write refuses)
    last = dict(counts, pairs=sum(tried), payload_before=sum(len(o[1]) for o in objects), payload_after=sum(len(p) for p in payloads))
    return {"pack": pack, "idx": idx, "entries": entries, "keep": keep, "depth": depth, "payloads": payloads, "last": last}
