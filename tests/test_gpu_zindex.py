"""The index of one long stream on the GPU (md_inflate_index_*; csrc/capi_zindex.cpp, zindex_kernels.hip).  Needs
an MI355X: `pytest -m gpu`.  Yardsticks: zlib for the plaintext, the existing one-stream calls for status / consumed /
size / checksum, a block walk of this file's own for where blocks start, tests/deflate_writer for the hand-built stream -
never the code under test."""
import contextlib
import ctypes
import random
import struct
import zlib

import pytest

from tests import deflate_writer as dw
from tests.deflate_tokens import DB, DX, LB, LX

pytestmark = pytest.mark.gpu
SPAN = 32 << 10
OK, END_OF_INPUT, END_OF_OUTPUT, INVALID_INDEX = 0, 1, 2, 21
FMT_RAW, FMT_ZLIB, FMT_GZIP = 0, 1, 2
GZ_HEAD = b"\x1f\x8b\x08\x08" + struct.pack("<I", 1234567) + b"\x00\x03" + b"name.txt\x00"


@pytest.fixture(scope="module")
def eng():
    from decompress_amd import engine
    return engine.default_engine(0)


def _Index():
    from decompress_amd.index import Index
    return Index


# ---- where blocks start: a plain walk over the stream ----
def _lookup(lens):
    """canonical code lengths -> (table over the next `mx` bits as they come, mx)"""
    mx = max(lens)
    nxt, code = [0] * (mx + 2), 0
    for b in range(1, mx + 1):
        code = (code + sum(1 for l in lens if l == b - 1 and l)) << 1
        nxt[b] = code
    tab = [None] * (1 << mx)
    for sym, l in enumerate(lens):
        if l:
            rev = int(format(nxt[l], "0%db" % l)[::-1], 2)
            nxt[l] += 1
            for hi in range(rev, 1 << mx, 1 << l):
                tab[hi] = (sym, l)
    return tab, mx


def block_starts(raw):
    """[(bit, out)] of every block of the raw DEFLATE stream `raw`, the bit behind the last one, the output's size"""
    data = raw + bytes(16)
    pos, out, starts = 0, 0, []

    def take(n):
        nonlocal pos
        v = (int.from_bytes(data[pos >> 3:(pos >> 3) + 8], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        return v

    fixed = (_lookup(dw.FIXED_LIT), _lookup(dw.FIXED_DIST))
    while True:
        starts.append((pos, out))
        last, kind = take(1), take(2)
        if kind == 0:
            pos = (pos + 7) & ~7
            n = take(16)
            assert take(16) == n ^ 0xffff
            pos += 8 * n
            out += n
        else:
            assert kind in (1, 2)
            if kind == 1:
                (lt, lm), (dt, dm) = fixed
            else:
                hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[dw.CL_ORDER[i]] = take(3)
                ct, cm = _lookup(cl)
                lens = []
                while len(lens) < hlit + hdist:
                    sym, l = ct[take(cm)]
                    pos -= cm - l
                    if sym < 16:
                        lens.append(sym)
                    elif sym == 16:
                        lens += [lens[-1]] * (3 + take(2))
                    else:
                        lens += [0] * ((3 + take(3)) if sym == 17 else (11 + take(7)))
                (lt, lm), (dt, dm) = _lookup(lens[:hlit]), _lookup(lens[hlit:] if any(lens[hlit:]) else [1])
            p = pos  # (the hot loop keeps the position in a local)
            while True:
                w = int.from_bytes(data[p >> 3:(p >> 3) + 8], "little") >> (p & 7)
                sym, l = lt[w & ((1 << lm) - 1)]
                p += l
                if sym < 256:
                    out += 1
                elif sym == 256:
                    break
                else:
                    w >>= l
                    i = sym - 257
                    out += LB[i] + (w & ((1 << LX[i]) - 1))
                    w >>= LX[i]
                    d, dl = dt[w & ((1 << dm) - 1)]
                    p += LX[i] + dl + DX[d]
            pos = p
        if last:
            return starts, pos, out


def test_block_walk_agrees_with_the_writer():
    """(the walk itself, on streams whose blocks the writer and libz know)"""
    blocks = [dw.Block("stored", list(range(200))), dw.Block("fixed", [65] * 10 + [(20, 5)]), dw.Block("dynamic", [66] * 40 + [(258, 7), 67])]
    raw = dw.write(blocks)
    starts, end, size = block_starts(raw)
    assert [o for _, o in starts] == [0, 200, 230] and starts[1][0] == 8 * 205 and size == len(dw.expand(blocks)[1]) == 529
    assert (end + 7) // 8 == len(raw)
    for name in ("text", "ascii", "fixed", "stored", "zeros"):
        raw, plain, starts = _input(name)
        _, end, size = block_starts(raw)
        assert size == len(plain) and (end + 7) // 8 == len(raw) and starts[0] == (0, 0), name


# ---- inputs ----
_CACHE = {}


def _deflate(plain, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(plain) + c.flush()


def _input(name):
    if name not in _CACHE:
        from decompress_amd import workloads
        plain, level, strategy = {
            "text": lambda: (workloads.text(7, 512 << 10), 6, zlib.Z_DEFAULT_STRATEGY),
            "ascii": lambda: (workloads.ascii_uniform(7, 256 << 10), 6, zlib.Z_DEFAULT_STRATEGY),
            "fixed": lambda: (workloads.text(9, 256 << 10), 6, zlib.Z_FIXED),
            "stored": lambda: (workloads.ascii_uniform(3, 256 << 10), 0, zlib.Z_DEFAULT_STRATEGY),
            "zeros": lambda: (bytes(512 << 10), 6, zlib.Z_DEFAULT_STRATEGY),
        }[name]()
        raw = _deflate(plain, level, strategy)
        assert zlib.decompress(raw, -15) == plain
        _CACHE[name] = (raw, plain, block_starts(raw)[0])
    return _CACHE[name]


def _frame(raw, plain, fmt):
    """(src, header length) of the raw body in the frame of `fmt`"""
    if fmt == FMT_ZLIB:
        return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(plain)), 2
    if fmt == FMT_GZIP:
        return GZ_HEAD + raw + struct.pack("<II", zlib.crc32(plain), len(plain) & 0xffffffff), len(GZ_HEAD)
    return raw, 0


@contextlib.contextmanager
def _path(eng, parallel):
    """the long-stream decoder for pieces from 16 KiB of input on, in pieces of 4 KiB - or never"""
    eng.set_option("inflate_parallel_chunk", 4)
    eng.set_option("inflate_parallel_min", 16 if parallel else 0)
    try:
        yield
    finally:
        eng.set_option("inflate_parallel_chunk", 64)
        eng.set_option("inflate_parallel_min", 96)


def _built(eng, name, parallel=None, fmt=FMT_RAW, span=SPAN):
    """the index of an input, built once per (input, path, frame)"""
    key = ("idx", name, parallel, fmt, span)
    if key not in _CACHE:
        raw, plain, _ = _input(name)
        src, _ = _frame(raw, plain, fmt)
        if parallel is None:
            _CACHE[key] = (_Index().build(src, fmt, span=span), src, None)
        else:
            with _path(eng, parallel):
                idx = _Index().build(src, fmt, span=span)
                last = eng.lib.md_set_option(eng.ctx, b"inflate_parallel_last", 0)
            _CACHE[key] = (idx, src, last)
    return _CACHE[key]


def _windows(blob):
    """the windows of a serialised index, by the layout in mdeflate.h"""
    npoints = struct.unpack_from("<Q", blob, 56)[0]
    at, out = 72 + 24 * npoints, []
    for k in range(npoints):
        w = struct.unpack_from("<I", blob, 72 + 24 * k + 16)[0]
        out.append(blob[at:at + w])
        at += w
    assert at == len(blob)
    return out


def _check_points(idx, plain, starts, bit0, span):
    pts = idx.points
    blocks = {(b + bit0, o) for b, o in starts}
    assert pts[0] == (bit0, 0)
    assert all(p in blocks for p in pts), [p for p in pts if p not in blocks]
    assert all(b[1] - a[1] >= span and b[0] > a[0] for a, b in zip(pts, pts[1:]))
    wins = _windows(idx.dumps())
    assert len(wins) == len(pts)
    for (_, o), w in zip(pts, wins):
        assert len(w) == min(32768, o) and w == plain[o - len(w):o], o
    return pts


def _greedy(starts, span):
    kept = [starts[0]]
    for s in starts[1:]:
        if s[1] >= kept[-1][1] + span:
            kept.append(s)
    return kept


# ---- build ----
@pytest.mark.parametrize("fmt", [FMT_RAW, FMT_ZLIB, FMT_GZIP])
def test_build_reports_what_the_plain_call_reports(eng, fmt):
    import numpy as np
    raw, plain, starts = _input("text")
    src, hdr = _frame(raw, plain, fmt)
    h_in, h_out = np.frombuffer(src, dtype=np.uint8), np.zeros(len(plain) + 64, dtype=np.uint8)
    out_len, consumed, status, checksum = eng.inflate_batch_host(fmt, h_in, [0], [len(src)], h_out, [0], [len(plain) + 64])
    assert status[0] == OK and h_out[:int(out_len[0])].tobytes() == plain
    for parallel in (True, False):
        idx, _, last = _built(eng, "text", parallel, fmt)
        info = idx.info
        assert (info["format"], info["src_len"], info["header_len"], info["span"]) == (fmt, len(src), hdr, SPAN)
        assert (info["consumed"], info["size"], info["checksum"]) == (int(consumed[0]), int(out_len[0]), int(checksum[0])), parallel
        assert (last != 0) == parallel  # (the path the options ask for is the path taken)
        assert info["points"] == len(_check_points(idx, plain, starts, 8 * hdr, SPAN))


@pytest.mark.parametrize("name,parallel", [("text", True), ("text", False), ("ascii", True), ("ascii", False), ("fixed", None),
                                           ("stored", None), ("zeros", None)])
def test_points_are_block_starts_with_their_windows(eng, name, parallel):
    raw, plain, starts = _input(name)
    idx, _, last = _built(eng, name, parallel)
    pts = _check_points(idx, plain, starts, 0, SPAN)
    greedy = _greedy(starts, SPAN)
    print(name, parallel, "blocks", len(starts), "greedy", len(greedy), "points", len(pts), "pieces | rounds << 24", last)
    assert len(pts) <= len(greedy)
    if name in ("text", "ascii"):
        assert len(pts) >= 4 and 2 * len(pts) >= len(greedy)  # (8 greedy points with libz 1.2.11)
        assert (last != 0) == parallel
    if name == "zeros":
        assert len(starts) == 1 and len(pts) == 1


def test_want_output_and_short_room(eng):
    raw, plain, _ = _input("text")
    src, _ = _frame(raw, plain, FMT_ZLIB)
    for parallel in (True, False):
        with _path(eng, parallel):
            idx, out = _Index().build(src, FMT_ZLIB, span=SPAN, want_output=True, dst_len=len(plain))
            assert out == plain and idx.info["size"] == len(plain)
            h, dst = ctypes.c_void_p(1), ctypes.create_string_buffer(len(plain))
            st = eng.lib.md_inflate_index_build(eng.ctx, FMT_ZLIB, src, len(src), SPAN, dst, len(plain) - 1, ctypes.byref(h), None)
            assert st == END_OF_OUTPUT and not h.value
    assert eng.lib.md_inflate_index_build(eng.ctx, FMT_ZLIB, src, len(src), 4095, None, 0, ctypes.byref(h), None) == -1
    assert eng.lib.md_inflate_index_build(eng.ctx, 3, src, len(src), 0, None, 0, ctypes.byref(h), None) == -1


def test_corrupted_stream_gives_the_plain_status_and_no_index(eng):
    import numpy as np
    raw, plain, _ = _input("text")
    good, _ = _frame(raw, plain, FMT_ZLIB)
    cap = len(plain) + 64
    cases = [good[:k] + bytes([good[k] ^ 0xff]) + good[k + 1:] for k in (0, len(good) // 4, len(good) // 2, len(good) - 2)]
    cases += [good[:len(good) // 2], good[:-1]]
    seen = set()
    for src in cases:
        h_out = np.zeros(cap, dtype=np.uint8)
        _, _, status, _ = eng.inflate_batch_host(FMT_ZLIB, np.frombuffer(src, dtype=np.uint8), [0], [len(src)], h_out, [0], [cap])
        want = int(status[0])
        assert want != OK
        seen.add(want)
        for parallel in (True, False):
            with _path(eng, parallel):
                h, dst = ctypes.c_void_p(1), ctypes.create_string_buffer(cap)
                assert eng.lib.md_inflate_index_build(eng.ctx, FMT_ZLIB, src, len(src), SPAN, dst, cap, ctypes.byref(h), None) == want
                assert not h.value
                if want != END_OF_OUTPUT:  # (without a destination there is no room to run out of)
                    h = ctypes.c_void_p(1)
                    assert eng.lib.md_inflate_index_build(eng.ctx, FMT_ZLIB, src, len(src), SPAN, None, 0, ctypes.byref(h), None) == want
                    assert not h.value
    assert len(seen) >= 3, seen  # (header, body or checksum, truncation)


# ---- read ----
def _pieces_of(pts, size, ranges):
    outs = [o for _, o in pts]
    hit = set()
    for off, n in ranges:
        for k in range(len(outs)):
            end = outs[k + 1] if k + 1 < len(outs) else size
            if n and off < end and off + n > outs[k] and end > outs[k]:
                hit.add(k)
    return hit


def _ranges(pts, size, seed):
    rng = random.Random(seed)
    outs = [o for _, o in pts]
    r = [(0, 1), (size - 1, 1), (0, size), (size // 2, 0)]
    r += [(max(0, o - 5), min(10, size - max(0, o - 5))) for o in outs]
    k = min(1, len(outs) - 1)
    r.append((outs[k], (outs[k + 1] if k + 1 < len(outs) else size) - outs[k]))  # exactly one piece
    for _ in range(64):
        a = rng.randrange(size)
        r.append((a, rng.randrange(1, min(size - a, 1 << rng.randrange(1, 18)) + 1)))
    return r


@pytest.mark.parametrize("name", ["text", "ascii", "fixed", "stored", "zeros"])
def test_read_many_equals_slices_of_the_plaintext(eng, name):
    raw, plain, _ = _input(name)
    parallel = True if name in ("text", "ascii") else None
    idx, src, _ = _built(eng, name, parallel)
    size, pts = len(plain), idx.points
    ranges = _ranges(pts, size, 11)
    got = idx.read_many(src, ranges)
    for (off, n), (st, data) in zip(ranges, got):
        assert st == OK and data == plain[off:off + n], (off, n, st)
    stats = idx.last_stats()
    assert stats["launches"] == 1 and stats["pieces"] == len(_pieces_of(pts, size, ranges)) == len([p for p in pts if p[1] < size])
    assert 0 < stats["bytes_in"] <= len(src) + len(pts) and stats["bytes_windows"] == sum(min(32768, o) for _, o in pts if o < size)
    # a few ranges touch a few pieces: only those are decoded, only their bytes cross
    if len(pts) >= 4:
        few = [(pts[2][1] + 7, 100), (pts[2][1] + 9, 5000)]
        assert [d for _, d in idx.read_many(src, few)] == [plain[o:o + n] for o, n in few]
        stats = idx.last_stats()
        assert stats["pieces"] == len(_pieces_of(pts, size, few)) == 1 and stats["bytes_in"] <= (pts[3][0] + 7) // 8 - pts[2][0] // 8
    assert idx.read(src, 3, 20) == plain[3:23] and idx.read_many(src, []) == []


def test_serially_built_index_reads_the_same(eng):
    raw, plain, _ = _input("text")
    idx, src, _ = _built(eng, "text", False)
    assert idx.read(src, 0, len(plain)) == plain


def test_hand_built_stream_with_matches_that_reach_32768_back(eng):
    rng = random.Random(5)
    head = [rng.randrange(256) for _ in range(32768 + 5)]
    fixed = [dw.match(258, 32768), dw.match(3, 1)] + [dw.match(258, 32768)] * 16 + [rng.randrange(256) for _ in range(300)]
    dyn = [dw.match(200, 32768)] + [rng.randrange(97, 123) for _ in range(900)] + [dw.match(258, 32768), dw.match(258, 1)] * 20
    blocks = [dw.Block("stored", head), dw.Block("fixed", fixed), dw.Block("dynamic", dyn)]
    raw = dw.write(blocks)
    st, plain = dw.expand(blocks)
    assert st == 0 and zlib.decompress(raw, -15) == plain
    starts = block_starts(raw)[0]
    assert len(starts) == 3 and starts[1][1] == 32773 and starts[2][1] - starts[1][1] >= 4096
    idx = _Index().build(raw, FMT_RAW, span=4096)
    assert _check_points(idx, plain, starts, 0, 4096) == starts  # both Huffman block starts are points
    ranges = [(0, len(plain)), (32773 - 3, 600), (starts[2][1] - 100, 400), (32773, 258), (starts[2][1], 200), (32770, len(plain) - 32770)]
    for (off, n), (st, data) in zip(ranges, idx.read_many(raw, ranges)):
        assert st == OK and data == plain[off:off + n], (off, n)


def test_rounds_at_the_smallest_workspace(eng):
    raw, plain, _ = _input("text")
    idx, src, _ = _built(eng, "text", True)
    for bad in (-1, (1 << 20) + 1):
        assert eng.lib.md_set_option(eng.ctx, b"index_read_workspace", bad) == -1
    eng.set_option("index_read_workspace", 0)
    try:
        assert idx.read(src, 0, len(plain)) == plain
        stats = idx.last_stats()
        assert stats["launches"] == stats["pieces"] == len(idx.points) >= 2
        ranges = _ranges(idx.points, len(plain), 3)
        assert [d for _, d in idx.read_many(src, ranges)] == [plain[o:o + n] for o, n in ranges]
        eng.set_option("index_read_workspace", 1)
        assert idx.read(src, 0, len(plain)) == plain and idx.last_stats()["launches"] == 1
    finally:
        eng.set_option("index_read_workspace", 256)


def test_save_load_read(eng):
    raw, plain, _ = _input("ascii")
    idx, src, _ = _built(eng, "ascii", True, FMT_GZIP)
    blob = idx.dumps()
    again = _Index().loads(blob)
    assert again.dumps() == blob and again.info == idx.info and again.points == idx.points
    ranges = _ranges(idx.points, len(plain), 23)
    assert again.read_many(src, ranges) == idx.read_many(src, ranges) == [(OK, plain[o:o + n]) for o, n in ranges]


def _piece_ranges(pts, size):
    """one range per piece, and ranges across every point"""
    outs = [o for _, o in pts] + [size]
    r = [(outs[k], outs[k + 1] - outs[k]) for k in range(len(pts))]
    return r + [(o - 50, 100) for o in outs[1:-1]]


def test_one_flipped_byte_fails_its_piece_alone(eng):
    raw, plain, _ = _input("text")
    idx, src, _ = _built(eng, "text", True)
    pts = idx.points
    assert len(pts) >= 5
    # the byte behind the one piece 3 begins in holds bits of its dynamic block's header (HLIT, HDIST, HCLEN): all of them
    # change, so the tables are others and the block cannot end where the next point says; piece 2 ends in front of it
    at = pts[3][0] // 8 + 1
    bad = src[:at] + bytes([src[at] ^ 0xff]) + src[at + 1:]
    ranges = _piece_ranges(pts, len(plain))
    got = idx.read_many(bad, ranges)
    for (off, n), (st, data) in zip(ranges, got):
        if 3 in _pieces_of(pts, len(plain), [(off, n)]):
            assert st != OK, (off, n)
        else:
            assert st == OK and data == plain[off:off + n], (off, n, st)
    assert idx.read(src, 0, len(plain)) == plain  # (and the index is as good as before)


def test_moved_point_fails_the_pieces_on_both_sides(eng):
    raw, plain, _ = _input("text")
    idx, src, _ = _built(eng, "text", True)
    pts = idx.points
    blob = bytearray(idx.dumps())
    struct.pack_into("<Q", blob, 72 + 24 * 3, pts[3][0] + 1)
    moved = _Index().loads(bytes(blob))  # (it still passes every rule of the layout)
    assert moved.points[3] == (pts[3][0] + 1, pts[3][1])
    ranges = _piece_ranges(pts, len(plain))
    for (off, n), (st, data) in zip(ranges, moved.read_many(src, ranges)):
        hit = _pieces_of(pts, len(plain), [(off, n)])
        if hit & {2, 3}:
            assert st != OK, (off, n)
        else:
            assert st == OK
        assert st != OK or data == plain[off:off + n]
    st2 = moved.read_many(src, [(pts[2][1], 10)])[0][0]
    assert st2 == INVALID_INDEX  # (piece 2 decodes well, and ends one bit in front of the point)


def test_read_refuses_another_src_and_ranges_behind_the_end(eng):
    from decompress_amd import engine
    raw, plain, _ = _input("text")
    idx, src, _ = _built(eng, "text", True)
    with pytest.raises(engine.Error, match="Invalid index"):
        idx.read_many(src + b"\0", [(0, 1)])
    with pytest.raises(engine.Error, match="Invalid index"):
        idx.read_many(src[:-1], [(0, 1)])
    for off, n in ((len(plain), 1), (len(plain) - 1, 2), (1 << 63, 1 << 63), ((1 << 64) - 1, 2)):
        with pytest.raises(engine.Error, match="Invalid argument"):
            idx.read_many(src, [(0, 1), (off, n)])
    assert idx.read_many(src, [(len(plain), 0), (len(plain) - 1, 1)]) == [(OK, b""), (OK, plain[-1:])]
    for off, n in ((-1, 2), (0, -1), (1 << 64, 1)):
        with pytest.raises(engine.Error, match="Invalid argument"):
            idx.read_many(src, [(off, n)])


def test_conveniences(eng):
    from decompress_amd import de, gz, zl
    raw, plain, _ = _input("ascii")
    for mod, fmt in ((de, FMT_RAW), (zl, FMT_ZLIB), (gz, FMT_GZIP)):
        src, _ = _frame(raw, plain, fmt)
        idx = mod.index(src, span=SPAN)
        assert idx.info["format"] == fmt and idx.read(src, 1000, 70000) == plain[1000:71000]
