"""The decoder's size query on the GPU (md_inflate_sizes_batch_device, md_inflate_plan_device): every stream's
inflated size without decoding it.  The yardsticks are libz, the CPU oracle and the token writer's expand(), never the
library's own decode - except where a test says that the planned decode equals the decode with generous room.

The contract (mdeflate.h), R being the decode with room that never runs out: R OK -> the same status, size and consumed;
R Invalid_checksum -> OK (GZIP: Invalid input size when ISIZE is wrong too), R's size, the consumed a correct checksum
would give; any other R -> the same status, consumed 0, the bytes in front of the failing token."""
import functools
import random
import zlib

import numpy as np
import pytest

from decompress_amd import workloads
from tests.conftest import load_golden
from tests.deflate_writer import Block, expand, write
from tests.test_gpu_fuzz import _corrupt, _plain
from tests.test_gpu_inflate import tiny_block_streams
from tests.test_gpu_inflate_rounds import FAMILIES, _raw

pytestmark = pytest.mark.gpu

DE, ZL, GZ = 0, 1, 2
OK, END_OF_INPUT, END_OF_OUTPUT, DISTANCE, CHECKSUM, SIZE = 0, 1, 2, 6, 9, 12


@pytest.fixture(scope="module")
def eng():
    import decompress_amd
    return decompress_amd.Engine(0)


def _upload(eng, streams):
    import torch
    blob, offs, lens = workloads.pack([bytes(s) for s in streams])
    t = lambda a: torch.from_numpy(a).to(eng.device)
    d = (t(blob), t(offs), t(lens))
    torch.cuda.synchronize(eng.device)
    return d


def _sizes(eng, fmt, streams):
    """[(status, consumed, out_len)] of the device form"""
    import torch
    d_in, d_off, d_len = _upload(eng, streams)
    out_len, consumed, status = eng.inflate_sizes(fmt, d_in, d_off, d_len)
    eng.synchronize()
    torch.cuda.synchronize(eng.device)
    out_len, consumed, status = out_len.cpu().numpy(), consumed.cpu().numpy(), status.cpu().numpy()
    return [(int(status[i]), int(consumed[i]), int(out_len[i])) for i in range(len(streams))]


def _gz(raw, plain, crc=None, isize=None):
    crc = zlib.crc32(plain) if crc is None else crc
    isize = len(plain) & 0xffffffff if isize is None else isize
    return b"\x1f\x8b\x08\x00\0\0\0\0\x00\x03" + raw + crc.to_bytes(4, "little") + isize.to_bytes(4, "little")


def _frames(raw, plain):
    return {DE: raw, ZL: b"\x78\x9c" + raw + zlib.adler32(plain).to_bytes(4, "big"), GZ: _gz(raw, plain)}


@functools.lru_cache(None)
def _kinds():
    """(format, stream, garbage behind it, plaintext length): the corpus at levels 1 / 6 / 9 / 0 and Z_FIXED"""
    rng = random.Random(11)
    out = []
    for data in workloads.corpus().values():
        for level, strat in ((1, 0), (6, 0), (9, 0), (0, 0), (6, zlib.Z_FIXED)):
            co = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strat)
            raw = co.compress(data) + co.flush()
            for fmt, s in _frames(raw, data).items():
                junk = bytes(rng.getrandbits(8) for _ in range(rng.randrange(1, 101))) if rng.random() < 0.4 else b""
                out.append((fmt, s, junk, len(data)))
    return out


def test_kinds(eng):
    """1. every kind of block, raw / zlib / gzip, some with bytes behind the stream"""
    for fmt in (DE, ZL, GZ):
        cases = [c for c in _kinds() if c[0] == fmt]
        assert len(cases) == 75
        res = _sizes(eng, fmt, [c[1] + c[2] for c in cases])
        for k, ((_, s, junk, n), r) in enumerate(zip(cases, res)):
            assert r == (OK, len(s), n), (fmt, k, len(junk), r, len(s), n)


@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_round_limits(eng, fam):
    """2. the hand-built streams at the decoder's round limits: sizes and statuses are expand()'s with unlimited room"""
    cases = FAMILIES[fam]()
    uniq = {id(c[1]): c for c in cases}.values()  # (a family lists a stream once per output cap)
    res = _sizes(eng, DE, [_raw(c[1]) for c in uniq])
    for (name, blocks, _, _), (st, used, n) in zip(uniq, res):
        est, eout = expand(blocks)
        assert (st, n) == (est, len(eout)), (name, st, n, est, len(eout))
        assert used == (len(_raw(blocks)) if est == OK else 0), name


def test_runs_of_tiny_blocks(eng, oracle):
    """2b. runs of empty fixed blocks and flush points (the decode test's streams, raw, one batch): the block loop walks them
    through the window it has in LDS, past the window's end and the limit of its reuse in the runs of 1700, 1800 and 5000"""
    _, cases = tiny_block_streams()
    res = _sizes(eng, DE, [src for src, _, _ in cases])
    assert len(res) == len(cases)
    for (src, _, plain_len), r in zip(cases, res):
        ost, oused, oout = oracle.de_inflate(src, plain_len + 16)  # room that never runs out
        assert r == ((OK, oused, len(oout)) if ost == OK else (ost, 0, len(oout))), (len(src), plain_len, r, ost, oused, len(oout))


def test_rounds_beyond_the_packed_count(eng):
    """3. two bits a 258-byte match: one round is more than 2^20 bytes, which the walks' packed count cannot hold"""
    plains = [bytes(n << 20) for n in (1, 4, 8)]
    assert [len(zlib.compress(p, 9)) for p in plains] == [1039, 4086, 8163]
    for period in (2, 3, 4):
        plains.append(bytes(range(1, period + 1)) * ((3 << 20) // period))
    plains.append(workloads.text(5, 300000))
    plains.append(bytes(1 << 20) + workloads.text(6, 100000) + bytes(2 << 20))
    streams = [zlib.compress(p, 9) for p in plains]
    res = _sizes(eng, ZL, streams)
    for p, s, r in zip(plains, streams, res):
        assert r == (OK, len(s), len(p)), (len(p), r)


def _distance_cases():
    """4. one match whose distance is exactly the output position (fine) or one more (Invalid_distance), at positions on
    both sides of 32 KiB.  Each position is reached three ways: by stored blocks, so that the match is its block's first
    token; by literals of the match's own block, so that the match lies deep in a round (about 60 zones in where the
    position allows 2 000 literals, else as many literals as the position has bytes: a token cannot produce less than a
    byte); and directly behind a stored block of 1 000 and of 33 000 bytes."""
    rng = random.Random(44)
    lits = lambda n: [rng.randrange(256) for _ in range(n)]

    def stored(n):
        out = []
        while n > 0:
            out.append(Block("stored", lits(min(n, 65535))))
            n -= min(n, 65535)
        return out

    cases = []
    spots = [(1, 1), (1, 2), (257, 257), (257, 258), (32767, 32767), (32767, 32768), (32768, 32768), (40000, 32768)]
    spots += [(1000, 1000), (1000, 1001), (33000, 32768)]
    for pos, d in spots:
        tail = [(3, d)] + lits(20)
        cases.append(("first pos %d d %d" % (pos, d), stored(pos) + [Block("dynamic", tail)]))
        if pos not in (1000, 33000):
            deep = min(pos, 2000)
            cases.append(("deep pos %d d %d" % (pos, d), stored(pos - deep) + [Block("dynamic", lits(deep) + tail)]))
    return cases


def test_distance_rule(eng):
    cases = _distance_cases()
    res = _sizes(eng, DE, [write(b) for _, b in cases])
    seen = set()
    for (name, blocks), (st, used, n) in zip(cases, res):
        est, eout = expand(blocks)
        pos = int(name.split()[2])
        assert est in (OK, DISTANCE) and (est == OK or len(eout) == pos), name
        assert (st, n) == (est, len(eout)), (name, st, n, est, len(eout))
        assert used == (len(write(blocks)) if est == OK else 0), name
        seen.add(est)
    assert seen == {OK, DISTANCE}


def test_reference_vectors(eng):
    """5. the reference's own test vectors; the one whose error is the output running out has no counterpart here"""
    ns, stream = load_golden("inflate_ns.json"), load_golden("inflate_stream.json")
    skip = lambda c: str(c.get("error", "")).replace(" ", "_").lower() == "unexpected_end_of_output"
    counted = sum(1 for c in ns + stream if c["status"] == END_OF_OUTPUT)
    keep_ns, keep_st = [c for c in ns if not skip(c)], [c for c in stream if not skip(c)]
    assert len(ns) + len(stream) - len(keep_ns) - len(keep_st) == counted == 1
    res = _sizes(eng, DE, [bytes.fromhex(c["src"]) for c in keep_ns + keep_st])
    for c, (st, used, n) in zip(keep_ns + keep_st, res):
        assert st == c["status"], (c["name"], st)
        if st == OK:
            want = c["written"] if "written" in c else len(bytes.fromhex(c["dst"]))
            assert n == want, c["name"]
            if "consumed" in c:
                assert used == c["consumed"], c["name"]
        else:
            assert used == 0, c["name"]


def _fuzz_streams(fmt, count, seed):
    rng = random.Random(seed)
    srcs = []
    for _ in range(count * 7 // 20 if fmt == DE else 0):  # pure garbage (test_gpu_fuzz's first loop)
        n = rng.choice((0, 1, 2, 3, 5, 8, 13, 40, 200, 1500))
        g = bytearray(rng.getrandbits(8) for _ in range(n))
        if g and rng.random() < 0.7:
            g[0] = (g[0] & 0xf8) | rng.choice((1, 3, 5, 4, 2, 0))
        srcs.append(bytes(g))
    while len(srcs) < count:  # corrupted valid streams of every block kind
        data = _plain(rng, rng.choice((0, 1, 50, 700, 5000, 40000)))
        strat = rng.choice((zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE))
        co = zlib.compressobj(rng.choice((0, 1, 6, 9)), zlib.DEFLATED, -15, rng.choice((1, 8, 9)), strat)
        z = _frames(co.compress(data) + co.flush(), data)[fmt]
        srcs.append(_corrupt(rng, z) if rng.random() < 0.85 else z)
    return srcs


def _oracle(oracle, fmt, src, cap):
    if fmt == DE:
        return oracle.de_inflate(src, cap)
    if fmt == ZL:
        return oracle.zl_inflate(src, cap)
    return oracle.gz_inflate(src, cap)[:3]


def _check_contract(oracle, fmt, src, got, ref):
    """one stream's (status, consumed, out_len) against R = (status, consumed, bytes) of the oracle with plenty of room"""
    st, used, n = got
    ost, oused, oout = ref
    assert ost != END_OF_OUTPUT, "1032 x the input + 1 024 is more than any stream of that length inflates to"
    if ost == OK:
        assert got == (OK, oused, len(oout)), (fmt, got, ost, oused, len(oout))
    elif ost == CHECKSUM:
        assert n == len(oout), (fmt, got, len(oout))
        assert st in ((OK, SIZE) if fmt == GZ else (OK,)), (fmt, got)
        if st == SIZE:
            assert used == 0
            return
        # the consumed a correct checksum would have given: put the right checksum there and ask the oracle
        fixed = bytearray(src)
        if fmt == ZL:
            fixed[used - 4:used] = zlib.adler32(oout).to_bytes(4, "big")
        else:
            fixed[used - 8:used - 4] = zlib.crc32(oout).to_bytes(4, "little")
        fst, fused, fout = _oracle(oracle, fmt, bytes(fixed), len(oout) + 16)
        assert (fst, fused, fout) == (OK, used, oout), (fmt, got, fst, fused)
    else:
        assert got == (ost, 0, len(oout)), (fmt, got, ost, len(oout))


@pytest.mark.parametrize("fmt", [DE, ZL, GZ])
def test_fuzz_contract(eng, oracle, fmt):
    """6. garbage and corrupted streams (the generators of test_gpu_fuzz), 2 000 per format"""
    srcs = _fuzz_streams(fmt, 2000, 20261017 + fmt)
    res = _sizes(eng, fmt, srcs)
    seen = set()
    for k, (src, got) in enumerate(zip(srcs, res)):
        ref = _oracle(oracle, fmt, src, 1032 * len(src) + 1024)
        try:
            _check_contract(oracle, fmt, src, got, ref)
        except AssertionError as e:
            raise AssertionError("stream %d of format %d (%d bytes): %s" % (k, fmt, len(src), e))
        seen.add(ref[0])
    if fmt == DE:
        assert seen >= {0, 1, 3, 4, 5, 6, 7}, seen  # every De.Inf.Ns error variant but the output's
    else:
        assert CHECKSUM in seen and OK in seen, seen


def _mixed(n):
    rng = random.Random(7000 + n)
    kinds = [c[1] + c[2] for c in _kinds() if c[0] == DE and len(c[1]) < 60000]
    bad = _fuzz_streams(DE, 300, 9)
    empty = [zlib.compressobj(6, zlib.DEFLATED, -15).flush(), b"\x03\x00", b"\x01\x00\x00\xff\xff"]
    pool = kinds + bad + empty
    if n == 1:
        return [kinds[3]]
    small = [s for s in pool if len(s) < 4000]
    return [rng.choice(pool if k < 150 else small) for k in range(n)]


@pytest.mark.parametrize("n", [1, 5000])
@pytest.mark.parametrize("align", [1, 256])
def test_plan_and_decode(eng, oracle, n, align):
    """7. sizes -> plan -> decode into the planned ranges: disjoint, aligned, and every result equal to the decode with
    generous room and to the oracle - failed streams included (every other check of a token precedes the output check)"""
    import torch
    streams = _mixed(n)
    d_in, d_off, d_len = _upload(eng, streams)
    sizes, s_used, s_st = eng.inflate_sizes(DE, d_in, d_off, d_len)
    out_off, out_cap, total = eng.inflate_plan(sizes, align)
    eng.synchronize()
    torch.cuda.synchronize(eng.device)
    tot = int(total.item())
    off, cap, sz = out_off.cpu().numpy(), out_cap.cpu().numpy(), sizes.cpu().numpy()
    assert (cap == sz).all() and (off % align == 0).all() and off[0] == 0
    ends = off + (cap + align - 1) // align * align
    assert (off[1:] == ends[:-1]).all() and tot == ends[-1]  # back to back, so disjoint; the total is the last end
    d_out = torch.zeros(tot + 16, dtype=torch.uint8, device=eng.device)
    torch.cuda.synchronize(eng.device)
    out_len, consumed, status, checksum = eng.inflate_batch(DE, d_in, d_off, d_len, d_out, out_off, out_cap)
    eng.synchronize()
    torch.cuda.synchronize(eng.device)
    out = d_out.cpu().numpy()
    out_len, consumed, status = out_len.cpu().numpy(), consumed.cpu().numpy(), status.cpu().numpy()
    checksum = checksum.cpu().numpy().view(np.uint32)
    s_used, s_st = s_used.cpu().numpy(), s_st.cpu().numpy()
    roomy = eng.inflate_many(streams, [int(x) + 300 for x in sz])
    refs = {}
    for i, s in enumerate(streams):
        got = (int(status[i]), int(consumed[i]), out[off[i]:off[i] + out_len[i]].tobytes(), int(checksum[i]))
        assert got == roomy[i], (i, got[:2], roomy[i][:2], len(got[2]), len(roomy[i][2]))
        if s not in refs:
            refs[s] = oracle.de_inflate(s, int(sz[i]) + 300)
        assert got[:3] == refs[s], (i, got[:2], refs[s][:2])
        assert (int(s_st[i]), int(s_used[i]), int(sz[i])) == (got[0], got[1], len(got[2])), i
        if got[0] == OK:
            assert got[3] == zlib.adler32(got[2]), i


def test_many_streams(eng):
    """8. more streams than a grid dimension of 65 535 holds"""
    import torch
    rng = random.Random(8)
    uniq = [bytes(rng.choice(b"abcdefgh \n") for _ in range(k)) for k in range(1, 201)]
    z = [zlib.compress(p, 6) for p in uniq]
    pick = [rng.randrange(200) for _ in range(70000)]
    streams = [z[k] for k in pick]
    want = np.array([k + 1 for k in pick], dtype=np.int64)
    d_in, d_off, d_len = _upload(eng, streams)
    sizes, used, st = eng.inflate_sizes(ZL, d_in, d_off, d_len)
    out_off, out_cap, total = eng.inflate_plan(sizes, 64)
    eng.synchronize()
    torch.cuda.synchronize(eng.device)
    assert (st.cpu().numpy() == 0).all() and (sizes.cpu().numpy() == want).all()
    assert (used.cpu().numpy() == np.array([len(s) for s in streams])).all()
    padded = (want + 63) // 64 * 64
    assert (out_cap.cpu().numpy() == want).all()
    assert (out_off.cpu().numpy() == np.cumsum(padded) - padded).all() and int(total.item()) == int(padded.sum())


def test_beyond_4_gib(eng):
    """9. 65 x 64 MiB of zeros and three bytes: more than 32 bits of output is a size like any other"""
    co = zlib.compressobj(9, zlib.DEFLATED, -15)
    chunk = co.compress(bytes(64 << 20)) + co.flush(zlib.Z_FULL_FLUSH)
    assert len(chunk) == 65236
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    tail = co.compress(b"abc") + co.flush()
    d = zlib.decompressobj(-15)
    n = sum(len(d.decompress(piece)) for piece in (chunk, chunk, chunk, tail))
    assert d.eof and n == 3 * (64 << 20) + 3
    stream = chunk * 65 + tail
    assert _sizes(eng, DE, [stream, tail]) == [(OK, len(stream), 65 * (1 << 26) + 3), (OK, len(tail), 3)]


def test_python_surface(eng):
    """10. inflate_many without caps, and inflated_size of the three modules"""
    from decompress_amd import de, gz, zl
    streams = [c[1] for c in _kinds() if c[0] == DE][:20] + _fuzz_streams(DE, 60, 3)
    sized = eng.inflate_many(streams)
    caps = [len(r[2]) for r in sized]
    assert sized == eng.inflate_many(streams, caps)
    assert any(r[0] != OK for r in sized) and any(r[0] == OK and r[2] for r in sized)
    plain = workloads.text(3, 50000)
    raw = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = raw.compress(plain) + raw.flush()
    f = _frames(raw, plain)
    for mod, fmt in ((de, DE), (zl, ZL), (gz, GZ)):
        assert mod.inflated_size(f[fmt]) == ("Ok", (len(f[fmt]), len(plain)))
        assert mod.inflated_size(f[fmt][:len(f[fmt]) // 2]) == ("Error", "Unexpected_end_of_input")
    assert gz.inflated_size(_gz(raw, plain, isize=7)) == ("Error", "Invalid input size")
    assert gz.inflated_size(_gz(raw, plain, crc=1)) == ("Ok", (len(f[GZ]), len(plain)))  # the CRC-32 is not looked at
