"""Every place of the library that computes an Adler-32 or a CRC-32, on the texts of tests/checksum_cases.py: sums that start a
step in state (65520, 65520) on bytes of 0xFF, checksums whose a or b is 0 mod 65521, lengths that are 0 mod 65521, one set
byte at every edge of the summing geometry, CRCs of 0 and ~0, every length of crc32_wave's lane geometry, and trailers that
are congruent to the right value without being it.  The yardstick is always zlib.adler32 / zlib.crc32 of the text (with the
seed where there is one), compared for equality - next to the status and the bytes.  Needs an MI355X: `pytest -m gpu`.

The long-stream decoder falls back to the serial one when its own checksum does not match the trailer, so a wrong segment sum
or join there gives right bytes: what shows it is `inflate_parallel_last` reporting no pieces for a valid frame."""
import ctypes
import io
import os
import re
import struct
import zipfile
import zlib

import numpy as np
import pytest

from tests import checksum_cases as cc
from tests import long_stream_cases as lc
from tests import test_gpu_inf_batch as gb
from tests import test_gpu_inflate as gi
from tests import test_gpu_long_stream as gl
from tests import test_gpu_zip as gz_
from tests import zip_util as zu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFLATE, ZLIB, GZIP = 0, 1, 2
WBITS = {"zl": 15, "gz": 31}
FORMAT = {"zl": ZLIB, "gz": GZIP}


def _status(name):
    hdr = open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    return int(re.search(r"\b%s\s*=\s*(\d+)" % name, hdr).group(1))


OK, END_OF_INPUT, END_OF_OUTPUT = _status("MD_OK"), _status("MD_UNEXPECTED_END_OF_INPUT"), _status("MD_UNEXPECTED_END_OF_OUTPUT")
BAD = {"checksum": _status("MD_INVALID_CHECKSUM"), "size": _status("MD_INVALID_SIZE")}


@pytest.fixture(scope="module")
def eng():
    import decompress_amd
    return decompress_amd.Engine(0)


def _sum(fmt, data, seed=None):
    if fmt in ("gz", GZIP):
        return zlib.crc32(data)
    return zlib.adler32(data) if seed is None else zlib.adler32(data, seed)


def _frame(fmt, data, level):
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[fmt])
    return c.compress(data) + c.flush()


def _raw(data, level):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def _first_diff(a, b):
    return next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), min(len(a), len(b)))


# ---- 1. batch inflate -------------------------------------------------------------------------------------------------------
def _inflate_texts():
    return (cc.top_texts() + [("slice-top", cc.slice_top())] + cc.unit_texts() + cc.one_hot() + cc.long_texts() + cc.forged_texts()
            + cc.forged_embedded_texts() + [("units-%s-x3" % k, cc.units(k, 65521, 3) + b"\0") for k in cc.KINDS])


@pytest.mark.parametrize("fmt", ["zl", "gz"])
def test_batch_inflate(eng, fmt):
    """Sink::flush's Adler-32 (csrc/inflate_wave.hip) and the quarter-chunk CRCs of csrc/inflate_batch.hip: every text as
    stored blocks and at level 6, and every bad trailer, in one batch"""
    frames, plains, names, want = [], [], [], []
    for name, t in _inflate_texts():
        for level in (0, 6):
            frames.append(_frame(fmt, t, level))
            plains.append(t)
            names.append("%s level %d" % (name, level))
            want.append(OK)
    for plain in (cc.SMALL_SUM_TEXT, cc.small_sum_long(200000)):
        for raw in (cc.stored_body(plain), _raw(plain, 6)):
            for name, f, frame, what in cc.bad_trailers(plain, raw):
                if f == fmt:
                    frames.append(frame)
                    plains.append(plain)
                    names.append("%s, %d bytes in %d" % (name, len(plain), len(raw)))
                    want.append(BAD[what])
    res = eng.inflate_many(frames, [len(p) for p in plains], FORMAT[fmt])
    assert want.count(OK) == 2 * len(_inflate_texts()) and len(want) - want.count(OK) == (28 if fmt == "zl" else 16)
    for name, frame, plain, w, (st, used, out, ck) in zip(names, frames, plains, want, res):
        assert st == w, (name, st)
        assert len(out) == len(plain) and out == plain, (name, _first_diff(out, plain))
        assert ck == _sum(fmt, plain), (name, hex(ck))
        if w == OK:
            assert used == len(frame), name


# ---- 2. the continue path ---------------------------------------------------------------------------------------------------
def _seeded_bodies():
    """(name, seed, data, a body of stored blocks of 65535 bytes, the blocks' starts in the output)"""
    out = []
    for name, seed, d in cc.seeded():
        starts = list(range(0, len(d), 65535))
        raw = b"".join(lc.stored_unit(d[c:c + 65535], last=c == starts[-1]).raw for c in starts)
        out.append((name, seed, d, raw, starts))
    return out


def _cut(d, starts):
    """bytes to drop from the end of the body so that it ends inside the last stored block (behind its five-byte header)"""
    assert len(d) > starts[-1]
    return min(100, len(d) - starts[-1])


@pytest.mark.parametrize("parallel", [False, True], ids=["serial", "pieces"])
def test_continue_host_seeded(eng, parallel):
    """md_de_inf_continue_host from every seed: Sink::flush seeded from adler_in (serial) and par_adler's join from it (a
    body of 16 KiB and more, in pieces of 4 KiB); whole, and cut inside the last block"""
    took = 0
    for name, seed, d, raw, starts in _seeded_bodies():
        with gl._path(eng, parallel=parallel):
            st, n, new, rs = gi._continue(eng, raw, 0, b"", len(d), seed)
            took += gl._par_last(eng)[0] > 0
        assert (st, n) == (OK, len(d)) and new == d, name
        assert rs.last == 1 and rs.out == len(d) and rs.consumed == len(raw), name
        assert rs.checksum == rs.adler == zlib.adler32(d, seed), (name, hex(rs.checksum))
        assert rs.crc_end == rs.crc_out == zlib.crc32(d), name
        if len(starts) > 1:  # cut short inside the last block's bytes: the boundary in front of that block is the resume point
            with gl._path(eng, parallel=parallel):
                st, n, new, rs = gi._continue(eng, raw[:-_cut(d, starts)], 0, b"", len(d), seed)
            assert st == END_OF_INPUT and rs.out == starts[-1] and d.startswith(new) and len(new) >= rs.out, name
            assert rs.adler == zlib.adler32(d[:rs.out], seed), (name, hex(rs.adler))
            assert rs.crc_out == zlib.crc32(d[:rs.out]) and rs.crc_end == zlib.crc32(new), name
    assert (took > 0) == parallel


def test_continue_batch_seeded(eng):
    """md_inflate_continue_batch_device: every seeded text whole (stored and level 6) and cut inside its last stored block, one
    launch: the checksum from the seed, and resume_adler at the last block boundary"""
    import torch
    rows = []  # (name, seed, data, piece, the output the last complete block ends at, or None for a whole stream)
    for name, seed, d, raw, starts in _seeded_bodies():
        rows.append((name, seed, d, raw, None))
        rows.append((name + " level 6", seed, d, _raw(d, 6), None))
        if len(starts) > 1:
            rows.append((name + " cut", seed, d, raw[:-_cut(d, starts)], starts[-1]))
    n = len(rows)
    dev = eng.device
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    pad = lambda x: x + b"\0" * (-len(x) % 16)
    pieces = [r[3] for r in rows]
    in_off = np.cumsum([0] + [len(pad(x)) for x in pieces[:-1]]).astype(np.int64)
    caps = [(len(r[2]) + 255) // 256 * 256 + 256 for r in rows]
    out_off = np.cumsum([0] + caps[:-1]).astype(np.int64)
    d_in = torch.from_numpy(np.frombuffer(b"".join(pad(x) for x in pieces) + bytes(16), dtype=np.uint8).copy()).to(dev)
    d_out = torch.zeros(int(sum(caps)) + 16, dtype=torch.uint8, device=dev)
    i32 = lambda v: v - (1 << 32) if v >= 1 << 31 else v
    args = [t(in_off, torch.int64), t([len(x) for x in pieces], torch.int64), d_out, t(out_off, torch.int64), t([len(r[2]) for r in rows], torch.int64),
            t([0] * n, torch.int32), t([0] * n, torch.int32), t([i32(r[1]) for r in rows], torch.int32)]
    out_len, consumed = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    status, checksum = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    r_bits, r_out = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    r_adl, r_last = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    eng._check(eng.lib.md_inflate_continue_batch_device(eng.ctx, n, p(d_in), *[p(x) for x in args], p(out_len), p(consumed), p(status),
                                                        p(checksum), p(r_bits), p(r_out), p(r_adl), p(r_last)))
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    u32 = lambda x: [v & 0xffffffff for v in x.cpu().tolist()]
    status, out_len, r_out, r_adl, checksum = status.cpu().tolist(), out_len.cpu().tolist(), r_out.cpu().tolist(), u32(r_adl), u32(checksum)
    for i, (name, seed, d, piece, upto) in enumerate(rows):
        got = out[out_off[i]:out_off[i] + out_len[i]].tobytes()
        if upto is None:
            assert status[i] == OK and got == d, (name, status[i])
            assert checksum[i] == zlib.adler32(d, seed), (name, hex(checksum[i]))
        else:
            assert status[i] == END_OF_INPUT and r_out[i] == upto and d.startswith(got), (name, status[i], r_out[i])
            assert r_adl[i] == zlib.adler32(d[:upto], seed), (name, hex(r_adl[i]))


# ---- 3. streaming decoders --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["zl", "gz"])
def test_streaming_decoders(eng, fmt):
    """md_inf_batch_*: `top` and the forged texts, a byte a round (level 6: the frames are short) and in pieces of 4097 and
    65536 bytes (stored blocks: the pieces are pieces of the text)"""
    texts = cc.top_texts() + cc.forged_texts() + cc.forged_embedded_texts()
    plans, plains, names = [], [], []
    for name, t in texts:
        z6, z0 = _frame(fmt, t, 6), _frame(fmt, t, 0)
        for z, piece in ((z6, 1), (z0, 4097), (z0, 65536)):
            if piece == 1 and len(z) >= 2000:  # (the embedded forged text: 61 KiB of random bytes)
                assert name.startswith("forged-embedded")
                continue
            plans.append([z[i:i + piece] for i in range(0, len(z), piece)])
            plains.append(t)
            names.append("%s in pieces of %d" % (name, piece))
    assert max(len(pl) for pl in plans) < 2000
    res, rounds, launches, _ = gb.run_batch(eng, FORMAT[fmt], plans)
    for name, plain, (sig, st, msg, out, ck, rem) in zip(names, plains, res):
        assert (sig, st, rem) == (gb.END, OK, 0), (name, sig, st, msg)
        assert out == plain, (name, _first_diff(out, plain))
        assert ck == _sum(fmt, plain), (name, hex(ck))
    k = names.index("top-4097 in pieces of 4097")
    assert gb.run_single(eng, FORMAT[fmt], plans[k]) == res[k]  # md_inf_* on the same pieces


# ---- 4. long-stream inflate -------------------------------------------------------------------------------------------------
LONG_MIN = lc.HIGHER_MIN + 4096


def _stored_raw(plain):
    """`plain` in stored blocks of 60001 bytes behind as many empty stored blocks as make the body at least LONG_MIN bytes
    long: the *_higher_uncompress entry points hand a stream to the pieces from lc.HIGHER_MIN bytes of input on"""
    cuts = list(range(0, len(plain), 60001))
    body = b"".join(lc.stored_unit(plain[c:c + 60001], last=c == cuts[-1]).raw for c in cuts)
    empty = lc.stored_unit(b"").raw
    return empty * max(0, (LONG_MIN - len(body) + len(empty) - 1) // len(empty)) + body


def _long_texts():
    out = [("top-200000", cc.top(200000)), ("slice-top", cc.slice_top())]
    out += [(nm, t) for nm, t in cc.one_hot() if len(t) == 65536 + 257]
    lens = (65535, 65536, 65537, 262144 + 4097, (1 << 20) + 1, (2 << 20) + 17)
    out += [("random-%d" % n, cc.long_random(n)) for n in lens] + [("zero-%d" % n, cc.long_zero(n)) for n in lens]
    return out + [("units-%s-x3" % k, cc.units(k, 65521, 3) + b"\0") for k in cc.KINDS]


def test_long_stream_through_the_pieces(eng):
    """adler_segments_kernel + par_adler and par_crc's join of 1 MiB pieces (csrc/capi_long_stream.cpp): the frame must come
    back THROUGH the pieces, which it only does when the path's own checksum equals the trailer"""
    for name, plain in _long_texts():
        raw = _stored_raw(plain)
        assert len(raw) >= LONG_MIN and zlib.decompress(raw, -15) == plain
        for fmt in ("zl", "gz"):
            src = lc.frame(raw, plain, fmt)
            with gl._path(eng):
                st, used, out = gl._higher(eng, fmt, src, len(plain))
                pieces, rounds = gl._par_last(eng)
            print("long stream: %-28s %s %8d bytes in %8d: status %d, %d pieces in %d round(s)" % (name, fmt, len(plain), len(src), st, pieces, rounds))
            assert st == OK and len(out) == len(plain), (name, fmt, st)
            assert out == plain, (name, fmt, _first_diff(out, plain))
            assert used in (None, len(src))
            assert pieces > 0, "%s %s: the serial path took the stream" % (name, fmt)


def test_long_stream_bad_trailers(eng):
    plain = cc.small_sum_long(200000)
    raw = _stored_raw(plain)
    for fmt, src in cc.good_frames(plain, raw):
        with gl._path(eng):
            st, used, out = gl._higher(eng, fmt, src, len(plain))
            pieces, _ = gl._par_last(eng)
        assert (st, out) == (OK, plain) and pieces > 0, (fmt, st, pieces)
    for name, fmt, src, what in cc.bad_trailers(plain, raw):
        with gl._path(eng):
            st, used, out = gl._higher(eng, fmt, src, len(plain))
            pieces, _ = gl._par_last(eng)
        assert st == BAD[what] and pieces == 0, (name, st, pieces)


# ---- 5. batch deflate -------------------------------------------------------------------------------------------------------
def _deflate_texts():
    return cc.top_texts() + [("slice-top", cc.slice_top())] + cc.one_hot() + [(nm, t) for nm, t in cc.unit_texts() if nm.startswith("zero-a")]


def _check_frames(fmt, names, plains, res):
    for name, plain, (st, z, ck) in zip(names, plains, res):
        assert st == OK, (name, st)
        want = _sum(fmt, plain)
        assert ck == want, (name, hex(ck))
        if fmt == "zl":
            assert struct.unpack(">I", z[-4:])[0] == want, name
        else:
            assert struct.unpack("<II", z[-8:]) == (want, len(plain)), name
        assert zlib.decompress(z, WBITS[fmt]) == plain, name


@pytest.mark.parametrize("level", [0, 1, 6])
def test_batch_deflate_texts(eng, level):
    """adler_of (csrc/deflate_kernel.hip): 4096 bytes a step from the text's start"""
    texts = _deflate_texts()
    res = eng.deflate_many([t for _, t in texts], ZLIB, level=level)
    _check_frames("zl", [n for n, _ in texts], [t for _, t in texts], res)


@pytest.mark.parametrize("cap_mib", [2, 8])
def test_batch_deflate_in_slices_of_positions(eng, cap_mib):
    """adler_of going on from the running value: with the workspace capped the batch goes through in slices of positions
    (multiples of 32 KiB: P is two), and the kernel brings its own Adler-32 up to the end of every slice"""
    texts = cc.top_texts() + [("slice-top", cc.slice_top())] + [(nm, t) for nm, t in cc.one_hot() if len(t) > 65536]
    assert 13 * sum(len(t) for _, t in texts) > 4 * (cap_mib << 20)  # (13 bytes of workspace a position: several slices)
    eng.set_option("deflate_workspace_cap_mib", cap_mib)
    try:
        res = eng.deflate_many([t for _, t in texts], ZLIB, level=6)
    finally:
        eng.set_option("deflate_workspace_cap_mib", 0)
    _check_frames("zl", [n for n, _ in texts], [t for _, t in texts], res)


def test_batch_deflate_texts_gzip(eng):
    """the CRC-32 of the input comes from md_launch_crc32 (csrc/gz_kernels.hip)"""
    texts = _deflate_texts() + cc.forged_texts() + cc.forged_embedded_texts()
    res = eng.deflate_many([t for _, t in texts], GZIP, level=6)
    _check_frames("gz", [n for n, _ in texts], [t for _, t in texts], res)


@pytest.mark.parametrize("level", [1, 4])
def test_def_ns_texts(eng, level):
    """csrc/deflate_ns.hip: 1024 bytes a step"""
    texts = _deflate_texts()
    res = eng.def_ns_many([t for _, t in texts], level=level, fmt=ZLIB, caps=[2 * len(t) + 8192 for _, t in texts])
    _check_frames("zl", [n for n, _ in texts], [t for _, t in texts], res)


def _deflate_lengths(eng, fmt, level, ns=False, kind="random"):
    """every prefix of the 8400 bytes at the four base offsets, read where it lies in one blob, as one batch
    -> [(status, frame, checksum)] in the order of cc.lengths_descriptors()"""
    import torch
    blob, _ = cc.lengths_blob(kind)
    desc = cc.lengths_descriptors()
    n = len(desc)
    in_off = np.array([o for o, _ in desc], dtype=np.int64)
    in_len = np.array([k for _, k in desc], dtype=np.int64)
    cap = in_len + in_len // 4 + 1024
    out_off = np.zeros(n, dtype=np.int64)
    np.cumsum(((cap + 63) // 64 * 64)[:-1], out=out_off[1:])
    dev = eng.device
    t = lambda a: torch.from_numpy(a).to(dev)
    d_in = t(np.frombuffer(blob, dtype=np.uint8).copy())
    d_out = torch.zeros(int(out_off[-1] + cap[-1]) + 64, dtype=torch.uint8, device=dev)
    d_ioff, d_ilen, d_ooff, d_cap = t(in_off), t(in_len), t(out_off), t(cap)
    if ns:
        out_len = torch.empty(n, dtype=torch.int64, device=dev)
        status, checksum = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        p = lambda x: ctypes.c_void_p(x.data_ptr())
        eng._check(eng.lib.md_def_ns_batch_device(eng.ctx, FORMAT[fmt], level, int(in_len.sum()), n, p(d_in), p(d_ioff), p(d_ilen), p(d_out),
                                                  p(d_ooff), p(d_cap), p(out_len), p(status), p(checksum)))
    else:
        out_len, status, checksum = eng.deflate_batch(FORMAT[fmt], d_in, d_ioff, d_ilen, d_out, d_ooff, d_cap, level=level, total_in=int(in_len.sum()))
    torch.cuda.synchronize(dev)
    out = d_out.cpu().numpy()
    out_len, status = out_len.cpu().numpy(), status.cpu().numpy()
    checksum = checksum.cpu().numpy().view(np.uint32)
    return [(int(status[i]), out[out_off[i]:out_off[i] + out_len[i]].tobytes(), int(checksum[i])) for i in range(n)]


def _check_lengths(fmt, res, kind="random", refused=None):
    """refused: the status with which the encoder may refuse a text (the checksum it reports is still the text's)"""
    text = cc.lengths_text(kind)
    adl, crc = cc.prefix_sums(kind)
    desc = cc.lengths_descriptors()
    assert len(res) == len(desc) == 4 * 8401
    for (off, k), (st, z, ck) in zip(desc, res):
        want = adl[k] if fmt == "zl" else crc[k]
        assert st in (OK, refused) and ck == want, (off % 64, k, st, hex(ck))
        if st != OK:
            continue
        assert (struct.unpack(">I", z[-4:])[0] if fmt == "zl" else struct.unpack("<II", z[-8:])) == (want if fmt == "zl" else (want, k)), (off % 64, k)
        assert zlib.decompress(z, WBITS[fmt]) == text[:k], (off % 64, k)


@pytest.mark.parametrize("level", [0, 1, 6])
def test_batch_deflate_every_length(eng, level):
    _check_lengths("zl", _deflate_lengths(eng, "zl", level))


def test_batch_deflate_every_length_gzip(eng):
    _check_lengths("gz", _deflate_lengths(eng, "gz", 6))


def test_def_ns_every_length(eng):
    """De.Def.Ns refuses a text that stored blocks hold in the fewest bytes (MD_UNEXPECTED_END_OF_OUTPUT whatever the room: the
    reference's behaviour, tests/test_gpu_def_ns.py), which random bytes are from 40 on - its Adler-32 is reported all the
    same; the text of four byte values is refused at no length"""
    res = _deflate_lengths(eng, "zl", 4, ns=True)
    _check_lengths("zl", res, refused=END_OF_OUTPUT)
    assert [st for st, _, _ in res[:40]] == [OK] * 40
    res = _deflate_lengths(eng, "zl", 4, ns=True, kind="four")
    print("def_ns: refused lengths of the four-value text:", sorted({k for (_, k), (st, _, _) in zip(cc.lengths_descriptors(), res) if st != OK})[:20])
    _check_lengths("zl", res, kind="four")


# ---- 6. streaming encoders --------------------------------------------------------------------------------------------------
PIECES = (1, 4095, 4096, 4097, 65537)


@pytest.mark.parametrize("fmt", ["zl", "gz"])
def test_streaming_encoders_at_once(eng, fmt):
    """md_def_batch_*: five encoders, one per piece size, on top(70000).  The running checksum advances per md_def_batch_src
    call (md::adler32_update / md::crc32_update over that piece), and the trailer is the value it has at the end.  The driving
    loop is test_many_encoders_at_once's; the encoder fed a byte a call gets 4096 calls per round, so that it needs 34 rounds
    and not 135 536."""
    data = cc.top(70000)
    lib = eng.lib
    params = eng._params(6, 4096, 0, True)
    n = len(PIECES)
    b = lib.md_def_batch_open(eng.ctx, FORMAT[fmt], ctypes.byref(params), n)
    assert b
    try:
        outs, pos, sent_end = [bytearray() for _ in range(n)], [0] * n, [False] * n
        buf = ctypes.create_string_buffer(1 << 20)
        rounds = 0
        while not all(lib.md_def_batch_status(b, i) == 2 for i in range(n)):  # MD_END
            rounds += 1
            assert rounds < 100
            for i, piece in enumerate(PIECES):
                for _ in range(4096 if piece == 1 else 1):
                    if sent_end[i]:
                        break
                    chunk = data[pos[i]:pos[i] + piece]
                    pos[i] += len(chunk)
                    assert lib.md_def_batch_src(b, i, chunk, len(chunk)) == 0
                    sent_end[i] = len(chunk) == 0
            assert lib.md_def_batch_encode(b) == 0
            for i in range(n):
                assert lib.md_def_batch_status(b, i) in (0, 2), (i, lib.md_def_batch_error(b, i))
                while lib.md_def_batch_pending(b, i):
                    k = lib.md_def_batch_out(b, i, buf, len(buf))
                    assert k > 0
                    outs[i] += buf.raw[:k]
        res = [(OK, bytes(outs[i]), lib.md_def_batch_checksum(b, i)) for i in range(n)]
    finally:
        lib.md_def_batch_close(b)
    _check_frames(fmt, ["top-70000 in pieces of %d" % p for p in PIECES], [data] * n, res)


@pytest.mark.parametrize("fmt", ["zl", "gz"])
def test_single_encoder_in_pieces(eng, fmt):
    """md_def_*: the same pieces; from 4095 bytes on every piece is a launch ("encoder_piece_bytes")"""
    data = cc.top(70000)
    lib = eng.lib
    res = []
    try:
        for piece in PIECES:
            eng.set_option("encoder_piece_bytes", max(piece, 4095))
            params = eng._params(6, 4096, 0, True)
            o = ctypes.create_string_buffer(1 << 16)
            s = lib.md_def_encoder(eng.ctx, FORMAT[fmt], ctypes.byref(params), o, len(o))
            assert s
            try:
                out, pos = bytearray(), 0
                while True:
                    sig = lib.md_def_encode(s)
                    if sig == 0:
                        chunk = data[pos:pos + piece]
                        pos += len(chunk)
                        assert lib.md_def_src(s, chunk, 0, len(chunk)) == 0
                        continue
                    assert sig in (1, 2), lib.md_def_status(s)
                    out += o.raw[:len(o) - lib.md_def_dst_rem(s)]
                    if sig == 2:
                        break
                    lib.md_def_dst(s, o, len(o))
                res.append((lib.md_def_status(s), bytes(out), lib.md_def_checksum(s)))
            finally:
                lib.md_def_free(s)
    finally:
        eng.set_option("encoder_piece_bytes", 1 << 20)
    _check_frames(fmt, ["top-70000 in pieces of %d" % p for p in PIECES], [data] * len(PIECES), res)


# ---- 7. spans ---------------------------------------------------------------------------------------------------------------
def _span_cases():
    """(name, text, span, whether some but not all spans must go out stored)"""
    out = []
    for n in cc.UNIT_LENGTHS:
        for kind in cc.KINDS:  # every span with a == 0 (mod 65521), a == 1, b == 0; a length of 0 (mod 65521)
            out.append(("%s-%d x 5" % (kind, n), cc.units(kind, n, 5), n, False))
    out.append(("zeros, span 65521", bytes(3 * 65521 + 1), 65521, False))
    out.append(("0xFF, span 65521", b"\xff" * (3 * 65521 + 1), 65521, False))
    out.append(("random, span 65521", cc.long_random(3 * 65521 + 1), 65521, False))
    out.append(("top-200000, span 4096", cc.top(200000), 4096, False))
    out.append(("top-4097, span 4096", cc.top(4097), 4096, False))
    for span in (64, 4096):  # random spans do not fit their slots and go out stored (adler_kernel sums them), runs of 0xFF fit
        mixed = b"".join(cc.rand(3 * span + 17 * i, 20 + i) + b"\xff" * (5 * span + i) for i in range(4)) + cc.rand(span + 1, 30)
        out.append(("random and 0xFF, span %d" % span, mixed, span, True))
    return out


@pytest.mark.parametrize("fmt", ["zl", "gz"])
def test_spans(eng, fmt):
    """adler_kernel, adler_fold and crc_fold of csrc/deflate_spans.hip"""
    for name, text, span, mixed in _span_cases():
        st, z, ck = eng.deflate_spans(text, FORMAT[fmt], span=span)
        info = eng.deflate_spans_last()
        _check_frames(fmt, [name], [text], [(st, z, ck)])
        assert info["spans"] == (len(text) + span - 1) // span, (name, info)
        print("spans: %-28s %s %d spans, %d stored" % (name, fmt, info["spans"], info["stored_spans"]))
        if mixed:
            assert 0 < info["stored_spans"] < info["spans"], (name, info)


# ---- 8. crc32_batch ---------------------------------------------------------------------------------------------------------
def test_crc32_every_length(eng):
    """crc32_wave (csrc/gz_crc.hpp): every length 0 .. 8400 from bases 0, 1, 15 and 63 mod 64 - every lane segment size up to
    192, every head length up to the next 64-byte line, lanes with nothing - the long texts, whose zero runs pin every
    gf_xpow8, and a lane CRC of 0 / ~0 next to the "CRC of nothing" """
    import torch
    blob, _ = cc.lengths_blob()
    desc = cc.lengths_descriptors()
    _, crc = cc.prefix_sums()
    want = [crc[k] for _, k in desc]
    data = bytearray(blob)
    for name, t in cc.long_texts() + cc.forged_texts() + cc.forged_embedded_texts():
        for shift in (0, 1):  # on a 64-byte line, and one byte behind it
            data += bytes((shift - len(data)) % 64)
            desc.append((len(data), len(t)))
            want.append(zlib.crc32(t))
            data += t
    dev = eng.device
    d = torch.from_numpy(np.frombuffer(bytes(data) + bytes(64), dtype=np.uint8).copy()).to(dev)
    got = eng.crc32_batch(d, torch.tensor([o for o, _ in desc], dtype=torch.int64, device=dev), torch.tensor([k for _, k in desc], dtype=torch.int64, device=dev))
    eng.synchronize()
    got = [int(x) & 0xffffffff for x in got.cpu().tolist()]
    assert len(got) == len(want) == 4 * 8401 + 2 * (18 + 4)
    bad = [(o % 64, k, hex(g), hex(w)) for (o, k), g, w in zip(desc, got, want) if g != w]
    assert not bad, (len(bad), bad[:8])


# ---- 9. ZIP reading ---------------------------------------------------------------------------------------------------------
def test_zip_entries_at_the_segment_joins(eng):
    """zip_kernels.hip's join_crc: an entry's CRC-32 from segments of 4 KiB (the smallest "zip_crc_segment"), 64 segments a
    wavefront's worth"""
    seg = 4096
    lens = (seg - 1, seg, seg + 1, 64 * seg, 64 * seg + 1, 65 * seg - 1)
    files = [("zero-%d" % n, bytes(n)) for n in lens] + [("random-%d" % n, cc.long_random(n)) for n in lens]
    files += cc.forged_texts() + cc.forged_embedded_texts()
    victim = [n for n, _ in files].index("random-%d" % (64 * seg + 1))
    gz_._segment(eng, 4)
    try:
        for method in (zipfile.ZIP_STORED, zipfile.ZIP_DEFLATED):
            blob = zu.zipfile_bytes(files, method, 6 if method == zipfile.ZIP_DEFLATED else None)
            with zipfile.ZipFile(io.BytesIO(blob)) as z:
                infos = z.infolist()
                assert [(i.filename, i.file_size, i.CRC, i.compress_type) for i in infos] == [(n, len(d), zlib.crc32(d), method) for n, d in files]
                at = z.start_dir
            gz_._check_all(eng, blob, [d for _, d in files], method)
            # one flipped bit of one entry's CRC-32 in the directory
            for _ in range(victim):
                assert blob[at:at + 4] == b"PK\x01\x02"
                at += 46 + sum(struct.unpack_from("<HHH", blob, at + 28))
            assert struct.unpack_from("<I", blob, at + 16)[0] == zlib.crc32(files[victim][1])
            bad = bytearray(blob)
            bad[at + 18] ^= 0x04
            rc, st, off, res, out = gz_._run(eng, bytes(bad))
            assert rc == 0 and res[:2] == (len(files), 1), (method, rc, res)
            assert st == [BAD["checksum"] if k == victim else OK for k in range(len(files))], (method, st)
            for k, (_, d) in enumerate(files):
                if k != victim:
                    assert out[off[k]:off[k + 1]] == d, (method, k)
    finally:
        gz_._segment(eng, 0)
