"""Many streaming decoders at once (md_inf_batch_*): every decoder's bytes, status, message, checksum and
src_rem equal md_inf_*'s (md_inf_chunk_bytes(1), the same pieces) and the whole-buffer answer, whatever the pieces; one
launch per round; output room and long blocks handled as md_inf_* handles them.  Needs an MI355X: `pytest -m gpu`."""
import ctypes
import gzip
import math
import random
import zlib

import pytest

pytestmark = pytest.mark.gpu

DEFLATE, ZLIB, GZIP = 0, 1, 2
AWAIT, FLUSH, END, MALFORMED = 0, 1, 2, 3


@pytest.fixture(scope="module")
def eng():
    import decompress_amd
    return decompress_amd.Engine(0)


def _compress(fmt, data, level):
    if fmt == ZLIB:
        return zlib.compress(data, level)
    c = zlib.compressobj(level, zlib.DEFLATED, -15 if fmt == DEFLATE else 31)
    return c.compress(data) + c.flush()


def _cut(src, spec, rng):
    """pieces of `src`: a fixed size, or random sizes (log-uniform, 1 B .. 300 KB) when spec is None"""
    out, p = [], 0
    while p < len(src):
        k = spec if spec else max(1, int(math.exp(rng.uniform(0, math.log(300000)))))
        out.append(src[p:p + k])
        p += k
    return out


def run_batch(eng, fmt, plans, fetch_every=1, on_round=None):
    """decode_many by hand: every unfinished decoder gets its next piece (or its end) per round -> per decoder
    (status, error, message, bytes, checksum, src_rem), and the number of rounds"""
    lib = eng.lib
    n = len(plans)
    b = lib.md_inf_batch_open(eng.ctx, fmt, n)
    assert b
    outs = [bytearray() for _ in range(n)]
    pos, ended = [0] * n, [False] * n
    buf = ctypes.create_string_buffer(1 << 20)

    def drain(i):
        while lib.md_inf_batch_pending(b, i):
            k = lib.md_inf_batch_out(b, i, buf, len(buf))
            assert k > 0
            outs[i] += buf.raw[:k]
    rounds = 0
    try:
        while True:
            live = [i for i in range(n) if lib.md_inf_batch_status(b, i) == AWAIT]
            if not live:
                break
            for i in live:
                if pos[i] < len(plans[i]):
                    c = plans[i][pos[i]]
                    pos[i] += 1
                    assert lib.md_inf_batch_src(b, i, c, len(c)) == 0
                elif not ended[i]:
                    ended[i] = True
                    assert lib.md_inf_batch_src(b, i, None, 0) == 0
            assert lib.md_inf_batch_decode(b) == 0
            rounds += 1
            if on_round:
                on_round(b, rounds, pos, ended)
            if rounds % fetch_every == 0:
                for i in range(n):
                    drain(i)
        for i in range(n):
            drain(i)
        res = [(lib.md_inf_batch_status(b, i), lib.md_inf_batch_error(b, i), lib.md_inf_batch_message(b, i).decode(),
                bytes(outs[i]), lib.md_inf_batch_checksum(b, i), lib.md_inf_batch_src_rem(b, i)) for i in range(n)]
        return res, rounds, lib.md_i_inf_batch_launches(b), [lib.md_i_inf_batch_attempts(b, i) for i in range(n)]
    finally:
        lib.md_inf_batch_close(b)


def run_single(eng, fmt, pieces):
    """md_inf_* with md_inf_chunk_bytes(1) on the same pieces -> (signal, status, message, bytes, checksum, src_rem)"""
    lib = eng.lib
    o = ctypes.create_string_buffer(65536)
    d = lib.md_inf_decoder(eng.ctx, fmt, o, 65536)
    lib.md_inf_chunk_bytes(d, 1)
    it, out = iter(pieces), bytearray()
    try:
        while True:
            sig = lib.md_inf_decode(d)
            if sig == AWAIT:
                c = next(it, b"")
                lib.md_inf_src(d, bytes(c), 0, len(c))
                continue
            out += o.raw[:65536 - lib.md_inf_dst_rem(d)]
            lib.md_inf_flush(d)
            if sig in (END, MALFORMED):
                return (sig, lib.md_inf_status(d), lib.md_inf_message(d).decode(), bytes(out), lib.md_inf_checksum(d),
                        lib.md_inf_src_rem(d))
    finally:
        lib.md_inf_free(d)


def _plains():
    from decompress_amd import workloads
    rng = random.Random(7)
    return {
        "empty": b"",
        "one": b"q",
        "text": workloads.text(3, 50_000),
        "random": rng.randbytes(150_000),  # incompressible: stored blocks
        "runs": b"".join(bytes([rng.randrange(4)]) * rng.randrange(1, 600) for _ in range(800)),
        "markov": workloads.markov_text(4, 400_000),
        "long": workloads.text(5, 3_000_000),
    }


@pytest.mark.parametrize("fmt", [DEFLATE, ZLIB, GZIP])
def test_parity_matrix(eng, fmt):
    """~14 streams per format: zlib levels 0/1/6/9 and this project's deflate, pieces of 1, 7, 4 096, 65 536, 300 000
    bytes or random sizes, garbage behind some; output left unfetched for three rounds at a time"""
    rng = random.Random(100 + fmt)
    plains = _plains()
    own = {k: v for k, v in zip(plains, eng.deflate_many(list(plains.values()), fmt, level=6))}
    specs = [1, 7, 4096, 65536, 300000, None]
    streams = []
    for j, (name, plain) in enumerate(plains.items()):
        for level in ((0, 9) if name in ("long", "markov") else (1, 6)):
            streams.append((name, level, plain, _compress(fmt, plain, level)))
        st, z, _ = own[name]
        assert st == 0
        streams.append((name, "own", plain, z))
    plans, meta = [], []
    for k, (name, level, plain, z) in enumerate(streams):
        garbage = b"garbage!"[:k % 5]
        src = z + garbage
        spec = specs[k % len(specs)]
        if spec in (1, 7) and len(src) > 4000:
            spec = 4096
        plans.append(_cut(src, spec, rng))
        meta.append((name, level, plain, garbage, src))
    res, rounds, launches, _ = run_batch(eng, fmt, plans, fetch_every=3)
    assert 0 < launches
    for (name, level, plain, garbage, src), r, pl in zip(meta, res, plans):
        sig, st, msg, out, ck, rem = r
        assert (sig, st) == (END, 0), (name, level, r[:3])
        assert out == plain, (name, level, len(out), len(plain))
        assert ck == (zlib.crc32(plain) if fmt == GZIP else zlib.adler32(plain)), (name, level)
        assert rem == len(garbage), (name, level, rem)
    # and md_inf_* on the same pieces, for a sample (every field)
    for k in range(0, len(plans), 3):
        assert run_single(eng, fmt, plans[k]) == res[k], (meta[k][0], meta[k][1])


def _gz_member(body, data, crc_xor=0, size_add=0, hcrc_xor=0):
    fixed = bytes([0x1f, 0x8b, 8, 2 | 4 | 8 | 16]) + b"\0\0\0\0" + bytes([0, 3])
    extra, name, comment = b"\x00\x05hello", b"a name\0", b"a comment\0"
    hcrc = ((zlib.crc32(fixed + name + comment) >> 16) & 0xffff) ^ hcrc_xor
    head = fixed + extra + name + comment + bytes([hcrc >> 8, hcrc & 0xff])
    tail = ((zlib.crc32(data) ^ crc_xor) & 0xffffffff).to_bytes(4, "little") + ((len(data) + size_add) & 0xffffffff).to_bytes(4, "little")
    return head + body + tail


def test_malformed_same_as_single_decoder(eng, oracle):
    """the malformed cases of test_streaming_decoder_hands_out_before_the_end, in one batch per format next to valid
    streams: every field equals md_inf_*'s, and the whole-buffer oracle agrees on status and bytes"""
    from decompress_amd import workloads
    rng = random.Random(0x57e)
    plain = workloads.text(11, 900_000) + rng.randbytes(100_000) + workloads.markov_text(12, 300_000)
    z = zlib.compress(plain, 6)
    raw = z[2:-4]
    cases = {
        DEFLATE: [("raw", raw + b"xyz", 0), ("raw-flipped", raw[:len(raw) // 2] + bytes([raw[len(raw) // 2] ^ 0x10]) + raw[len(raw) // 2 + 1:], None),
                  ("raw-cut", raw[:len(raw) // 3], 1)],
        ZLIB: [("zlib", z, 0), ("zlib-checksum", z[:-1] + bytes([z[-1] ^ 1]), 9), ("zlib-cut", z[:len(z) // 2], 1),
               ("zlib-header", bytes([0x78, 0x9d]) + z[2:], None)],
        GZIP: [("gzip", _gz_member(raw, plain) + b"rest", 0), ("gzip-crc", _gz_member(raw, plain, crc_xor=1), 9),
               ("gzip-size", _gz_member(raw, plain, size_add=1), 12), ("gzip-hcrc", _gz_member(raw, plain, hcrc_xor=1), 11),
               ("gzip-cut", _gz_member(raw, plain)[:len(raw) // 2], 1), ("gzip-magic", b"\x1f\x8c" + _gz_member(raw, plain)[2:], None)],
    }
    valid = workloads.text(13, 200_000)
    for fmt, cs in cases.items():
        srcs = [src for _, src, _ in cs] + [_compress(fmt, valid, 6)] * 2
        plans = [[s[i:i + 50000] for i in range(0, len(s), 50000)] for s in srcs]
        plans[-1] = _cut(srcs[-1], 7000, rng)
        res, _, _, _ = run_batch(eng, fmt, plans)
        for (name, src, want), r, pl in zip(cs, res, plans):
            assert run_single(eng, fmt, pl) == r, name
            sig, st, msg, out, ck, rem = r
            if want is not None:
                assert st == want, (name, st, msg)
            if name == "zlib-cut":
                ost, _, oout = oracle.de_inflate(src[2:], len(plain) + 16)
            elif name == "gzip-cut":
                ost, _, oout = oracle.de_inflate(src[len(_gz_member(b"", b"")) - 8:], len(plain) + 16)
            elif fmt == GZIP:
                ost, _, oout, _ = oracle.gz_inflate(src, len(plain) + 16)
                if ost in (9, 12):
                    oout = plain
            elif fmt == ZLIB:
                ost, _, oout = oracle.zl_inflate(src, len(plain) + 16)
            else:
                ost, _, oout = oracle.de_inflate(src, len(plain) + 16)
            assert st == ost, (name, st, ost)
            if ost in (0, 9, 12) or name in ("zlib-cut", "gzip-cut"):
                assert out == oout, (name, len(out), len(oout))
        for r in res[-2:]:
            assert r[:2] == (END, 0) and r[3] == valid


def test_split_frames_every_offset(eng):
    """GZip headers with FEXTRA / FNAME / FCOMMENT / FHCRC, ZLIB headers and both trailers split at every byte offset
    (one decoder per offset, two rounds), and fed a byte a round"""
    from decompress_amd import workloads
    data = workloads.text(21, 3000)
    raw = _compress(DEFLATE, data, 6)
    for fmt, src in ((GZIP, _gz_member(raw, data) + b"zz"), (ZLIB, zlib.compress(data, 9) + b"zz")):
        plans = [[src[:s], src[s:]] if 0 < s < len(src) else [src] for s in range(len(src) + 1)]
        plans.append([src[i:i + 1] for i in range(len(src))])
        plans.append([src[i:i + 3] for i in range(0, len(src), 3)])
        res, _, _, _ = run_batch(eng, fmt, plans)
        want_ck = zlib.crc32(data) if fmt == GZIP else zlib.adler32(data)
        for s, (r, pl) in enumerate(zip(res, plans)):
            assert r[:2] == (END, 0) and r[3:5] == (data, want_ck), (fmt, s, r[:3])
            if len(pl) <= 2:  # src_rem: the garbage that came with the piece that ended the stream (later pieces are not fed)
                end, got = len(src) - 2, 0
                for c in pl:
                    got += len(c)
                    if got >= end:
                        break
                assert r[5] == got - end, (fmt, s, r[5])
        # (a byte a round: the need rule looks again only once the input has doubled, garbage that came meanwhile counts)
        for k in (0, 40, len(src) - 3, len(plans) - 2, len(plans) - 1):
            assert run_single(eng, fmt, plans[k]) == res[k], (fmt, k)


def test_output_before_the_end(eng):
    """with 64 KiB pieces, output is pending before a decoder's end of input is sent"""
    from decompress_amd import workloads
    datas = [workloads.text(30 + i, 1_500_000) for i in range(4)]
    seen = [False] * 4

    def on_round(b, r, pos, ended):
        for i in range(4):
            if not ended[i] and eng.lib.md_inf_batch_pending(b, i):
                seen[i] = True
    for fmt in (ZLIB, GZIP):
        srcs = [_compress(fmt, d, 6) for d in datas]
        res, _, _, _ = run_batch(eng, fmt, [_cut(s, 65536, None) for s in srcs], on_round=on_round)
        assert all(r[:2] == (END, 0) and r[3] == d for r, d in zip(res, datas))
    assert all(seen)


def test_output_room_runs_out(eng):
    """64 MiB of zeros at level 9 in 4 KiB pieces: the room grows in the same call, in a few rounds only"""
    plain = bytes(64 << 20)
    z = zlib.compress(plain, 9)
    lib = eng.lib
    per_round = []

    def on_round(b, r, pos, ended):
        per_round.append(lib.md_i_inf_batch_launches(b) - sum(per_round))
    res, rounds, launches, _ = run_batch(eng, ZLIB, [_cut(z, 4096, None), _cut(zlib.compress(b"abc" * 999, 6), 4096, None)],
                                         on_round=on_round)
    assert res[0][:2] == (END, 0) and res[0][3] == plain and res[0][4] == zlib.adler32(plain)
    assert res[1][3] == b"abc" * 999
    assert sum(per_round) == launches and len(per_round) == rounds
    grew = [d for d in per_round if d > 1]  # (a round is one launch, more only where a room grew)
    assert 0 < len(grew) <= 3, per_round  # (the room a decoder needed stays: later rounds start there)


def test_one_block_over_many_rounds(eng):
    """one dynamic block of ~1 MiB of compressed tokens in 1 KiB pieces: decoded right, and the decoder tries again only
    when its buffered input has doubled - a logarithmic number of attempts, not one per piece"""
    from tests import deflate_writer as dw
    rng = random.Random(5)
    toks = []
    for _ in range(700_000):
        if toks and rng.random() < 0.3:
            toks.append(dw.match(rng.randrange(3, 12), rng.randrange(1, min(len(toks), 30000) + 1)))
        else:
            toks.append(rng.randrange(256))
    blocks = [dw.Block("dynamic", toks)]
    raw = dw.write(blocks)
    st, want = dw.expand(blocks)
    assert st == 0 and len(raw) > 700_000
    plans = [_cut(raw, 1024, None)]
    res, rounds, launches, attempts = run_batch(eng, DEFLATE, plans)
    assert res[0][:2] == (END, 0) and res[0][3] == want
    assert rounds >= len(plans[0])
    assert attempts[0] <= 2 * math.log2(len(plans[0])) + 4, (attempts[0], len(plans[0]))
    assert launches == attempts[0]


def test_launch_count(eng):
    """64 decoders over R rounds: R launches; a decode with nothing new launches nothing"""
    from decompress_amd import workloads
    lib = eng.lib
    datas = [workloads.text(200 + i, 400_000) for i in range(64)]
    srcs = [zlib.compress(d, 1) for d in datas]
    res, rounds, launches, attempts = run_batch(eng, ZLIB, [_cut(s, 65536, None) for s in srcs])
    assert all(r[:2] == (END, 0) and r[3] == d for r, d in zip(res, datas))
    assert launches == rounds
    b = lib.md_inf_batch_open(eng.ctx, ZLIB, 64)
    try:
        assert lib.md_inf_batch_decode(b) == 0
        assert lib.md_i_inf_batch_launches(b) == 0
        assert lib.md_inf_batch_src(b, 3, srcs[3][:1000], 1000) == 0
        assert lib.md_inf_batch_decode(b) == 0 and lib.md_i_inf_batch_launches(b) == 1
        assert lib.md_inf_batch_decode(b) == 0 and lib.md_i_inf_batch_launches(b) == 1
        assert lib.md_i_inf_batch_attempts(b, 3) == 1 and lib.md_i_inf_batch_attempts(b, 4) == 0
    finally:
        lib.md_inf_batch_close(b)


def test_slots_reset_and_misuse(eng):
    lib = eng.lib
    assert not lib.md_inf_batch_open(eng.ctx, 7, 4)
    assert not lib.md_inf_batch_open(eng.ctx, ZLIB, 0)
    b = lib.md_inf_batch_open(eng.ctx, GZIP, 2)
    try:
        a, c = gzip.compress(b"first stream " * 500, mtime=0), gzip.compress(b"second one " * 700, mtime=0)
        assert lib.md_inf_batch_src(b, 2, a, len(a)) < 0  # (no such slot)
        assert lib.md_inf_batch_src(b, 0, None, 5) < 0
        assert lib.md_inf_batch_src(b, 0, a, (1 << 30) + 1) < 0  # (more than a round takes: refused before it is read)
        assert lib.md_inf_batch_src(b, 0, a, len(a)) == 0
        assert lib.md_inf_batch_src(b, 1, a[:10], 10) == 0
        assert lib.md_inf_batch_src(b, 1, None, 0) == 0
        assert lib.md_inf_batch_src(b, 1, a, 1) < 0  # (after the end of input)
        assert lib.md_inf_batch_src(b, 1, None, 0) < 0
        assert lib.md_inf_batch_decode(b) == 0
        assert lib.md_inf_batch_status(b, 0) == END and lib.md_inf_batch_status(b, 1) == MALFORMED
        assert lib.md_inf_batch_error(b, 1) == 1 and lib.md_inf_batch_message(b, 1) == b"Unexpected end of input"
        assert lib.md_inf_batch_src(b, 0, a, 1) < 0  # (a finished slot)
        buf = ctypes.create_string_buffer(1 << 16)
        k = lib.md_inf_batch_out(b, 0, buf, len(buf))
        assert buf.raw[:k] == b"first stream " * 500 and lib.md_inf_batch_checksum(b, 0) == zlib.crc32(b"first stream " * 500)
        for i in (0, 1):
            lib.md_inf_batch_reset(b, i)
            assert lib.md_inf_batch_status(b, i) == AWAIT and lib.md_inf_batch_pending(b, i) == 0
        assert lib.md_inf_batch_src(b, 1, c, len(c)) == 0
        assert lib.md_inf_batch_decode(b) == 0
        assert lib.md_inf_batch_status(b, 1) == END and lib.md_inf_batch_status(b, 0) == AWAIT
        k = lib.md_inf_batch_out(b, 1, buf, len(buf))
        assert buf.raw[:k] == b"second one " * 700 and lib.md_inf_batch_src_rem(b, 1) == 0
    finally:
        lib.md_inf_batch_close(b)


def test_decode_many(eng):
    from decompress_amd import de
    datas = [b"", b"x" * 100_000, bytes(range(256)) * 300]
    streams = [[zlib.compress(d)[i:i + 999] for i in range(0, len(zlib.compress(d)), 999)] for d in datas]
    streams.append([b"\x78\x9c\x01"])
    res = de.Inf.decode_many(streams, fmt=ZLIB)
    assert [r[:2] for r in res[:3]] == [("Ok", d) for d in datas]
    assert res[3][0] == "Unexpected_end_of_input" and res[3][2] == "Unexpected end of input"


def test_many_decoders_one_round(eng):
    """66 000 tiny ZLIB streams - more than gridDim.y - in one round"""
    n = 66_000
    datas = [(b"%d," % i) * (1 + i % 7) for i in range(n)]
    srcs = [zlib.compress(d, 6) for d in datas]
    res, rounds, launches, _ = run_batch(eng, ZLIB, [[s] for s in srcs])
    assert rounds == 1 and launches == 1
    bad = [i for i, (r, d) in enumerate(zip(res, datas)) if r[:2] != (END, 0) or r[3] != d or r[4] != zlib.adler32(d)]
    assert not bad, bad[:5]
