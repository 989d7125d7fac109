"""ONE long stream's hash chains built in segments by many workgroups instead of by one (capi_deflate.cpp link_segments,
csrc/deflate_chunked.hip).  The bytes must be the oracle's and the one-workgroup path's in every case, and the
segments must have run (Engine.link_segments).  Small "deflate_link_segment_min" and segment sizes make moderate inputs
take it, with many segment boundaries.  Needs an MI355X: `pytest -m gpu`."""
import os
import random
import zlib

import pytest

pytestmark = pytest.mark.gpu

SEG_KIB = 16
SEG = SEG_KIB << 10


@pytest.fixture(scope="module")
def eng():
    import decompress_amd
    e = decompress_amd.Engine(0)
    e.set_option("deflate_link_segment_min", 64)
    e.set_option("deflate_link_segment", SEG_KIB)
    return e


def _rand(seed, n):
    return random.Random(seed).randbytes(n)


def _inputs():
    from decompress_amd import workloads
    text = workloads.text(41, 200_000)
    ascii_only = bytes(b & 0x7f for b in workloads.text(42, 120_000))
    return {
        "corpus": workloads.corpus_slice(3, 300_000),
        "markov": workloads.markov_text(5, 250_000),
        "random": _rand(6, 200_000),
        # 258-byte matches straddle every segment boundary
        "zeros": bytes(200_000),
        "period7": (b"abcdefg" * 40_000)[:250_000],
        "period3x": (b"xy\x00" * 70_000)[:200_001],
        # binary first: the first fill uses few codes (the pkzip mutation of the first tree build)
        "bin_then_text": bytes(70_000) + text,
        # symbols that appear only late (the Zl driver's Leave splits)
        "late_symbols": ascii_only + bytes(range(128, 256)) * 40 + ascii_only,
    }


def _boundary_lengths():
    from decompress_amd import workloads
    base = workloads.text(43, 5 * SEG + 64)
    return {"len%+d" % d: base[:5 * SEG + d] for d in (-3, -1, 1, 3)}


def _stats(e):
    return e.link_segments()


def _one(e, data, fmt, **kw):
    st, out, ck = e.deflate_one(data, fmt, **kw)
    return st, out, ck, _stats(e)


def test_zlib_levels_match_oracle(eng, oracle):
    import decompress_amd
    data = dict(_inputs(), **_boundary_lengths())
    for name, d in data.items():
        for level in (1, 4, 6, 9):
            st, out, adler, segs = _one(eng, d, decompress_amd.FORMAT_ZLIB, level=level)
            assert st == 0, (name, level)
            # segments of the positions inserted ahead, [0, len - 3)
            assert segs == (len(d) - 3 + SEG - 1) // SEG and segs >= 2, (name, level, segs)
            assert out == oracle.zl_deflate(d, level, 4096, True), (name, level)
            assert zlib.decompress(out) == d and adler == zlib.adler32(d)


@pytest.mark.parametrize("driver", [0, 1, 2], ids=["Zl.Def", "De.Higher", "CLI"])
def test_raw_drivers_queues_dynamic(eng, oracle, driver):
    import decompress_amd
    data = _inputs()
    data.update(_boundary_lengths())
    for name in ("corpus", "markov", "zeros", "bin_then_text", "late_symbols", "len-3", "len+1"):
        d = data[name]
        for q in (4096, 256, 64):
            for dyn in (True, False):
                for level in ((4,) if driver == 1 else (1, 6, 9)):
                    want, wadler = oracle.deflate_raw(d, level, q, driver, dyn)
                    st, out, adler, segs = _one(eng, d, decompress_amd.FORMAT_DEFLATE, level=level, queue=q,
                                                        driver=driver, dynamic=dyn)
                    assert segs >= 2, (name, q, dyn, level)
                    if want is None:  # De.Queue.Full in the reference (the CLI driver's end-of-block push)
                        assert (st, out) == (13, b""), (name, q, dyn, level)
                        continue
                    assert st == 0, (name, q, dyn, level)
                    assert out == want, (name, q, dyn, level, len(out), len(want))
                    assert zlib.decompress(out, -15) == d and adler == wadler == zlib.adler32(d)


def test_gzip_matches_oracle(eng, oracle):
    import decompress_amd
    data = _inputs()
    for name in ("corpus", "markov", "random", "period7"):
        d = data[name]
        for level in (1, 6, 9):
            st, out, crc, segs = _one(eng, d, decompress_amd.FORMAT_GZIP, level=level)
            assert st == 0 and segs >= 2, (name, level)
            assert out == oracle.gz_deflate(d, level=level), (name, level)
            assert zlib.decompress(out, 31) == d and crc == zlib.crc32(d)


def test_equal_to_serial_path(eng):
    """the same call with the path switched off: the same status, bytes and checksum"""
    import decompress_amd
    data = _inputs()
    cases = [(decompress_amd.FORMAT_ZLIB, dict(level=6)), (decompress_amd.FORMAT_DEFLATE, dict(level=4, driver=1, queue=256)),
             (decompress_amd.FORMAT_DEFLATE, dict(level=9, driver=2)), (decompress_amd.FORMAT_GZIP, dict(level=4))]
    try:
        for name in ("corpus", "zeros", "late_symbols"):
            for fmt, kw in cases:
                eng.set_option("deflate_link_segment_min", 64)
                par = _one(eng, data[name], fmt, **kw)
                eng.set_option("deflate_link_segment_min", 0)
                ser = _one(eng, data[name], fmt, **kw)
                assert par[3] >= 2 and ser[3] == 0, (name, fmt, kw)
                assert par[:3] == ser[:3], (name, fmt, kw)
    finally:
        eng.set_option("deflate_link_segment_min", 64)


def test_fallbacks_are_exact(eng, oracle):
    """what the path does not take runs as before (segments == 0), and what it takes reports exactly what the serial
    path reports, an output buffer too small included"""
    import decompress_amd
    d = _inputs()["markov"]
    # level 0 (stored blocks: no matcher)
    st, out, _, stats = _one(eng, d, decompress_amd.FORMAT_ZLIB, level=0)
    assert st == 0 and stats == 0 and out == oracle.zl_deflate(d, 0, 4096, True)
    # Lz's matcher
    st, out, _, stats = _one(eng, d, decompress_amd.FORMAT_DEFLATE, level=6, matcher=1)
    assert st == 0 and stats == 0 and out == oracle.deflate_raw(d, 6, matcher=1)[0]
    # below the threshold
    small = d[:60_000]
    st, out, _, stats = _one(eng, small, decompress_amd.FORMAT_ZLIB, level=6)
    assert st == 0 and stats == 0 and out == oracle.zl_deflate(small, 6, 4096, True)
    # one segment: nothing to spread
    eng.set_option("deflate_link_segment", 1024)
    try:
        st, out, _, stats = _one(eng, d, decompress_amd.FORMAT_ZLIB, level=6)
        assert st == 0 and stats == 0 and out == oracle.zl_deflate(d, 6, 4096, True)
    finally:
        eng.set_option("deflate_link_segment", SEG_KIB)
    # switched off
    eng.set_option("deflate_link_segment_min", 0)
    try:
        st, out, _, stats = _one(eng, d, decompress_amd.FORMAT_ZLIB, level=6)
        assert st == 0 and stats == 0 and out == oracle.zl_deflate(d, 6, 4096, True)
        ser_small = [_one(eng, d, decompress_amd.FORMAT_ZLIB, level=6, cap=c)[:3] for c in (100, 5000)]
    finally:
        eng.set_option("deflate_link_segment_min", 64)
    # too little room: the serial path's status and bytes
    for c, ser in zip((100, 5000), ser_small):
        par = _one(eng, d, decompress_amd.FORMAT_ZLIB, level=6, cap=c)
        assert par[0] != 0 and par[:3] == ser, (c, par[0], ser[0])
    # a batch of several streams keeps the one-workgroup path
    import numpy as np
    blob = np.frombuffer(d + d, dtype=np.uint8).copy()
    out = np.zeros(4 * len(d), dtype=np.uint8)
    eng.deflate_batch_host(decompress_amd.FORMAT_ZLIB, blob, [0, len(d)], [len(d), len(d)], out, [0, 2 * len(d)],
                           [2 * len(d), 2 * len(d)], level=6)
    assert _stats(eng) == 0


def test_options_are_checked(eng):
    import decompress_amd
    with pytest.raises(decompress_amd.Error):
        eng.set_option("deflate_link_segment_min", -1)
    with pytest.raises(decompress_amd.Error):
        eng.set_option("deflate_link_segment", -1)


def test_higher_compress_default_settings(oracle):
    """Zl.Higher.compress / De.Higher.compress / Gz.Higher.compress and the CLI on a stream above the default threshold
    (128 KiB) take the segments with the default segment size"""
    from decompress_amd import cli, de, engine, gz, workloads, zl
    d = workloads.markov_text(8, (1 << 20) + 12345)
    e = engine.default_engine(0)
    z = zl.Higher.compress(d, level=6)
    segs = e.link_segments()
    assert segs == (len(d) - 3 + 65535) // 65536, segs
    assert z == oracle.zl_deflate(d, 6, 4096, True) and zlib.decompress(z) == d
    r = de.Higher.compress(d)
    assert e.link_segments() == segs
    assert r == oracle.deflate_raw(d, 4, 4096, 1)[0]
    g = gz.Higher.compress(d, level=4)
    assert e.link_segments() == segs
    assert g == oracle.gz_deflate(d, level=4) and zlib.decompress(g, 31) == d
    for fmt in ("deflate", "zlib", "gzip"):
        rc, out, _ = cli.run(True, fmt, 6, d, now=0)
        assert rc == 0 and e.link_segments() == segs, fmt
        assert zlib.decompress(out, {"deflate": -15, "zlib": 15, "gzip": 31}[fmt]) == d


@pytest.mark.skipif(not os.environ.get("MD_SLOW"), reason="64 MiB through the sequential kernel and the oracle (set MD_SLOW=1)")
def test_64mib_text_level6(oracle):
    from decompress_amd import workloads, zl, engine
    d = workloads.text(44, 64 << 20)
    z = zl.Higher.compress(d, level=6)
    assert engine.default_engine(0).link_segments() >= 2
    assert z == oracle.zl_deflate(d, 6, 4096, True)
