"""PRIMED joined spans on the GPU (md_set_option "deflate_span_prime", `prime=` of the Python entry points).  Needs
an MI355X: `pytest -m gpu`.  The yardstick is tests/primed_spans_model.py - the definition over the oracle's own matcher and
encoder - and the bytes must equal it exactly in all three formats; unprimed, the same calls still equal
tests/deflate_spans_model.py; libz and this library's own decoders read the streams back."""
import ctypes
import subprocess
import sys
import zlib

import pytest

from tests import deflate_spans_model as U
from tests import primed_spans_model as P

pytestmark = pytest.mark.gpu
CASES = P.cases()
END_OF_OUTPUT = 2


@pytest.fixture(scope="module")
def eng():
    from decompress_amd import engine
    return engine.default_engine(0)


def _spans(eng, data, span, fmt, header=None, cap=None, prime=True, **params):
    return eng.deflate_spans(data, fmt, span=span, header=header, cap=cap, prime=prime, **params)


@pytest.mark.parametrize("name,data,span,params", CASES, ids=[c[0] for c in CASES])
def test_bytes_equal_the_model(eng, name, data, span, params):
    for fmt in (P.DEFLATE, P.ZLIB, P.GZIP):
        hdr = P.GZ_HEADER if fmt == P.GZIP else None
        for prime, M in ((True, P), (False, U)):
            want = M.expected(data, span, fmt, header=hdr, **params)
            st, out, sum_ = _spans(eng, data, span, fmt, header=hdr, prime=prime, **params)
            if want is None:  # a span's Queue.Full is the call's
                assert (st, out) == (P.QUEUE_FULL, b"")
                continue
            assert st == 0
            assert out == want, (fmt, prime, len(out), len(want))
            assert sum_ == (zlib.crc32(data) if fmt == P.GZIP else zlib.adler32(data))
            f = M.forms(data, span, **(dict(params, driver=P.ZL, dynamic=True) if fmt == P.GZIP else params))
            assert eng.deflate_spans_last() == {"spans": len(f), "stored_spans": sum(x[0] == "S" for x in f), "span_bytes": span}


def test_repeat_is_small_only_when_primed(eng):
    name, data, span, params = [c for c in CASES if c[0] == "repeat"][0]
    st, out, _ = _spans(eng, data, span, P.DEFLATE)
    assert st == 0 and len(out) < 4096 + 8 * 64 and zlib.decompress(out, -15) == data
    st, out, _ = _spans(eng, data, span, P.DEFLATE, prime=False)
    assert st == 0 and len(out) > 8 * 4096


def test_prefix_chunks_left_out_or_not_same_bytes(eng):
    """deflate_test_flags bit 5: the match kernel also takes the chunks below a span's first position - no byte depends on it"""
    for name in ("growth", "slide-65536", "text40k-dy1-le9"):
        _, data, span, params = [c for c in CASES if c[0] == name][0]
        want = P.expected(data, span, P.ZLIB, **params)
        try:
            eng.set_option("deflate_test_flags", 32)
            st, out, _ = _spans(eng, data, span, P.ZLIB, **params)
        finally:
            eng.set_option("deflate_test_flags", 0)
        assert st == 0 and out == want


def test_dst_cap(eng):
    data, span = U._text(31, 20000), 4096
    for fmt in (P.DEFLATE, P.ZLIB, P.GZIP):
        want = P.expected(data, span, fmt)
        n = len(want)
        lib, p = eng.lib, eng._params(6, 4096, 0, True)
        try:
            eng.set_option("deflate_span_prime", 1)
            for cap, status in ((n, 0), (n - 1, END_OF_OUTPUT), (0, END_OF_OUTPUT)):
                dst = ctypes.create_string_buffer(b"\xa5" * (n + 16), n + 16)
                w = ctypes.c_size_t(123)
                st = lib.md_deflate_spans_host(eng.ctx, fmt, ctypes.byref(p), span, data, len(data), dst, cap, ctypes.byref(w), None)
                assert st == status
                assert dst.raw[cap:] == b"\xa5" * (n + 16 - cap)  # nothing behind dst_cap
                if st == 0:
                    assert w.value == n and dst.raw[:n] == want
                else:
                    assert w.value == 0
        finally:
            eng.set_option("deflate_span_prime", 0)


def test_device_form(eng):
    import torch
    for name, data, span, params in [c for c in CASES if c[0] in ("alternating", "odd-5000", "straddle", "ff-5552")]:
        for fmt in (P.DEFLATE, P.ZLIB, P.GZIP):
            want = P.expected(data, span, fmt, **params)
            d_src = torch.frombuffer(bytearray(data + b"\0" * 16), dtype=torch.uint8).to(eng.device)
            for room, status in ((len(want) + 7, 0), (len(want), 0), (len(want) - 1, END_OF_OUTPUT)):
                d_dst = torch.full((max(room, 1),), 0xa5, dtype=torch.uint8, device=eng.device)[:room]
                written, st, sum_ = eng.deflate_spans_device(d_src, len(data), d_dst, fmt, span=span, prime=True, **params)
                eng.synchronize()
                assert int(st.item()) == status and int(written.item()) == len(want)
                assert int(sum_.item()) & 0xffffffff == (zlib.crc32(data) if fmt == P.GZIP else zlib.adler32(data))
                got = bytes(d_dst.cpu().numpy().tobytes())
                assert got == (want + b"\xa5" * (room - len(want)) if status == 0 else b"\xa5" * room)


def test_option_and_prime_argument(eng):
    from decompress_amd import engine
    data, span = U._text(32, 9000), 2048
    primed, plain = P.expected(data, span, P.ZLIB), U.expected(data, span, P.ZLIB)
    assert primed != plain
    for bad in (2, -1, 100):
        with pytest.raises(engine.Error):
            eng.set_option("deflate_span_prime", bad)
    assert _spans(eng, data, span, P.ZLIB, prime=None)[1] == plain  # the default is 0
    try:
        eng.set_option("deflate_span_prime", 1)
        assert _spans(eng, data, span, P.ZLIB, prime=None)[1] == primed  # None follows the option
        assert _spans(eng, data, span, P.ZLIB, prime=False)[1] == plain
        assert _spans(eng, data, span, P.ZLIB, prime=None)[1] == primed  # ... which a call with prime=False put back
    finally:
        eng.set_option("deflate_span_prime", 0)
    assert _spans(eng, data, span, P.ZLIB, prime=True)[1] == primed
    assert _spans(eng, data, span, P.ZLIB, prime=None)[1] == plain  # the old value is back after prime=True
    # every other entry point keeps its bytes whatever the option says
    try:
        eng.set_option("deflate_span_prime", 1)
        st, out, _ = eng.deflate_one(data, P.ZLIB, level=6)
        assert st == 0 and out == U.expected(data, 1 << 20, P.ZLIB)
    finally:
        eng.set_option("deflate_span_prime", 0)


def test_workspace_cap_slices_primed_spans(eng):
    """with a workspace cap the primed spans go through the deflate launch in slices of positions: same bytes"""
    data, span = U._text(33, 600 << 10), 200 << 10
    want = P.expected(data, span, P.ZLIB)
    grid = [c for c in CASES if c[0] == "text40k-dy1-le6"][0]
    for cap, (d, s, params) in ((3, (data, span, {})), (1, grid[1:])):
        try:
            eng.set_option("deflate_workspace_cap_mib", cap)
            st, out, sum_ = _spans(eng, d, s, P.ZLIB, **params)
        finally:
            eng.set_option("deflate_workspace_cap_mib", 0)
        assert st == 0 and out == (want if cap == 3 else P.expected(d, s, P.ZLIB, **params)) and sum_ == zlib.adler32(d)
    assert _spans(eng, data, span, P.ZLIB)[1] == want  # (and without a cap)


def test_round_trips(eng):
    from decompress_amd import de, gz, zl
    data = b"".join(U._text(40 + i, 3000) if i % 3 else U._rand(40 + i, 3000) for i in range(9))
    d = de.compress_spans(data, level=6, span=4096, prime=True)
    z = zl.compress_spans(data, level=9, span=1000, prime=True)
    g = gz.compress_spans(data, 4, 5000, filename=b"a.txt", comment=b"c", mtime=77, prime=True)
    assert d == P.expected(data, 4096, P.DEFLATE) and z == P.expected(data, 1000, P.ZLIB, level=9)
    assert g == P.expected(data, 5000, P.GZIP, level=4, header=dict(filename=b"a.txt", comment=b"c", mtime=77))
    assert de.Higher.uncompress(d, len(data)) == data
    assert zl.Higher.uncompress(z, len(data)) == data
    r = gz.Higher.uncompress(g, len(data))
    assert r[0] == "Ok" and r[2] == data and r[1]["filename"] == b"a.txt" and r[1]["mtime"] == 77
    for s, fmt in ((d, P.DEFLATE), (z, P.ZLIB), (g, P.GZIP)):
        chunks = [s[i:i + 777] for i in range(0, len(s), 777)]
        verdict, out, _ = de.Inf.decode_chunks(chunks, o_len=4096, fmt=fmt)
        assert (verdict, out) == ("Ok", data)
    assert zlib.decompress(z) == data and zlib.decompress(g, 31) == data and zlib.decompress(d, -15) == data


def test_one_mib_through_the_long_stream_decoder(eng):
    from decompress_amd import zl
    data = U._text(50, 1 << 20)
    z = zl.compress_spans(data, level=6, span=64 << 10, prime=True)
    assert eng.deflate_spans_last()["spans"] == 16
    assert z == P.expected(data, 64 << 10, P.ZLIB)
    assert len(z) < len(zl.compress_spans(data, level=6, span=64 << 10))
    assert zlib.decompress(z) == data
    assert zl.Higher.uncompress(z, len(data)) == data


def test_cli_prime(eng, tmp_path):
    data = U._text(51, 30000)
    src, dst, back = tmp_path / "in", tmp_path / "out.z", tmp_path / "back"
    src.write_bytes(data)
    tool = [sys.executable, "-m", "decompress_amd.cli"]
    subprocess.check_call(tool + ["-d", "-f", "zlib", "-l", "6", "--span", "4", "--prime", str(src), str(dst)])
    assert dst.read_bytes() == P.expected(data, 4096, P.ZLIB)
    subprocess.check_call(tool + ["-f", "zlib", str(dst), str(back)])
    assert back.read_bytes() == data
    from decompress_amd import cli
    assert cli.main(["-d", "-f", "zlib", "--prime", str(src), str(dst)]) == cli.CLI_ERROR  # --prime needs --span


def test_front_workspace_of_one_primed_span(eng):
    """the front kernels see X_i as the stream it is, so the existing models apply unchanged: link[] is lz77_model.links(X_i),
    and a verdict at a position >= first is what look_ahead(X_i) says"""
    import numpy as np

    from tests import deflate_front_probe, lz77_model
    data = U._text(80, (48 << 10) + 1)
    s, e, w = P.prefixes(len(data), 4096)[10]
    assert w == 32768
    x = data[s - w:e]
    res = deflate_front_probe.run([x], 0, 6)
    dist, _ = lz77_model.links(x, 0)
    assert (res.link(0) & 0xFFFF).tolist() == dist
    flg, m, mq = res.flg(0), res.m(0), res.mq(0)
    positions = range(w, len(dist))
    look = lz77_model.look_ahead(x, 0, 6, positions)
    settled = 0
    for p in positions:
        lk = look[p]
        if flg[p] == 2:  # FL_ENDED
            assert not lk.share3, p
        elif flg[p] == 4:  # FL_MATCH
            assert not lk.near_end and (int(m[p]) >> 16, int(mq[p]) >> 16) == (lk.full[0], lk.quarter[0]), p
            assert (int(m[p]) & 0xFFFF) == lk.full[1] and (lk.quarter[0] <= 2 or (int(mq[p]) & 0xFFFF) == lk.quarter[1]), p
        else:
            assert flg[p] == 0 and (lk.near_end or lk.walked > 128), p
        settled += int(flg[p] != 0)
    assert settled > 3000
    assert np.isin(flg[w:], (0, 2, 4)).all()
