"""One stream written as joined spans on the GPU (md_deflate_spans_*; csrc/deflate_spans.hip).  Needs an MI355X:
`pytest -m gpu`.  The yardstick is tests/deflate_spans_model.py - the definition restated over the oracle's per-span bodies -
and the bytes must equal it exactly in all three formats; libz and this library's own decoders read every stream back."""
import ctypes
import subprocess
import sys
import zlib

import pytest

from tests import deflate_spans_model as M

pytestmark = pytest.mark.gpu
CASES = M.cases()
END_OF_OUTPUT = 2


@pytest.fixture(scope="module")
def eng():
    from decompress_amd import engine
    return engine.default_engine(0)


def _spans(eng, data, span, fmt, header=None, cap=None, **params):
    return eng.deflate_spans(data, fmt, span=span, header=header, cap=cap, **params)


@pytest.mark.parametrize("name,data,span,params", CASES, ids=[c[0] for c in CASES])
def test_bytes_equal_the_model(eng, name, data, span, params):
    for fmt in (M.DEFLATE, M.ZLIB, M.GZIP):
        hdr = M.GZ_HEADER if fmt == M.GZIP else None
        want = M.expected(data, span, fmt, header=hdr, **params)
        st, out, sum_ = _spans(eng, data, span, fmt, header=hdr, **params)
        if want is None:  # a span's Queue.Full is the call's
            assert (st, out) == (M.QUEUE_FULL, b"")
            continue
        assert st == 0
        assert out == want, (fmt, len(out), len(want))
        assert sum_ == (zlib.crc32(data) if fmt == M.GZIP else zlib.adler32(data))
        last = eng.deflate_spans_last()
        f = M.forms(data, span, **(dict(params, driver=M.ZL, dynamic=True) if fmt == M.GZIP else params))
        assert last == {"spans": len(f), "stored_spans": sum(x[0] == "S" for x in f), "span_bytes": span}


def test_dst_cap(eng):
    data, span = M._text(31, 20000), 4096
    for fmt in (M.DEFLATE, M.ZLIB, M.GZIP):
        want = M.expected(data, span, fmt)
        n = len(want)
        lib, p = eng.lib, eng._params(6, 4096, 0, True)
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


def test_device_form(eng):
    import torch
    for name, data, span, params in [c for c in CASES if c[0] in ("alternating", "small-7-22", "small-1-0", "ff-5552")]:
        for fmt in (M.DEFLATE, M.ZLIB, M.GZIP):
            want = M.expected(data, span, fmt, **params)
            d_src = torch.frombuffer(bytearray(data + b"\0" * 16), dtype=torch.uint8).to(eng.device)
            for room, status in ((len(want) + 7, 0), (len(want), 0), (len(want) - 1, END_OF_OUTPUT)):
                d_dst = torch.full((max(room, 1),), 0xa5, dtype=torch.uint8, device=eng.device)[:room]
                written, st, sum_ = eng.deflate_spans_device(d_src, len(data), d_dst, fmt, span=span, **params)
                eng.synchronize()
                assert int(st.item()) == status and int(written.item()) == len(want)
                assert int(sum_.item()) & 0xffffffff == (zlib.crc32(data) if fmt == M.GZIP else zlib.adler32(data))
                got = bytes(d_dst.cpu().numpy().tobytes())
                assert got == (want + b"\xa5" * (room - len(want)) if status == 0 else b"\xa5" * room)
            f = M.forms(data, span, **(dict(params, driver=M.ZL, dynamic=True) if fmt == M.GZIP else params))
            assert eng.deflate_spans_last() == {"spans": len(f), "stored_spans": sum(x[0] == "S" for x in f), "span_bytes": span}


def test_span_option_and_arguments(eng):
    data = M._text(32, 5000)
    try:
        eng.set_option("deflate_span_kib", 2)
        st, out, _ = _spans(eng, data, None, M.ZLIB)
        assert st == 0 and out == M.expected(data, 2048, M.ZLIB)
        assert eng.deflate_spans_last()["span_bytes"] == 2048
    finally:
        eng.set_option("deflate_span_kib", 0)
    _spans(eng, data, None, M.ZLIB)
    assert eng.deflate_spans_last() == {"spans": 1, "stored_spans": 0, "span_bytes": 64 << 10}
    from decompress_amd import engine
    for bad in (dict(level=10), dict(level=-1), dict(driver=3), dict(matcher=2), dict(queue=100)):
        with pytest.raises(engine.Error):
            _spans(eng, data, 1024, M.DEFLATE, **bad)
    with pytest.raises(engine.Error):
        _spans(eng, data, 1024, 3)
    p = eng._params(6, 4096, 0, True)
    p.wbits = 14
    w = ctypes.c_size_t()
    assert eng.lib.md_deflate_spans_host(eng.ctx, 0, ctypes.byref(p), 1024, data, len(data), ctypes.create_string_buffer(8192), 8192,
                                         ctypes.byref(w), None) == -1
    p.wbits = 15
    assert eng.lib.md_deflate_spans_host(eng.ctx, 0, ctypes.byref(p), 1024, data, len(data), ctypes.create_string_buffer(8192), 8192,
                                         ctypes.byref(w), None) == 0


def test_workspace_cap_slices_spans(eng):
    """with a workspace cap the spans go through the deflate launch in slices of positions: same bytes"""
    data, span = M._text(33, 600 << 10), 200 << 10
    want = M.expected(data, span, M.ZLIB)
    try:
        eng.set_option("deflate_workspace_cap_mib", 3)
        st, out, _ = _spans(eng, data, span, M.ZLIB)
    finally:
        eng.set_option("deflate_workspace_cap_mib", 0)
    assert st == 0 and out == want


def test_stored_span_that_runs_out_of_room_in_an_early_slice(eng):
    """a batch in slices of positions, and spans of random bytes in fixed blocks (5 % longer than the text): their slots run
    out some 5 % in front of their end, slices before the last one, where the encoder's Adler-32 has not seen the whole
    span.  The stream's Adler-32 and the call's checksum are the text's all the same."""
    span = 1536 << 10
    data = M._rand(60, span) + M._rand(61, span) + M._text(62, 100 << 10)
    params = dict(level=1, dynamic=False)
    assert [f[0] for f in M.forms(data, span, **params)] == ["S", "S", "J"]
    try:
        eng.set_option("deflate_workspace_cap_mib", 1)  # slices of 64 KiB: 24 a span
        for fmt in (M.ZLIB, M.DEFLATE):
            st, out, sum_ = _spans(eng, data, span, fmt, **params)
            assert st == 0 and sum_ == zlib.adler32(data)
            assert out == M.expected(data, span, fmt, **params)
    finally:
        eng.set_option("deflate_workspace_cap_mib", 0)
    assert zlib.decompress(M.expected(data, span, M.ZLIB, **params)) == data


def test_round_trips(eng):
    from decompress_amd import de, gz, zl
    data = b"".join(M._text(40 + i, 3000) if i % 3 else M._rand(40 + i, 3000) for i in range(9))
    d = de.compress_spans(data, level=6, span=4096)
    z = zl.compress_spans(data, level=9, span=1000)
    g = gz.compress_spans(data, 4, 5000, filename=b"a.txt", comment=b"c", mtime=77)
    assert d == M.expected(data, 4096, M.DEFLATE) and z == M.expected(data, 1000, M.ZLIB, level=9)
    assert g == M.expected(data, 5000, M.GZIP, level=4, header=dict(filename=b"a.txt", comment=b"c", mtime=77))
    assert de.Higher.uncompress(d, len(data)) == data
    assert zl.Higher.uncompress(z, len(data)) == data
    r = gz.Higher.uncompress(g, len(data))
    assert r[0] == "Ok" and r[2] == data and r[1]["filename"] == b"a.txt" and r[1]["mtime"] == 77
    for s, fmt in ((d, M.DEFLATE), (z, M.ZLIB), (g, M.GZIP)):
        chunks = [s[i:i + 777] for i in range(0, len(s), 777)]
        verdict, out, _ = de.Inf.decode_chunks(chunks, o_len=4096, fmt=fmt)
        assert (verdict, out) == ("Ok", data)
    assert zlib.decompress(z) == data and zlib.decompress(g, 31) == data and zlib.decompress(d, -15) == data


def test_one_mib_through_the_long_stream_decoder(eng):
    from decompress_amd import zl
    data = M._text(50, 1 << 20)
    z = zl.compress_spans(data, level=6, span=64 << 10)
    assert eng.deflate_spans_last()["spans"] == 16
    assert zlib.decompress(z) == data
    assert zl.Higher.uncompress(z, len(data)) == data


def test_cli_span(eng, tmp_path):
    from decompress_amd import zl
    data = M._text(51, 30000)
    src, dst, back = tmp_path / "in", tmp_path / "out.z", tmp_path / "back"
    src.write_bytes(data)
    tool = [sys.executable, "-m", "decompress_amd.cli"]
    subprocess.check_call(tool + ["-d", "-f", "zlib", "-l", "6", "--span", "4", str(src), str(dst)])
    assert dst.read_bytes() == zl.compress_spans(data, level=6, span=4096) == M.expected(data, 4096, M.ZLIB)
    subprocess.check_call(tool + ["-f", "zlib", str(dst), str(back)])
    assert back.read_bytes() == data
