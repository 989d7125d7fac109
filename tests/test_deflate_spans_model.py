"""CPU-side checks of the writer of joined spans (md_deflate_spans_*): the model of its output (tests/
deflate_spans_model.py) is a stream that libz and the oracle's inflaters read to the end, one span is the oracle's whole
stream, the case list really holds every joint there is, the bound covers every case, and the entry points are declared,
exported and bound."""
import ctypes
import os
import re
import zlib

import pytest

from decompress_amd import _lib, build
from tests import deflate_spans_model as M
from tests.test_inf_batch_abi import _all_kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["md_deflate_spans_bound", "md_deflate_spans_host", "md_deflate_spans_device", "md_deflate_spans_last"]
CASES = M.cases()


def test_declared_exported_bound():
    build.build()
    assert "deflate_spans.hip" in build.SOURCES and "capi_deflate_spans.cpp" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    so = ctypes.CDLL(_lib.SO)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert hasattr(so, f), f
        assert f in bound, f
    assert "md_deflate_spans_info" in hdr and ctypes.sizeof(_lib.DeflateSpansInfo) == 3 * ctypes.sizeof(ctypes.c_size_t)
    assert '"deflate_span_kib"' in hdr


def test_misuse_refused_without_device():
    lib = _lib.load()
    w, dst = ctypes.c_size_t(), ctypes.create_string_buffer(64)
    p = _lib.DeflateParams(6, 4096, 0, 1, 0, None, 0, 0)
    assert lib.md_deflate_spans_host(None, 0, ctypes.byref(p), 4, b"x", 1, dst, 64, ctypes.byref(w), None) < 0
    assert lib.md_deflate_spans_last(None, None) < 0
    assert lib.md_deflate_spans_bound(3, 10, 4, None) == 0  # no such format
    assert lib.md_deflate_spans_bound(0, 10, 0xfffffff1, None) == 0  # a span above MD_MAX_STREAM
    long_name = _lib.GzHeader(0, 3, 0, 0, b"n" * 256, None)
    assert lib.md_deflate_spans_bound(2, 10, 4, ctypes.byref(long_name)) == 0


def test_new_kernels_use_no_scratch(tmp_path):
    build.build()
    mine = {k: v for k, v in _all_kernel_metadata(_lib.SO, tmp_path).items() if "2md3spn" in k}  # namespace md::spn
    for want in ("plan_kernel", "size_kernel", "join_kernel"):
        assert any(want in k for k in mine), (want, sorted(mine))
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0, (name, k)


def test_closing_block_walker():
    # a stored block alone; a fixed block alone (the empty stream 03 00: header at bit 0, 3 + 7 bits); two blocks
    assert M.closing_block(b"\x01\x03\x00\xfc\xffabc") == (0, 64, 0)
    assert M.closing_block(b"\x03\x00") == (0, 10, 1)
    two = b"\x00\x01\x00\xfe\xffa" + b"\x03\x00"
    assert M.closing_block(two) == (48, 58, 1)
    assert zlib.decompress(two, -15) == b"a"
    # the joined form of 03 00 is the sync flush of an empty fixed block: 02 00 | 00 00 ff ff
    assert M.joined_form(b"\x03\x00", 0, 10) == b"\x02\x00\x00\x00\xff\xff"
    # e on a byte boundary: the three bits need a byte of their own
    assert M.joined_form(b"\x01\x00\x00\xff\xff", 0, 40) == b"\x00\x00\x00\xff\xff" + b"\x00" + b"\x00\x00\xff\xff"
    assert M.stored_form(b"", True) == b"\x01\x00\x00\xff\xff"
    s = M.stored_form(b"x" * 65536, False)
    assert len(s) == 65536 + 10 and s[:5] == b"\x00\xff\xff\x00\x00" and s[65540:65545] == b"\x00\x01\x00\xfe\xff"


@pytest.mark.parametrize("name,data,span,params", CASES, ids=[c[0] for c in CASES])
def test_expected_is_a_stream_every_inflater_reads(oracle, name, data, span, params):
    lib = _lib.load()
    # (libz does not take the header CRC as Gz.Def writes it - the upper half, big-endian: it reads the header without one)
    plain = dict(M.GZ_HEADER, hcrc=False)
    for fmt, wbits, hdr in ((M.DEFLATE, -15, None), (M.ZLIB, 15, None), (M.GZIP, 31, plain), (M.GZIP, None, M.GZ_HEADER)):
        want = M.expected(data, span, fmt, header=hdr, **params)
        if want is None:  # Queue.Full (the CLI driver with a short queue): nothing to read
            assert params.get("driver") == M.CLI
            continue
        if wbits is not None:
            d = zlib.decompressobj(wbits)
            assert d.decompress(want) == data and d.eof and d.unused_data == b""
        cap = len(data) + 64
        if fmt == M.DEFLATE:
            assert oracle.de_inflate(want, cap) == (0, len(want), data)
        elif fmt == M.ZLIB:
            assert oracle.zl_inflate(want, cap) == (0, len(want), data)
        else:
            st, used, out, meta = oracle.gz_inflate(want, cap)
            assert (st, used, out) == (0, len(want), data) and meta["name"] == b"spans.txt" and meta["comment"] == b"joined"
        gz = _lib.GzHeader(hdr["mtime"], hdr["os"], int(hdr["hcrc"]), int(hdr["ascii"]), hdr["filename"], hdr["comment"]) if hdr else None
        bound = lib.md_deflate_spans_bound(fmt, len(data), span, ctypes.byref(gz) if gz else None)
        assert bound >= len(want), (bound, len(want))
        if span >= 1024:  # span 0: the bound of the smallest span the option selects
            assert lib.md_deflate_spans_bound(fmt, len(data), 0, ctypes.byref(gz) if gz else None) >= bound


def test_one_span_is_the_whole_stream(oracle):
    for data, params in ((b"", {}), (M._text(3, 5000), {}), (M._text(4, 30000), dict(level=9, queue=256)),
                         (M._text(5, 3000), dict(level=1, dynamic=False)), (M._text(6, 100), dict(level=0))):
        raw, _ = oracle.deflate_raw(data, params.get("level", 6), params.get("queue", 4096), 0, params.get("dynamic", True), 0)
        for span in (max(1, len(data)), len(data) + 1, 1 << 20):
            assert M.forms(data, span, **params)[0][0] == "J"
            assert M.expected(data, span, M.DEFLATE, **params) == raw
            if params.get("dynamic", True):
                assert M.expected(data, span, M.ZLIB, **params) == oracle.zl_deflate(data, params.get("level", 6), params.get("queue", 4096), True)
                assert M.expected(data, span, M.GZIP, **params) == oracle.gz_deflate(data, params.get("level", 6), params.get("queue", 4096))


def test_case_list_covers_every_joint():
    """asserted, not assumed: every e mod 8 at a joint, both marker lengths, fixed and dynamic closing blocks at a joint, a
    stored closing block (it survives in the last span alone: at a joint it ends on a byte, the marker takes five bytes, and
    the stored form is the shorter one), stored-form spans - as first, inner and last span, next to joined spans both ways
    round - and a stored span split at 65 535"""
    e_mod, markers, closing, pairs, stored_at, split = set(), set(), set(), set(), set(), False
    for name, data, span, params in CASES:
        f = M.forms(data, span, **params)
        if f is None:
            continue
        for i, (form, e, marker, bt) in enumerate(f):
            if form == "J":
                closing.add(bt)
                assert bt != 0 or i + 1 == len(f)
            if form == "J" and i + 1 < len(f):
                e_mod.add(e)
                markers.add(marker)
                assert marker == (4 if (8 - e) % 8 >= 3 else 5)
            if form == "S":
                stored_at.add("first" if i == 0 else "last" if i + 1 == len(f) else "inner")
                split = split or len(M.spans_of(data, span)[i]) > 65535
            if i:
                pairs.add(f[i - 1][0] + form)
    assert e_mod == set(range(8)), e_mod
    assert markers == {4, 5}
    assert closing == {0, 1, 2}, closing  # stored, fixed and dynamic closing blocks
    assert pairs == {"JJ", "JS", "SJ", "SS"}, pairs
    assert stored_at == {"first", "inner", "last"}, stored_at
    assert split
    full = [name for name, data, span, params in CASES if M.forms(data, span, **params) is None]
    assert full == ["queue-full"]  # a span's Queue.Full, and only where it is meant


def test_cli_refuses_span_where_it_means_nothing(capsys):
    from decompress_amd import cli
    for argv in (["--span", "4"], ["--span=4", "-f", "zlib"], ["-d", "-f", "lzo", "--span", "4"], ["-d", "--span", "0"], ["-d", "--span"]):
        assert cli.main(argv) == cli.CLI_ERROR, argv
        assert "pan" in capsys.readouterr().err
    assert cli.take_span(["-d", "--span", "4", "-f", "zlib", "in"]) == (["-d", "-f", "zlib", "in"], 4096)
