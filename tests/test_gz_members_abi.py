"""CPU-side checks of the many-member GZip entry points (md_gz_members_*, md_bgzf_*): declared, exported and
bound; the bound's arithmetic; misuse refused without a device; the new kernels use no scratch; the files the GPU tests
feed are good by Python's gzip; and the two facts about Gz.Inf's reading (MD_FORMAT_GZIP, restated in oracle/gz.c) that
make these entry points necessary."""
import ctypes
import gzip
import os
import random
import re

from decompress_amd import _lib, build
from tests import gz_members_util as gu
from tests.test_inf_batch_abi import _all_kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["md_gz_members_scan", "md_gz_members_uncompress", "md_bgzf_compress_bound", "md_bgzf_compress"]
KERNELS = ["mark_kernel", "scan_kernel", "compact_kernel", "link_kernel", "jump_kernel", "select_kernel", "header_kernel",
           "verdict_kernel", "bgzf_plan_kernel", "bgzf_size_kernel", "bgzf_pack_kernel"]


def test_declared_exported_bound():
    build.build()
    assert "gz_members.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    so = ctypes.CDLL(_lib.SO)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert hasattr(so, f), f
        assert f in bound, f
    assert "md_gz_members_info" in hdr and ctypes.sizeof(_lib.GzMembersInfo) == 3 * ctypes.sizeof(ctypes.c_size_t) + 8


def test_compress_bound_formula():
    lib = _lib.load()
    for block in (1, 7, 4096, 0xff00 - 1, 0xff00):
        for k in (0, 1, 2, 3, 1000):
            for d in (-1, 0, 1):
                n = k * block + d
                if n < 0:
                    continue
                nb = -(-n // block)
                # per block 26 + 5 + its bytes (the stored form, the worst case), + 28 for the EOF marker
                assert lib.md_bgzf_compress_bound(n, block) == n + 31 * nb + 28, (n, block)
    assert lib.md_bgzf_compress_bound(0, 0) == 28
    assert lib.md_bgzf_compress_bound(0xff00 + 1, 0) == 0xff00 + 1 + 62 + 28  # block 0 = the default, 0xff00
    assert lib.md_bgzf_compress_bound(10, 0xff01) == 0  # out of range


def test_misuse_refused_without_device():
    lib = _lib.load()
    info = _lib.GzMembersInfo()
    w = ctypes.c_size_t()
    dst = ctypes.create_string_buffer(64)
    assert lib.md_gz_members_scan(None, b"x", 1, ctypes.byref(info), None, None, 0) < 0
    assert lib.md_gz_members_uncompress(None, b"x", 1, dst, 64, ctypes.byref(info)) < 0
    assert lib.md_bgzf_compress(None, 6, 0, b"x", 1, dst, 64, ctypes.byref(w)) < 0


def test_new_kernels_use_no_scratch(tmp_path):
    build.build()
    kernels = _all_kernel_metadata(_lib.SO, tmp_path)
    mine = {k: v for k, v in kernels.items() if "2md3gzm" in k}  # namespace md::gzm
    for want in KERNELS:
        assert any(want in k for k in mine), (want, sorted(mine))
    assert len(mine) == len(KERNELS) + 1, sorted(mine)  # (the scan in two widths)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0, (name, k)


def _helper_files():
    rng = random.Random(5)
    text = bytes(rng.choice(b"abcdefgh \n") for _ in range(200000))
    yield gu.bgzf_file(text)[0], text
    yield gu.bgzf_file(text, eof=False)[0], text
    yield gu.bgzf_file(text, block=1000)[0] + b"\0" * 100, text
    yield gu.bgzf_file(text[:5000], block=1)[0], text[:5000]
    yield gu.bgzf_of_members([b"ab", b"", b"", b"cd"])[0], b"abcd"
    yield gu.bgzf_file(text, before=gu.subfield(b"XY", b"12345"), after=gu.subfield(b"ZZ", b""))[0], text
    yield gu.member(b"abc", name=b"n", comment=b"c", hcrc=True, extra=gu.subfield(b"AB", b"xyz")) + gu.member(b"def"), b"abcdef"
    yield gu.bgzf_member(b"abc") + gu.member(b"def", hcrc=True) + gu.bgzf_member(b"ghi"), b"abcdefghi"


def test_helper_files_are_good_gzip():
    for f, plain in _helper_files():
        assert gzip.decompress(f) == plain
        assert gu.libz_members(f)[:2] == ("ok", plain)
    f, idx = gu.bgzf_file(b"x" * 200000)
    offs, end = gu.walk_bsize(f)
    assert offs == [c for c, _ in idx] and end == len(f) and f[-28:] == gu.EOF_MARKER


def test_gz_inf_stops_after_one_member(oracle):
    """Gz.Inf's contract (and so MD_FORMAT_GZIP's): one member, the rest is left in the source"""
    two = gzip.compress(b"a" * 100, mtime=0) + gzip.compress(b"b" * 100, mtime=0)
    assert len(two) == 48
    st, used, out, _ = oracle.gz_inflate(two, 1 << 16)
    assert (st, used, out) == (0, 24, b"a" * 100)


def test_gz_inf_cannot_read_a_bgzf_block(oracle):
    """Gz.Inf reads FEXTRA's XLEN big-endian (lib/gz.ml:455): the RFC's 06 00 is 1 536 bytes of extra field to it"""
    blk = gu.bgzf_member(b"hello bgzf world " * 1000)
    assert gzip.decompress(blk + gu.EOF_MARKER) == b"hello bgzf world " * 1000
    st = oracle.gz_inflate(blk, 1 << 16)[0]
    assert st != 0 and oracle.status_string(st) == "Unexpected end of input"
