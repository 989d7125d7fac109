"""CPU-side checks of the speculative reader of many-member GZip files (md_gz_members_last, csrc/gz_spec.hip; DESIGN
4f): the query is declared, exported and bound, its struct has the header's size, misuse is refused without a device, the
new file is built, and the kernels of its namespace use no scratch memory."""
import ctypes
import os
import re

from decompress_amd import _lib, build
from tests.test_inf_batch_abi import _all_kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ["mark_kernel", "compact_kernel", "span_kernel", "classify_kernel", "room_kernel", "verify_kernel"]


def test_declared_exported_bound():
    build.build()
    assert "gz_spec.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    so = ctypes.CDLL(_lib.SO)
    assert re.search(r"\bint\s+md_gz_members_last\s*\(\s*const\s+md_ctx\s*\*", hdr)
    assert hasattr(so, "md_gz_members_last")
    assert "md_gz_members_last" in {name for name, _, _ in _lib.SYMBOLS}
    assert '"gz_members_speculate"' in hdr


def test_stats_struct_matches_header():
    hdr = open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    body = re.search(r"typedef struct md_gz_members_stats \{(.*?)\} md_gz_members_stats;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(ctype, n.strip()) for n in names.split(",")]
    assert [n for _, n in fields] == [n for n, _ in _lib.GzMembersStats._fields_]
    assert [t for t, _ in fields] == ["int"] + ["size_t"] * 7
    # an int, padded to the alignment of the seven size_t behind it
    assert ctypes.sizeof(_lib.GzMembersStats) == 8 * ctypes.sizeof(ctypes.c_size_t)
    # md_gz_members_info keeps its layout
    assert ctypes.sizeof(_lib.GzMembersInfo) == 3 * ctypes.sizeof(ctypes.c_size_t) + 8


def test_misuse_refused_without_device():
    lib = _lib.load()
    s = _lib.GzMembersStats()
    assert lib.md_gz_members_last(None, ctypes.byref(s)) < 0
    assert lib.md_gz_members_last(None, None) < 0
    # (a context that is not NULL needs a device: NULL `out` with a live context is in tests/test_gpu_gz_members_spec.py)


def test_spec_kernels_use_no_scratch(tmp_path):
    build.build()
    kernels = _all_kernel_metadata(_lib.SO, tmp_path)
    mine = {k: v for k, v in kernels.items() if "2md3gzs" in k}  # namespace md::gzs
    for want in KERNELS:
        assert any(want in k for k in mine), (want, sorted(mine))
    assert len(mine) == len(KERNELS), sorted(mine)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0, (name, k)
