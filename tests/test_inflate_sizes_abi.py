"""CPU-side checks of the decoder's size query (md_inflate_sizes_batch_*, md_inflate_plan_device): declared,
exported and bound; misuse refused without a device; and the residency of md::wv::inflate_count_kernel read from the
code object - LDS <= 8 192 B (20 streams per CU), <= 96 VGPRs (five wavefronts per SIMD), no more scratch than the decode
kernel is allowed - with no scratch at all in the finish and plan kernels."""
import ctypes
import os
import re

from decompress_amd import _lib, build
from tests.test_inf_batch_abi import _all_kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["md_inflate_sizes_batch_device", "md_inflate_sizes_batch_host", "md_inflate_plan_device"]
INVALID_ARGUMENT = -1


def test_declared_exported_bound():
    build.build()
    assert "inflate_count.hip" in build.SOURCES and "capi_inflate_sizes.cpp" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    so = ctypes.CDLL(_lib.SO)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert hasattr(so, f), f
        assert f in bound, f
    assert "cannot see this" in hdr  # the contract's wording for MD_INVALID_CHECKSUM


def test_misuse_refused_without_device():
    lib = _lib.load()
    assert re.search(r"MD_E_INVALID_ARGUMENT\s*=\s*-1\b", open(os.path.join(ROOT, "include", "mdeflate.h")).read())
    a = (ctypes.c_uint64 * 4)()
    p = ctypes.addressof(a)
    st = (ctypes.c_int32 * 4)()
    # a NULL context
    assert lib.md_inflate_sizes_batch_device(None, 0, 1, p, p, p, p, p, ctypes.addressof(st)) == INVALID_ARGUMENT
    assert lib.md_inflate_sizes_batch_host(None, 0, 1, p, 8, p, p, p, p, ctypes.addressof(st)) == INVALID_ARGUMENT
    assert lib.md_inflate_plan_device(None, 1, p, 256, p, p, p) == INVALID_ARGUMENT
    ctx = lib.md_create(0, None)
    if not ctx:  # (md_create needs a device: the checks below run where there is one)
        return
    try:
        for fmt in (-1, 3, 99):  # an unknown format
            assert lib.md_inflate_sizes_batch_device(ctx, fmt, 1, p, p, p, p, p, ctypes.addressof(st)) == INVALID_ARGUMENT
            assert lib.md_inflate_sizes_batch_host(ctx, fmt, 1, p, 8, p, p, p, p, ctypes.addressof(st)) == INVALID_ARGUMENT
        for k in range(6):  # a NULL array with n != 0
            args = [p, p, p, p, p, ctypes.addressof(st)]
            args[k] = None
            assert lib.md_inflate_sizes_batch_device(ctx, 0, 1, *args) == INVALID_ARGUMENT, k
        assert lib.md_inflate_sizes_batch_device(ctx, 0, 0, None, None, None, None, None, None) == 0
        for align in (0, 3, 6, 255, 257):  # not a power of two
            assert lib.md_inflate_plan_device(ctx, 1, p, align, p, p, p) == INVALID_ARGUMENT, align
        assert lib.md_inflate_plan_device(ctx, 1, None, 1, p, p, p) == INVALID_ARGUMENT
        assert lib.md_inflate_plan_device(ctx, 1, p, 1, p, p, None) == INVALID_ARGUMENT
    finally:
        lib.md_destroy(ctx)


def test_count_kernel_residency(tmp_path):
    build.build()
    kernels = _all_kernel_metadata(_lib.SO, tmp_path)
    count = {k: v for k, v in kernels.items() if "inflate_count_kernel" in k}
    assert count, sorted(k for k in kernels if "inflate" in k)
    for name, k in count.items():
        assert k["group_segment_fixed_size"] <= 8192, (name, k)
        assert k["vgpr_count"] <= 96, (name, k)
        assert k["private_segment_fixed_size"] <= 40, (name, k)
    for want in ("sizes_gz_finish_kernel", "inflate_plan_kernel"):
        mine = {k: v for k, v in kernels.items() if want in k}
        assert mine, want
        for name, k in mine.items():
            assert k["private_segment_fixed_size"] == 0, (name, k)
