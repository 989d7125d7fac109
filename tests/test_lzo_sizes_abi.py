"""CPU-side checks of the LZO size query (md_lzo_sizes_batch_*, md_lzo_uncompress_with_buffer): declared,
exported and bound; the new status and its string; misuse refused without a device."""
import ctypes
import os
import re

from decompress_amd import _lib, build, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["md_lzo_sizes_batch_device", "md_lzo_sizes_batch_host", "md_lzo_uncompress_with_buffer"]
INVALID_ARGUMENT = -1


def test_declared_exported_bound():
    build.build()
    hdr = open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    so = ctypes.CDLL(_lib.SO)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert hasattr(so, f), f
        assert f in bound, f
    assert "format-blind" in hdr  # md_inflate_plan_device says that it serves LZO too
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for f in FUNCS:
        assert f in doc, f


def test_status_17():
    hdr = open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    assert re.search(r"MD_LZO_MALFORMED_INPUT\s*=\s*17\b", hdr)
    lib = _lib.load()
    assert lib.md_status_string(17) == b"Malformed input"
    assert lib.md_status_string(4) == b"Invalid dictionary"
    assert lib.md_status_string(16) == b"Input is malformed or output is not large enough"  # (as before)
    assert engine.STATUS_NAMES[17] == "Malformed input" and engine.STATUS_CODES["Malformed input"] == 17


def test_null_context_refused():
    lib = _lib.load()
    a = (ctypes.c_uint64 * 4)()
    p = ctypes.addressof(a)
    st = (ctypes.c_int32 * 4)()
    assert lib.md_lzo_sizes_batch_device(None, 1, p, p, p, p, ctypes.addressof(st)) == INVALID_ARGUMENT
    assert lib.md_lzo_sizes_batch_host(None, 1, p, 8, p, p, p, ctypes.addressof(st)) == INVALID_ARGUMENT
    dst, n = ctypes.c_void_p(), ctypes.c_size_t()
    assert lib.md_lzo_uncompress_with_buffer(None, b"\x11\0\0", 3, ctypes.byref(dst), ctypes.byref(n)) == INVALID_ARGUMENT
    assert not dst.value and n.value == 0


def test_count_kernel_residency(tmp_path):
    """md::lzo::lzo_count_kernel from the code object: the input ring is all its LDS, no scratch, and registers for eight
    wavefronts per SIMD (DESIGN 4c states the figures)"""
    from tests.test_inf_batch_abi import _all_kernel_metadata
    build.build()
    kernels = _all_kernel_metadata(_lib.SO, tmp_path)
    count = {k: v for k, v in kernels.items() if "lzo_count_kernel" in k}
    assert len(count) == 1, sorted(k for k in kernels if "lzo" in k)
    for name, k in count.items():
        assert k["group_segment_fixed_size"] <= 2048 + 64, (name, k)
        assert k["vgpr_count"] <= 64, (name, k)
        assert k["private_segment_fixed_size"] == 0, (name, k)
