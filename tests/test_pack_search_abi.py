"""CPU-side checks of the base search's entry points (md_pack_sketch_*, md_pack_delta_sizes_*, md_pack_choose_bases,
md_pack_search_last): declared, exported and bound; the stats struct has the size the header declares; the
header's constants are pack_search.hpp's and the model's; pack_search.hpp has no HIP in it; misuse is refused without a
device; and "choosing bases" has left the out-of-scope lists."""
import ctypes
import os
import re

from decompress_amd import _lib, build
from decompress_amd import pack as mp
from tests import pack_search_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["md_pack_sketch_device", "md_pack_sketch_host", "md_pack_delta_sizes_device", "md_pack_delta_sizes_host", "md_pack_choose_bases",
         "md_pack_search_last"]


def test_declared_exported_bound():
    build.build()
    for f in ("pack_search_kernels.hip", "capi_pack_search.cpp"):
        assert f in build.SOURCES and os.path.exists(os.path.join(build.CSRC, f)), f
    hdr = open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    so = ctypes.CDLL(_lib.SO)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert hasattr(so, f), f
        assert f in bound, f
    assert "} md_pack_search_stats;" in hdr and ctypes.sizeof(_lib.PackSearchStats) == 64
    assert [k for k, _ in _lib.PackSearchStats._fields_] == re.search(r"uint64_t (featured[^;]*);\s*} md_pack_search_stats", hdr).group(1).split(", ")
    assert "Out of scope: choosing bases" not in hdr and "searching for them (git's window) is out of scope" not in hdr
    # pack_search.hpp is plain C++ with no HIP in it, and its constants are the header's and the model's
    text = open(os.path.join(build.CSRC, "pack_search.hpp")).read()
    assert "#include <hip" not in text and "__device__" not in text and "ctx.hpp" not in text
    assert sm.SEEDS[0] == 0 and len(sm.SEEDS) == sm.FEATURES
    assert "kFeatures = %d" % sm.FEATURES in text and "kSeeds[kFeatures] = {0, %s}" % ", ".join("0x%08Xu" % s for s in sm.SEEDS[1:]) in text
    assert "kSegPositions = %d" % sm.SEG_POSITIONS in text and "kMaxWindow = 64" in text
    assert "S = {0, %s}" % ", ".join("0x%08X" % s for s in sm.SEEDS[1:]) in hdr and "0x9E3779B1" in hdr and "4 096 positions" in hdr
    # the kernels live in a file and a namespace of their own
    kernels = open(os.path.join(build.CSRC, "pack_search_kernels.hip")).read()
    assert "namespace pks" in kernels and "sketch_kernel" in kernels and "size_kernel" in kernels
    assert "sketch_kernel" not in open(os.path.join(build.CSRC, "pack_write_kernels.hip")).read()


def _sources(lens):
    src = (_lib.PackSource * max(len(lens), 1))()
    for s, n in zip(src, lens):
        s.off, s.len, s.base, s.type = 0, n, mp.NO_BASE, 3
    return src


def test_misuse_refused_without_device():
    lib = _lib.load()
    pair, src, out = (_lib.PackDeltaPair * 1)(), _sources([1]), _sources([1])
    one64, two64, one32 = (ctypes.c_uint64 * 1)(), (ctypes.c_uint64 * 1)(), (ctypes.c_int32 * 1)()
    feats, stats = (ctypes.c_uint32 * 4)(), _lib.PackSearchStats()
    assert lib.md_pack_sketch_host(None, 1, one64, two64, b"x", 1, feats) == -1
    assert lib.md_pack_sketch_host(None, 0, None, None, None, 0, None) == -1
    assert lib.md_pack_sketch_device(None, 1, one64, two64, None, None) == -1
    assert lib.md_pack_delta_sizes_host(None, 1, pair, b"x", 1, one64, one32) == -1
    assert lib.md_pack_delta_sizes_host(None, 0, None, None, 0, None, None) == -1
    assert lib.md_pack_delta_sizes_device(None, 1, pair, None, None, None) == -1
    assert lib.md_pack_choose_bases(None, 4, 50, 1, src, b"x", 1, out, one64) == -1
    assert lib.md_pack_choose_bases(None, 4, 50, 0, None, None, 0, None, None) == -1
    assert lib.md_pack_search_last(None, ctypes.byref(stats)) == -1
