"""CPU-side checks of the object graph's entry points (md_pack_graph_*, md_pack_reachable, md_pack_reach_last):
declared, exported and bound; the structs have the sizes and fields the header declares; the header's constants are
pack_graph.hpp's, the model's and the Python layer's; pack_graph.hpp has no HIP in it; the lookup is shared with the header
kernel; misuse is refused without a device."""
import ctypes
import os
import re

from decompress_amd import _lib, build
from decompress_amd import pack as mp
from tests import pack_graph_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["md_pack_graph_build", "md_pack_graph_get", "md_pack_graph_edges", "md_pack_graph_status", "md_pack_reachable", "md_pack_reach_last",
         "md_pack_graph_free"]


def test_declared_exported_bound():
    build.build()
    for f in ("pack_graph_kernels.hip", "capi_pack_graph.cpp"):
        assert f in build.SOURCES and os.path.exists(os.path.join(build.CSRC, f)), f
    hdr = open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    so = ctypes.CDLL(_lib.SO)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert hasattr(so, f), f
        assert f in bound, f
    assert "MD_INVALID_OBJECT = 27" in hdr and mp.INVALID_OBJECT == gm.INVALID_OBJECT == 27
    assert mp._status_name(27) == "Invalid object" and '"Invalid object"' in hdr
    assert "#define MD_PACK_NO_LINK 0xffffffffu" in hdr and mp.NO_LINK == gm.NO_LINK == 0xFFFFFFFF
    for k, name in enumerate(("COMMIT_TREE", "COMMIT_PARENT", "TAG_TARGET", "TREE_BLOB", "TREE_TREE", "TREE_GITLINK"), 1):
        assert "#define MD_PACK_EDGE_%s %d\n" % (name, k) in hdr and getattr(mp, name) == getattr(gm, name) == k
    assert "#define MD_PACK_EDGE_ABSENT 0x40" in hdr and "#define MD_PACK_EDGE_MISTYPED 0x80" in hdr
    assert (mp.EDGE_ABSENT, mp.EDGE_MISTYPED) == (gm.ABSENT, gm.MISTYPED) == (0x40, 0x80)
    assert ctypes.sizeof(_lib.PackGraphInfo) == 80 and ctypes.sizeof(_lib.PackReachStats) == 48
    assert [k for k, _ in _lib.PackGraphInfo._fields_] == re.search(r"uint64_t (n, edges[^;]*);\s*} md_pack_graph_info", hdr).group(1).split(", ")
    assert [k for k, _ in _lib.PackReachStats._fields_] == re.search(r"uint64_t (host_closed[^;]*);\s*} md_pack_reach_stats", hdr).group(1).split(", ")
    # pack_graph.hpp is plain C++ with no HIP in it, and its constants are the header's
    text = open(os.path.join(build.CSRC, "pack_graph.hpp")).read()
    assert "#include <hip" not in text and "ctx.hpp" not in text and "internal.hpp" not in text
    assert "kNoLink = 0xffffffffu" in text and "kAbsent = 0x40, kMistyped = 0x80" in text
    assert "kCommitTree = 1, kCommitParent = 2, kTagTarget = 3, kTreeBlob = 4, kTreeTree = 5, kTreeGitlink = 6" in text
    # the kernels live in a file and a namespace of their own and share the name lookup with the header kernel
    kernels = open(os.path.join(build.CSRC, "pack_graph_kernels.hip")).read()
    assert "namespace pkg" in kernels and "find_name(" in kernels and '#include "pack_graph.hpp"' in kernels
    assert "find_name(" in open(os.path.join(build.CSRC, "pack_kernels.hip")).read()


def test_misuse_refused_without_device():
    lib = _lib.load()
    h, info, stats = ctypes.c_void_p(), _lib.PackGraphInfo(), _lib.PackReachStats()
    one64, count, mark = (ctypes.c_uint64 * 1)(), ctypes.c_uint64(0), (ctypes.c_uint8 * 1)()
    assert lib.md_pack_graph_build(None, None, b"x", 1, 0, ctypes.byref(h)) == -1
    assert lib.md_pack_graph_get(None, ctypes.byref(info)) == -1
    assert lib.md_pack_graph_edges(None, None, None, None, 0) == -1
    assert lib.md_pack_graph_status(None, None) == -1
    assert lib.md_pack_reachable(None, None, one64, 1, None, 0, mark, ctypes.byref(count)) == -1
    assert lib.md_pack_reach_last(None, ctypes.byref(stats)) == -1
    lib.md_pack_graph_free(None)
