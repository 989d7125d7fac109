"""CPU-side checks of the tree diff's entry points (md_pack_diff*): declared, exported and bound; md_tree_change
and md_pack_diff_info have the sizes and fields the header declares; the header's constants are pack_diff.hpp's, the model's
and the Python layer's; pack_diff.hpp has no HIP in it; misuse is refused without a device."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from decompress_amd import _lib, build
from decompress_amd import pack as mp
from tests import pack_diff_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["md_pack_diff", "md_pack_diff_get", "md_pack_diff_changes", "md_pack_diff_status", "md_pack_diff_free"]
OFFSETS = {"pair": 0, "parent": 4, "kind": 8, "flags": 9, "a_mode": 12, "b_mode": 16, "a_obj": 20, "b_obj": 24, "name_len": 28, "name_off": 32,
           "a_name": 40, "b_name": 60}


def test_declared_exported_bound():
    build.build()
    for f in ("pack_diff_kernels.hip", "capi_pack_diff.cpp"):
        assert f in build.SOURCES and os.path.exists(os.path.join(build.CSRC, f)), f
    hdr = open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    so = ctypes.CDLL(_lib.SO)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert hasattr(so, f), f
        assert f in bound, f
    assert "#define MD_TREE_NONE 0xffffffffu" in hdr and mp.TREE_NONE == 0xFFFFFFFF
    assert "#define MD_PACK_DIFF_RECURSIVE 1u" in hdr and mp.DIFF_RECURSIVE == 1
    assert "#define MD_TREE_CHANGE_TREE 1\n" in hdr and "#define MD_TREE_CHANGE_OPAQUE 2\n" in hdr
    assert (mp.CHANGE_TREE, mp.CHANGE_OPAQUE) == (dm.TREE, dm.OPAQUE) == (1, 2)
    assert ctypes.sizeof(_lib.TreeChange) == 80 and ctypes.sizeof(_lib.PackDiffInfo) == 72
    assert {k: getattr(_lib.TreeChange, k).offset for k, _ in _lib.TreeChange._fields_} == OFFSETS
    assert [k for k, _ in _lib.PackDiffInfo._fields_] == re.search(r"uint64_t (pairs, changes[^;]*);\s*} md_pack_diff_info", hdr).group(1).split(", ")
    assert mp._CHANGE_DTYPE.itemsize == 80 and {k: mp._CHANGE_DTYPE.fields[k][1] for k in mp._CHANGE_DTYPE.names} == OFFSETS
    assert list(mp._DIFF_INFO_KEYS) ==[k for k, _ in _lib.PackDiffInfo._fields_]
    # pack_diff.hpp is plain C++ with no HIP in it, and its constants are the header's
    text = open(os.path.join(build.CSRC, "pack_diff.hpp")).read()
    assert "#include <hip" not in text and "ctx.hpp" not in text and "internal.hpp" not in text
    assert "kNone = 0xffffffffu" in text and "kFlagTree = 1, kFlagOpaque = 2" in text
    kernels = open(os.path.join(build.CSRC, "pack_diff_kernels.hip")).read()
    assert "namespace pkd" in kernels and '#include "pack_diff.hpp"' in kernels and "find_key(" in kernels and "classify(" in kernels


def test_the_compilers_layout_of_a_record(tmp_path):
    """sizeof and offsetof as a C compiler sees the header, against the ctypes mirror"""
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    fields = list(OFFSETS)
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "mdeflate.h"\nint main(void) {\n  printf("%zu %zu", sizeof(md_tree_change), sizeof(md_pack_diff_info));\n' +
                   "".join('  printf(" %%zu", offsetof(md_tree_change, %s));\n' % f for f in fields) + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert got == [80, 72] + [OFFSETS[f] for f in fields]


def test_misuse_refused_without_device():
    lib = _lib.load()
    h, info = ctypes.c_void_p(), _lib.PackDiffInfo()
    one = (ctypes.c_uint32 * 1)(0)
    assert lib.md_pack_diff(None, None, None, b"x", 1, 1, one, one, 0, ctypes.byref(h)) == -1
    assert lib.md_pack_diff_get(None, ctypes.byref(info)) == -1
    assert lib.md_pack_diff_changes(None, None, 0, None, 0) == -1
    assert lib.md_pack_diff_status(None, None) == -1
    lib.md_pack_diff_free(None)
