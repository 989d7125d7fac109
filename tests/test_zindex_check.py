"""csrc/zindex.hpp under AddressSanitizer and UBSan, as a stand-alone host program (zindex_check.cpp, nothing preloaded, no
device): a good blob of 3 points cut at every length and every single-byte change of its head and point table.  The
program must end clean, and say of every case what md_inflate_index_load says through ctypes."""
import ctypes
import os
import shutil
import subprocess

import pytest

from decompress_amd import _lib, build
from tests import zindex_blob as zb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    base = zb.blob()
    cases = [("T", n, 0) for n in range(len(base) + 1)]
    for pos in range(zb.HEAD + 3 * zb.POINT):
        cases += [("M", pos, v) for v in range(256) if v != base[pos]]
    return base, cases


def _status(lib, blob):
    h = ctypes.c_void_p()
    st = lib.md_inflate_index_load(blob, len(blob), ctypes.byref(h))
    lib.md_inflate_index_free(h)
    return st


def test_index_loader_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "zindex_check"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "decompress_amd", "csrc"), os.path.join(ROOT, "tests", "zindex_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler cannot link the sanitizers")
    assert r.returncode == 0, r.stderr
    base, cases = _cases()
    assert len(cases) == len(base) + 1 + (zb.HEAD + 3 * zb.POINT) * 255
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        f.write("B %s\n" % base.hex())
        for kind, a, v in cases:
            f.write("M 0 %d %d\n" % (a, v) if kind == "M" else "T 0 %d\n" % a)
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = [int(x) for x in r.stdout.split()]
    assert len(got) == len(cases)
    build.build()
    lib = _lib.load()
    ok = bad = 0
    for (kind, a, v), st in zip(cases, got):
        blob = base[:a] if kind == "T" else base[:a] + bytes([v]) + base[a + 1:]
        assert _status(lib, blob) == st, (kind, a, v, st)
        assert st in (0, 21)
        ok += st == 0
        bad += st == 21
    assert ok > 100 and bad > 100  # (both answers occur: the cases reach the loader's checks, and pass some)
