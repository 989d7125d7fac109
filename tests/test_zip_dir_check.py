"""csrc/zip_dir.hpp under AddressSanitizer and UBSan, as a stand-alone host program (zip_dir_check.cpp, nothing preloaded,
no device): a good archive cut at every length and every single-byte change of the last 400 bytes of three archives.  The
program must end clean, and say of every case what md_zip_directory says through ctypes."""
import ctypes
import os
import shutil
import subprocess

import pytest

from decompress_amd import _lib, build
from tests import zip_util as zu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAIL = 400


def _archives():
    small = [("a", b"hello hello hello hello"), ("b/", b""), ("c.bin", bytes(range(40)))]
    ents = lambda **kw: [zu.entry(n, d, method=8 if d else 0, **kw) for n, d in small]
    return [zu.archive(ents(), comment=b"tail")[0],
            zu.archive(ents(zip64_dir=True), zip64_end=True)[0],
            zu.archive(ents(descriptor="sig", dir_extra=zu.extra_field(0x5455, b"\1abcd")), prefix=b"stub" * 5, zip64_end=True, comment=b"PK")[0]]


def _cases():
    bases = _archives()
    cases = [(0, "T", n, 0) for n in range(len(bases[0]) + 1)]
    for b, blob in enumerate(bases):
        for pos in range(max(0, len(blob) - TAIL), len(blob)):
            cases += [(b, "M", pos, v) for v in range(256) if v != blob[pos]]
    return bases, cases


def _status(lib, blob):
    info = _lib.ZipInfo()
    st = lib.md_zip_directory(blob, len(blob), ctypes.byref(info), None, 0)
    if st == 0:
        ents = (_lib.ZipEntry * max(info.entries, 1))()
        assert lib.md_zip_directory(blob, len(blob), ctypes.byref(info), ents, info.entries) == 0
    return st


def test_directory_parser_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "zip_dir_check"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "decompress_amd", "csrc"), os.path.join(ROOT, "tests", "zip_dir_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler cannot link the sanitizers")
    assert r.returncode == 0, r.stderr
    bases, cases = _cases()
    assert len(cases) > 3 * TAIL * 255 * 0.9
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for b in bases:
            f.write("B %s\n" % b.hex())
        for b, kind, a, v in cases:
            f.write("%s %d %d %d\n" % (kind, b, a, v) if kind == "M" else "T %d %d\n" % (b, a))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = [int(x) for x in r.stdout.split()]
    assert len(got) == len(cases)
    build.build()
    lib = _lib.load()
    ok = bad = 0
    for (b, kind, a, v), st in zip(cases, got):
        blob = bases[b][:a] if kind == "T" else bases[b][:a] + bytes([v]) + bases[b][a + 1:]
        assert _status(lib, blob) == st, (b, kind, a, v, st)
        assert st in (0, 18)
        ok += st == 0
        bad += st == 18
    assert ok > 1000 and bad > 1000  # (both answers occur: the cases reach the parser's checks, and pass some)
