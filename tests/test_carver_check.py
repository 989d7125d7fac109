"""md::Carver (csrc/host_util.hpp) under AddressSanitizer and UBSan, as a stand-alone host program (carver_check.cpp,
nothing preloaded, no device).  Every list of (element size, count) is carved twice, once for the size and once over a heap
block of exactly that size, and every element of every array is written: arrays start on 16 bytes, do not overlap, the two
passes agree, and no write leaves the block.  The block's size is also worked out here, on its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = (1, 2, 4, 8, 48)
COUNTS = (0, 1, 15, 16, 17, 4099)


def _lists():
    lists = [[(e, n)] for e in SIZES for n in COUNTS]                       # one array
    lists += [[(e, n) for e in SIZES] for n in COUNTS]                      # every element size, one count (n = 0: all zero)
    lists += [[(e, n) for n in COUNTS] for e in SIZES]                      # one element size, every count
    lists += [[(8, 17), (4, 17), (1, 17), (48, 3), (2, 0)]]                 # ends in a zero-length take
    lists += [[(1, 0), (8, 1), (1, 0), (4, 15), (1, 0)]]                    # zero-length takes between others
    lists += [[(8, 3000)] * 8 + [(4, 3000)] * 7 + [(1, 3000)]]              # a round of the long-stream decoder
    lists += [[(48, 5), (8, 5), (8, 6), (8, 6)] + [(8, 5)] * 6 + [(8, 1), (4, 5), (4, 5), (4, 9), (4, 9), (1, 5), (1, 33)]]  # a ZIP read
    return lists


def _size(lst):
    return sum((e * n + 15) // 16 * 16 for e, n in lst)


def test_carver_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "carver_check"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "decompress_amd", "csrc"), os.path.join(ROOT, "tests", "carver_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler cannot link the sanitizers")
    assert r.returncode == 0, r.stderr
    lists = _lists()
    assert any(all(n == 0 for _, n in lst) and len(lst) > 1 for lst in lists)
    assert any(lst[-1][1] == 0 and lst[0][1] != 0 for lst in lists)
    path = tmp_path / "lists.txt"
    with open(path, "w") as f:
        for lst in lists:
            f.write(" ".join("%d %d" % p for p in lst) + "\n")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    got = [int(x) for x in r.stdout.split()]
    assert got == [_size(lst) for lst in lists]
