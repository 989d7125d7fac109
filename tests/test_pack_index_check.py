"""csrc/pack_index.hpp under AddressSanitizer and UBSan, as a stand-alone host program (pack_index_check.cpp, nothing
preloaded, no device): every idx of the index family, one valid idx cut at every length, and single-byte changes of its
header, of parts of its fan-out and of its offsets.  The program must end clean, and say of every case what the model of
tests/pack_model.py says."""
import os
import shutil
import subprocess

import pytest

from tests import pack_cases as pc
from tests import pack_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cases():
    family, _, _ = pc.index_cases()
    bases = [blob for _, blob, _ in family]
    cases = [(b, "T", len(blob), 0) for b, blob in enumerate(bases)]  # each as it is
    good, big = bases[0], bases[1]
    cases += [(0, "T", n, 0) for n in range(len(good))]
    n = pm.read_idx(good)[2]["n"]
    spots = list(range(8)) + list(range(8 + 4 * 250, 8 + 1024)) + list(range(1032 + 24 * n, 1032 + 24 * n + 16))
    for b, blob in ((0, good), (1, big)):
        cases += [(b, "M", pos, v) for pos in spots for v in (0, 1, 0x7f, 0x80, 0xff) if v != blob[pos]]
    return bases, cases


def test_index_reader_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "pack_index_check"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "decompress_amd", "csrc"), os.path.join(ROOT, "tests", "pack_index_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler cannot link the sanitizers")
    assert r.returncode == 0, r.stderr
    bases, cases = _cases()
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for b in bases:
            f.write("B %s\n" % b.hex())
        for b, kind, a, v in cases:
            f.write("%s %d %d %d\n" % (kind, b, a, v) if kind == "M" else "T %d %d\n" % (b, a))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = [int(x) for x in r.stdout.split()]
    assert len(got) == len(cases) > 2000
    seen = set()
    for (b, kind, a, v), st in zip(cases, got):
        blob = bases[b][:a] if kind == "T" else bases[b][:a] + bytes([v]) + bases[b][a + 1:]
        assert pm.read_idx(blob)[0] == st, (b, kind, a, v, st)
        seen.add(st)
    assert seen == {pm.OK, pm.INVALID_INDEX, pm.UNSUPPORTED}
