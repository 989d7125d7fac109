"""csrc/pack_graph.hpp - the rules by which a tree, a commit and a tag name other objects, the very functions the link
kernels run - under AddressSanitizer and UBSan, as a stand-alone host program (pack_graph_check.cpp, nothing preloaded, no
device), against the model's reading (tests/pack_graph_model.py) of the same bytes: every commit, tree and tag of
tests/pack_graph_cases.py and a few hundred seeded mutations of them."""
import os
import random
import shutil
import subprocess

import pytest

from tests import pack_graph_cases as gc
from tests import pack_graph_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _want(type_, data):
    parsed = gm.PARSERS[type_](data)
    if parsed is None:
        return "bad"
    return "%d" % len(parsed) + "".join(" %d:%s" % (k, nm.hex()) + (":%d" % w if type_ == gm.TAG else "") for k, nm, w in parsed)


def _objects():
    """[(type, bytes)]: the cases' own and mutations of them"""
    out = []
    for c in gc.cases():
        for lay in gc.build(c)["layout"]:
            if lay["type"] in gm.PARSERS and len(lay["data"]) <= 40000:
                out.append((lay["type"], lay["data"]))
    seen, own = set(), []
    for o in out:
        if o not in seen:
            seen.add(o)
            own.append(o)
    rng = random.Random(7)
    mutated = []
    for _ in range(600):
        t, data = rng.choice(own)
        b = bytearray(data)
        what = rng.randrange(5)
        if what == 0 and b:
            b[rng.randrange(len(b))] = rng.choice((0, 0x20, 0x0a, 0x30, 0x37, 0x38, 0x67, 0xff))
        elif what == 1:
            b = b[:rng.randrange(len(b) + 1)]
        elif what == 2 and b:
            at = rng.randrange(len(b))
            del b[at:at + rng.choice((1, 2, 20, 21))]
        elif what == 3:
            at = rng.randrange(len(b) + 1)
            b[at:at] = rng.choice((b"\0", b" ", b"\n", b"parent ", b"100644 x\0", bytes(21)))
        else:
            b += bytes(rng.choice((1, 20, 21, 22, 23)))
        mutated.append((t, bytes(b)))
    return own + mutated


def test_parse_rules_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "pack_graph_check"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "decompress_amd", "csrc"), os.path.join(ROOT, "tests", "pack_graph_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler cannot link the sanitizers")
    assert r.returncode == 0, r.stderr
    objects = _objects()
    path = tmp_path / "objects.txt"
    path.write_text("".join("%d %s\n" % (t, data.hex() or "-") for t, data in objects))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = r.stdout.splitlines()
    assert len(got) == len(objects) > 800
    bad = 0
    for (t, data), g in zip(objects, got):
        assert g == _want(t, data), (t, data[:200])
        bad += g == "bad"
    assert 100 < bad < len(objects) - 300
