"""csrc/pack_diff.hpp - the canonical mode, the key compare, the search by key and the classification, the very functions the
diff kernels run - under AddressSanitizer and UBSan, as a stand-alone host program (pack_diff_check.cpp, nothing preloaded,
no device), against the model's reading (tests/pack_diff_model.py) of the same bytes: every pair of trees of
tests/pack_diff_cases.py, every sub-pair below them, and a few hundred seeded mutations."""
import os
import random
import shutil
import subprocess

import pytest

from tests import pack_diff_cases as dc
from tests import pack_diff_model as dm
from tests import pack_graph_model as gm
from tests import pack_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _want(a, b):
    ea, eb = dm.entries(a), dm.entries(b)
    if ea is None or eb is None or not dm.is_sorted(ea) or not dm.is_sorted(eb):
        return "bad"
    recs = dm.diff_entries(ea, eb)
    out = ""
    for kind, _, i, j in recs:
        out += " %s:%o:%o:%s" % (kind, ea[i][0] if i is not None else 0, eb[j][0] if j is not None else 0, (ea[i][1] if i is not None else eb[j][1]).hex())
    return "%d" % len(recs) + out


def _pairs():
    """[(A's bytes, B's bytes)]: the level-0 pairs of the cases, the sub-pairs the model descends into, and mutations of them"""
    own, seen = [], set()
    for c in dc.cases():
        if c["workspace"] is not None or c["commits"]:
            continue
        b = dc.build(c)
        g = gm.Graph(b["pack"], b["idx"])
        data = {i: d for i, (st, d) in enumerate(g.model.read()) if st == pm.OK and g.model.objects[i]["type"] == gm.TREE}
        d = dm.Diff(g, b["ipairs"])
        subs = [(r["a_obj"] if r["kind"] != "A" else None, r["b_obj"] if r["kind"] != "D" else None) for r in d.records if r["flags"] & dm.TREE]
        for x, y in list(b["ipairs"]) + subs:
            if all(t is None or t in data for t in (x, y)):
                pr = (data[x] if x is not None else b"", data[y] if y is not None else b"")
                if pr not in seen and len(pr[0]) + len(pr[1]) <= 40000:
                    seen.add(pr)
                    own.append(pr)
    rng = random.Random(11)
    mutated = []
    for _ in range(400):
        a, b = rng.choice(own)
        m = bytearray(b if b else a)
        what = rng.randrange(5)
        if what == 0 and m:
            m[rng.randrange(len(m))] = rng.choice((0, 0x20, 0x2f, 0x30, 0x31, 0x34, 0x37, 0x38, 0xff))
        elif what == 1:
            m = m[:rng.randrange(len(m) + 1)]
        elif what == 2 and m:
            at = rng.randrange(len(m))
            del m[at:at + rng.choice((1, 20, 21, 28))]
        elif what == 3:
            at = rng.randrange(len(m) + 1)
            m[at:at] = rng.choice((b"\0", b" ", b"/", b"100644 x\0" + bytes(20), b"40000 x\0" + bytes(20)))
        else:
            m += b"100755 zzzz\0" + bytes(range(20))
        mutated.append((a, bytes(m)) if rng.randrange(2) else (bytes(m), a))
    return own + mutated


def test_diff_rules_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "pack_diff_check"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "decompress_amd", "csrc"), os.path.join(ROOT, "tests", "pack_diff_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler cannot link the sanitizers")
    assert r.returncode == 0, r.stderr
    pairs = _pairs()
    path = tmp_path / "pairs.txt"
    path.write_text("".join("%s %s\n" % (a.hex() or "-", b.hex() or "-") for a, b in pairs))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = r.stdout.splitlines()
    assert len(got) == len(pairs) > 500
    bad = 0
    for (a, b), g in zip(pairs, got):
        assert g == _want(a, b), (a[:200], b[:200])
        bad += g == "bad"
    assert 50 < bad < len(pairs) - 300
