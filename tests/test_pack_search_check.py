"""csrc/pack_search.hpp - positions and segments, the pack order, the candidates from the groups of equal (type, feature), the
choice - under AddressSanitizer and UBSan, as a stand-alone host program (pack_search_check.cpp, nothing preloaded, no
device), against the model's numbers (tests/pack_search_model.py) for the same inputs: every case of
tests/pack_search_cases.py with the model's features and scores, and made-up batches whose few feature values, types and
lengths collide all the time."""
import os
import random
import shutil
import subprocess

import pytest

from tests import pack_delta_model as dm
from tests import pack_search_cases as sc
from tests import pack_search_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _objects_text(kinds, lens, feats):
    return "%d %s" % (len(lens), " ".join("%d %d %d %d %d %d" % ((t, n) + tuple(f)) for t, n, f in zip(kinds, lens, feats)))


def _want_pairs(order, pairs):
    return " ".join(map(str, order)) + " |" + "".join(" %d:%d" % p for p in pairs)


def _want_choice(bases, depth):
    return "%d" % sum(b is not None for b in bases) + "".join(" %d:%d" % (-1 if b is None else b, d) for b, d in zip(bases, depth))


def _lines():
    """[(line, expected output)]"""
    out = []
    for n in (0, 1, 15, 16, 17, 78, 79, 80, 4110, 4111, 4112, 8207, 8208, 0xFFFFFFF0):
        npos = max(n - 15, 0)
        out.append(("G %d" % n, "%d %d" % (npos, -(-npos // sm.SEG_POSITIONS))))
    for c in sc.search_cases():
        kinds, lens = [t for t, _ in c["objects"]], [len(d) for _, d in c["objects"]]
        for t, max_depth in zip(sc.search_model(c["name"]), c["runs"]):
            objs = _objects_text(kinds, lens, t["features"])
            out.append(("C %d %s" % (c["window"], objs), _want_pairs(t["order"], t["pairs"])))
            scores = " ".join("%d %d" % (st == dm.MD_OK, n) for st, n in t["scores"])
            out.append(("S %d %d %s %d %s" % (c["window"], max_depth, objs, len(t["pairs"]), scores), _want_choice(t["bases"], t["depth"])))
    rng = random.Random(11)
    for _ in range(150):
        n = rng.randrange(0, 40)
        window = rng.choice((1, 2, 3, 4, 64))
        kinds = [rng.choice((1, 2, 3, 3, 3, 4)) for _ in range(n)]
        lens = [rng.choice((0, 15, 16, 63, 64, 64, 100, 100, 5000)) for _ in range(n)]
        feats = [tuple(rng.choice((0, 1, 7, 0xFFFFFFFF)) for _ in range(4)) for _ in range(n)]
        objects = [(t, bytes(k)) for t, k in zip(kinds, lens)]  # (the model's order and candidates look at lengths alone)
        order = sm.pack_order(objects)
        cand = sm.candidates(objects, order, feats, window)
        given = {(r, b): (rng.choice((dm.MD_OK, dm.MD_OK, dm.MD_UNEXPECTED_END_OF_OUTPUT)), rng.choice((5, 5, 6, 9, 1 << 33))) for r in range(n) for b in cand[r]}
        given = {k: (st, v if st == dm.MD_OK else 0) for k, (st, v) in given.items()}
        max_depth = rng.choice((0, 1, 2, 3, 50))
        bases, depth, pairs, scores, _ = sm.choose(cand, lambda r, b: given[(r, b)], max_depth)
        assert all(lens[order[r]] >= 64 and lens[order[b]] >= 16 and kinds[order[r]] == kinds[order[b]] and b < r for r, b in pairs)
        objs = _objects_text(kinds, lens, feats)
        out.append(("C %d %s" % (window, objs), _want_pairs(order, pairs)))
        text = " ".join("%d %d" % (st == dm.MD_OK, v) for st, v in scores)
        out.append(("S %d %d %s %d %s" % (window, max_depth, objs, len(pairs), text), _want_choice(bases, depth)))
    return out


def test_host_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "pack_search_check"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "decompress_amd", "csrc"), os.path.join(ROOT, "tests", "pack_search_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler cannot link the sanitizers")
    assert r.returncode == 0, r.stderr
    lines = _lines()
    path = tmp_path / "cases.txt"
    path.write_text("".join(line + "\n" for line, _ in lines))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = r.stdout.splitlines()
    assert len(got) == len(lines) > 300
    for (line, want), g in zip(lines, got):
        assert g == want, line[:200]
