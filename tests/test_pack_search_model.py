"""The yardstick of md_pack_sketch_* and md_pack_choose_bases (tests/pack_search_model.py) on the CPU: every case of
tests/pack_search_cases.py hits the edge it claims; the vectorised sketch is the definition taken one window at a time; the
searched packs read back through the reader's model; the shuffled version chains find every base within their own chain
and pack within 1.1 x of the pack with the true predecessors; and, with git (skipped without), every searched model pack
passes `git index-pack --strict`, `git verify-pack -v` shows the model's depths and `git cat-file --batch` returns the
contents."""
import os
import shutil
import subprocess

import pytest

from tests import pack_delta_model as dm
from tests import pack_model as pm
from tests import pack_search_cases as sc
from tests import pack_search_model as sm
from tests import pack_write_cases as wc

GIT = shutil.which("git")
needs_git = pytest.mark.skipif(not GIT, reason="no git")
LEVEL = 6


def test_every_sketch_claim_holds():
    cases = sc.sketch_cases()
    assert set().union(*[c["edges"] for c in cases]) == sc.SKETCH_EDGES
    assert len({c["name"] for c in cases}) == len(cases)
    for c, (f, p) in zip(cases, sc.sketch_model()):
        assert c["claim"](f, p), c["name"]
    assert len(next(c for c in cases if c["name"] == "64 positions")["data"]) == 79


def test_the_sketch_is_the_definition_window_by_window():
    for c in sc.sketch_cases():
        data = c["data"]
        if len(data) > 400:
            continue
        want = [min((sm.feature_value(data[p:p + 16], i), p) for p in range(len(data) - 15)) for i in range(4)] if len(data) >= 16 else None
        f, p = sm.sketch(data)
        assert (f, p) == ((tuple(w[0] for w in want), tuple(w[1] for w in want)) if want else (sm.NONE, None)), c["name"]
    assert sm.SEEDS[0] == 0 and sm.feature_value(sm.planted(0, 1), 0) == 0 and dm.block_hash(sm.planted(0, 1)) == 0


def test_the_layout_covers_every_alignment_and_the_last_byte():
    datas = [c["data"] for c in sc.sketch_cases()]
    blob, at = sc.laid_out(datas)
    assert {o % 16 for (o, n) in at if n >= 16} == set(sc.ALIGNMENTS)
    assert at[-1][0] + at[-1][1] == len(blob) and at[-1][1] > sm.SEG_POSITIONS
    for (o, n), d in zip(at, datas):
        assert blob[o:o + n] == d


def test_every_search_claim_holds():
    cases = sc.search_cases()
    assert set().union(*[c["edges"] for c in cases]) == sc.SEARCH_EDGES
    assert len({c["name"] for c in cases}) == len(cases)
    for c in cases:
        traces = sc.search_model(c["name"])
        assert c["claim"](traces), c["name"]
        for t in traces:  # what holds for every search
            n = len(c["objects"])
            assert sorted(t["order"]) == list(range(n)) and len(t["pairs"]) == len(set(t["pairs"])) <= n * 4 * c["window"]
            assert all(b is None or b < r for r, b in enumerate(t["bases"]))
            assert t["last"]["chosen"] <= t["last"]["fitted"] <= t["last"]["pairs"]


def test_md_pack_write_keeps_every_chosen_delta():
    for c in sc.search_cases():
        for t, r, max_depth in zip(sc.search_model(c["name"]), sc.pack_model(c["name"], LEVEL), c["runs"]):
            assert r["keep"] == [b is not None for b in t["bases"]] and r["depth"] == t["depth"], c["name"]
            assert r["last"]["dropped_size"] == r["last"]["dropped_depth"] == 0 and r["last"]["kept"] == t["last"]["chosen"], c["name"]
            assert max_depth == 0 or max(t["depth"] or [0]) <= max_depth


def test_shuffled_version_chains():
    """280 bases, each from the target's own chain, and a pack at most 1.1 x the pack with the true predecessors"""
    objs, chain = sc.shuffled_chains()
    t = sc.search_model("shuffled version chains")[0]
    assert t["last"]["chosen"] == 280 and t["last"]["featured"] == 320
    for r, b in enumerate(t["bases"]):
        assert b is None or chain[t["order"][r]] == chain[t["order"][b]]
    searched = sc.pack_model("shuffled version chains", LEVEL)[0]["pack"]
    true = wc.pack_model("version chains", LEVEL)[0]["pack"]
    print("shuffled version chains: pairs %d, searched pack %d bytes, true predecessors %d bytes, ratio %.4f"
          % (t["last"]["pairs"], len(searched), len(true), len(searched) / len(true)))
    assert len(searched) <= 1.1 * len(true)


def test_searched_packs_read_back_by_the_reader_model():
    for c in sc.search_cases():
        for t, r in zip(sc.search_model(c["name"]), sc.pack_model(c["name"], LEVEL)):
            if r["idx"] is None:
                continue
            m = pm.Model(r["pack"], r["idx"])
            assert m.rc == pm.OK, c["name"]
            where = {o["name"]: i for i, o in enumerate(m.objects)}
            got = m.read(verify=True)
            for rank, e in enumerate(r["entries"]):
                typ, data = c["objects"][t["order"][rank]]
                o = m.objects[where[e["name"]]]
                assert (o["status"], o["type"], o["depth"]) == (pm.OK, typ, t["depth"][rank]), c["name"]
                assert got[where[e["name"]]] == (pm.OK, data), c["name"]


def _git(d, *args, stdin=None):
    env = dict(os.environ, GIT_CONFIG_NOSYSTEM="1", HOME=str(d))
    return subprocess.run([GIT, *args], capture_output=True, env=env, cwd=str(d), input=stdin)


@needs_git
def test_git_accepts_every_searched_pack(tmp_path):
    k = 0
    for c in sc.search_cases():
        for t, r in zip(sc.search_model(c["name"]), sc.pack_model(c["name"], LEVEL)):
            d = tmp_path / ("p%d" % k)
            k += 1
            d.mkdir()
            assert _git(d, "init", "-q", "repo").returncode == 0
            store = d / "repo" / ".git" / "objects" / "pack"
            name = "pack-" + r["pack"][-20:].hex()
            (store / (name + ".pack")).write_bytes(r["pack"])
            strict = ["--strict"] if r["idx"] is not None else []  # (two objects with one name: --strict refuses, as md_pack_index_write does)
            g = _git(d / "repo", "index-pack", *strict, "-o", str(store / (name + ".idx")), str(store / (name + ".pack")))
            assert g.returncode == 0, (c["name"], g.stderr)
            if r["idx"] is None or not c["objects"]:
                continue
            assert (store / (name + ".idx")).read_bytes() == r["idx"], c["name"]
            v = _git(d / "repo", "verify-pack", "-v", str(store / (name + ".idx")))
            assert v.returncode == 0, (c["name"], v.stderr)
            depths = {}
            for line in v.stdout.decode().splitlines():
                f = line.split()
                if len(f) >= 5 and len(f[0]) == 40 and f[1] in ("commit", "tree", "blob", "tag"):
                    depths[f[0]] = int(f[5]) if len(f) >= 7 else 0
            assert [depths[e["name"].hex()] for e in r["entries"]] == t["depth"], c["name"]
            if all(typ == 3 for typ, _ in c["objects"]):
                contents = [c["objects"][i][1] for i in t["order"]]
                ask = b"".join(e["name"].hex().encode() + b"\n" for e in r["entries"])
                got = _git(d / "repo", "cat-file", "--batch", stdin=ask)
                assert got.returncode == 0
                want = b"".join(e["name"].hex().encode() + b" blob %d\n" % len(data) + data + b"\n" for e, data in zip(r["entries"], contents))
                assert got.stdout == want, c["name"]
