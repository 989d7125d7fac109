"""The yardstick of md_pack_delta_batch_* and md_pack_write (tests/pack_delta_model.py) on the CPU: every case of
tests/pack_write_cases.py hits the edge it claims; every model delta applied by the pack reader's model (tests/pack_model.py)
gives the target; and, with git (skipped without), every model pack passes `git index-pack --strict`, git's idx is the
model's byte for byte, `git verify-pack -v` shows the model's depths and `git cat-file --batch` returns the contents."""
import os
import shutil
import subprocess

import pytest

from tests import pack_delta_model as dm
from tests import pack_model as pm
from tests import pack_write_cases as wc

GIT = shutil.which("git")
needs_git = pytest.mark.skipif(not GIT, reason="no git")
LEVEL = 6


def test_every_delta_claim_holds():
    cases = wc.delta_cases()
    assert set().union(*[c["edges"] for c in cases]) == wc.DELTA_EDGES
    assert len({c["name"] for c in cases}) == len(cases)
    for c in cases:
        traces, deltas = wc.delta_model(c)
        assert c["claim"](traces, deltas), c["name"]


def test_every_model_delta_applies():
    for c in wc.delta_cases():
        _, deltas = wc.delta_model(c)
        for (b, t), d in zip(c["pairs"], deltas):
            base, target = c["bufs"][b], c["bufs"][t]
            assert pm.Model._apply(None, {"size": len(target)}, d, base) == (pm.OK, target), c["name"]
            assert dm.apply_delta(base, d) == target, c["name"]


def test_the_layout_covers_every_alignment():
    blob, rows, who = wc.laid_out(wc.delta_cases())
    assert {r[0] % 16 for r in rows} == set(wc.ALIGNMENTS) == {r[2] % 16 for r in rows}
    cases = wc.delta_cases()
    for (bo, bl, to, tl), (ci, pi) in zip(rows, who):
        b, t = cases[ci]["pairs"][pi]
        assert blob[bo:bo + bl] == cases[ci]["bufs"][b] and blob[to:to + tl] == cases[ci]["bufs"][t]


def test_every_pack_claim_holds():
    cases = wc.pack_cases()
    assert set().union(*[c["edges"] for c in cases]) == wc.PACK_EDGES
    for c in cases:
        assert c["claim"](wc.pack_model(c["name"], LEVEL)), c["name"]


def test_version_chains_keep_their_deltas():
    with_deltas, without = wc.pack_model("version chains", LEVEL)
    last = with_deltas["last"]
    assert last["pairs"] == 280 and last["kept"] >= 0.9 * 280
    assert len(with_deltas["pack"]) < len(without["pack"]) / 2
    assert without["last"]["pairs"] == 0 and without["last"]["payload_after"] == without["last"]["payload_before"]


def test_model_packs_read_back_by_the_reader_model():
    for c in wc.pack_cases():
        for r in wc.pack_model(c["name"], LEVEL):
            if r["idx"] is None:
                continue
            m = pm.Model(r["pack"], r["idx"])
            assert m.rc == pm.OK, c["name"]
            where = {o["name"]: i for i, o in enumerate(m.objects)}
            got = m.read(verify=True)
            for (t, data), e, depth in zip(c["objects"], r["entries"], r["depth"]):
                o = m.objects[where[e["name"]]]
                assert (o["status"], o["type"], o["depth"], o["offset"]) == (pm.OK, t, depth, e["offset"]), c["name"]
                assert got[where[e["name"]]] == (pm.OK, data), c["name"]


def _git(d, *args, stdin=None):
    env = dict(os.environ, GIT_CONFIG_NOSYSTEM="1", HOME=str(d))
    return subprocess.run([GIT, *args], capture_output=True, env=env, cwd=str(d), input=stdin)


@needs_git
def test_git_accepts_every_model_pack(tmp_path):
    k = 0
    for c in wc.pack_cases():
        for r in wc.pack_model(c["name"], LEVEL):
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
            if r["idx"] is None:
                continue
            assert (store / (name + ".idx")).read_bytes() == r["idx"], c["name"]
            if not c["objects"]:
                continue
            v = _git(d / "repo", "verify-pack", "-v", str(store / (name + ".idx")))
            assert v.returncode == 0, (c["name"], v.stderr)
            depths = {}
            for line in v.stdout.decode().splitlines():
                f = line.split()
                if len(f) >= 5 and len(f[0]) == 40 and f[1] in ("commit", "tree", "blob", "tag"):
                    depths[f[0]] = int(f[5]) if len(f) >= 7 else 0
            assert [depths[e["name"].hex()] for e in r["entries"]] == r["depth"], c["name"]
            if all(t == 3 for t, _ in c["objects"]):  # (cat-file checks nothing about a commit's form, but keep to blobs)
                ask = b"".join(e["name"].hex().encode() + b"\n" for e in r["entries"])
                got = _git(d / "repo", "cat-file", "--batch", stdin=ask)
                assert got.returncode == 0
                want = b"".join(e["name"].hex().encode() + b" blob %d\n" % len(data) + data + b"\n" for e, (_, data) in zip(r["entries"], c["objects"]))
                assert got.stdout == want, c["name"]
