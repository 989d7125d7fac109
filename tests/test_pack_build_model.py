"""The yardstick of md_pack_index_build, checked against git itself (needs git, skipped without): for every well-formed case of
tests/pack_build_cases.py the idx of the model (tests/pack_build_model.py), the idx pack_writer wrote and the idx `git
index-pack` writes are the same bytes; every malformed case is refused by git, with at most one exception that the list
below names and `git index-pack --strict` refuses; every edge of the issue's list is in the cases, and where a case
carries a claim about its bytes the claim holds."""
import os
import shutil
import subprocess

import pytest

from tests import pack_build_cases as bc
from tests import pack_build_model as bm
from tests import pack_model as pm

GIT = shutil.which("git")
needs_git = pytest.mark.skipif(not GIT, reason="no git")
# what git index-pack accepts and the builder refuses: at most one entry
GIT_ACCEPTS = ["the same object twice"]


def _index_pack(tmp_path, k, pack, *more):
    """-> (returncode, idx bytes or None)"""
    d = tmp_path / ("p%d" % k)
    d.mkdir()
    path = d / "x.pack"
    path.write_bytes(pack)
    env = dict(os.environ, GIT_CONFIG_NOSYSTEM="1", HOME=str(d))
    r = subprocess.run([GIT, "index-pack", *more, "-o", str(d / "x.idx"), str(path)], capture_output=True, env=env, cwd=str(d))
    idx = (d / "x.idx").read_bytes() if r.returncode == 0 and (d / "x.idx").exists() else None
    return r.returncode, idx


def test_the_cases_hold_every_edge_and_every_claim():
    cases = bc.cases()
    assert set().union(*[c["edges"] for c in cases]) == bc.REQUIRED_EDGES
    from tests import pack_cases as pc
    assert {c["name"] for c in pc.cases()} <= {c["name"] for c in cases}
    for c in cases:
        if c["claim"]:
            assert c["claim"](c), c["name"]
    assert len(GIT_ACCEPTS) <= 1 and sum(c["ours"] for c in cases) == 1


def test_model_agrees_with_the_writer():
    for c in bc.cases():
        m = bc.model(c["name"])
        assert (m.rc == pm.OK) == bc.accepted(c), c["name"]
        if c["idx"] is not None:
            assert m.idx == c["idx"], c["name"]
        if m.rc == pm.OK:
            assert len(m.idx) == 8 + 1024 + 28 * m.n + 40 and m.status == [pm.OK] * m.n, c["name"]
        else:
            assert m.idx == b"", c["name"]
    assert bc.model("a fan of 1000").generations == 2
    assert bc.model("copy lengths").generations == 1  # no REF_DELTA: one generation
    assert bc.model("an empty pack").idx == bc.model("an empty pack, built").idx and len(bc.model("an empty pack").idx) == 1072
    # the two-byte test passes for 132 of the 65 536 pairs of bytes: one position in 496 of random bytes
    assert len(bm._PAIRS) == 132 and (0x78, 0x9c) in bm._PAIRS and (0x78, 0x9d) not in bm._PAIRS and (0x79, 0x9c) not in bm._PAIRS


@needs_git
def test_well_formed_cases_get_gits_idx(tmp_path):
    for k, c in enumerate(bc.cases()):
        if not c["well"]:
            continue
        rc, idx = _index_pack(tmp_path, k, c["pack"])
        assert rc == 0, c["name"]
        assert idx == bc.model(c["name"]).idx, c["name"]
        if c["idx"] is not None:
            assert idx == c["idx"], c["name"]


@needs_git
def test_malformed_cases_are_refused_by_git(tmp_path):
    accepted = []
    for k, c in enumerate(bc.cases()):
        if c["well"]:
            continue
        rc, _ = _index_pack(tmp_path, k, c["pack"])
        if rc == 0:
            accepted.append(c["name"])
    assert accepted == GIT_ACCEPTS
    by_name = {c["name"]: c for c in bc.cases()}
    for k, name in enumerate(GIT_ACCEPTS):  # the builder is as strict as --strict here
        rc, _ = _index_pack(tmp_path, 1000 + k, by_name[name]["pack"], "--strict")
        assert rc != 0, name
        assert bc.model(name).rc == pm.INVALID_PACK
