"""The yardstick of the names tests on the CPU: tests/pack_names_model.py reads every case of tests/pack_name_cases.py as the
case says, leaves every case of tests/pack_cases.py as it is without names (their names are right wherever an object
decodes), reads the pack git wrote (tests/golden/git_pack) as all Ok with the names of objects.json; and where git is on
the machine, `git verify-pack` refuses a pack with one wrong name and accepts the same pack with the right one.  No device."""
import json
import os
import shutil
import subprocess

import pytest

from tests import pack_cases as pc
from tests import pack_model as pm
from tests import pack_name_cases as pnc
from tests import pack_names_model as pnm
from tests import pack_writer as pw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "git_pack")
GIT = shutil.which("git")
ENV = dict(os.environ, GIT_CONFIG_GLOBAL="/dev/null", GIT_CONFIG_SYSTEM="/dev/null")


@pytest.fixture(scope="module")
def built():
    return [pc.build(c) for c in pnc.cases()]


def _by_entry(c, got):
    return {k: got[c["order"][k]][0] for k in range(len(c["layout"])) if got[c["order"][k]][0] != pm.OK}


def test_the_model_reads_every_name_case_as_the_case_says(built):
    assert len({c["name"] for c in built}) == len(built) >= 12
    for c in built:
        m = pm.Model(c["pack"], c["idx"])
        assert m.rc == pm.OK and m.info["failed"] == 0, c["name"]
        assert _by_entry(c, m.read()) == {}, c["name"]  # without the flag nothing is wrong
        assert _by_entry(c, m.read(None, True)) == c.get("verify", {}), c["name"]
        assert _by_entry(c, pnm.read(m)) == c["names"], c["name"]
        assert _by_entry(c, pnm.read(m, None, True)) == c.get("both", c["names"]), c["name"]
        for (st, data), plain in zip(pnm.read(m), m.read()):
            assert st != pm.OK or data == plain[1], c["name"]
        if "select" in c:
            sel = [c["order"][k] for k in c["select"]]
            assert [st for st, _ in pnm.read(m, sel)] == c["selected"], c["name"]


def test_the_cases_hold_their_edges(built):
    by_name = {c["name"]: c for c in built}
    c = by_name["message lengths around the block"]
    sizes = c["sizes"]
    lengths = [pnc.message_length(3, s) for s in sizes]
    assert {(n // 64, n % 64) for n in lengths} == {(b, r) for b in range(3) for r in pnc.EDGE_REMAINDERS} - {(0, 0), (0, 1)}
    whole = [x["data"] for x in c["layout"][:len(sizes)]]
    results = [x["data"] for x in c["layout"][len(sizes) + 1:]]
    assert [len(d) for d in whole] == sizes == [len(d) for d in results]  # each length once whole and once as a delta's result
    c = by_name["sizes where the header grows"]
    assert sorted({len(x["data"]) for x in c["layout"]} & {9, 10, 99, 100, 999, 1000}) == [9, 10, 99, 100, 999, 1000]
    c = by_name["a tree's bytes stored as a blob"]
    m = pm.Model(c["pack"], c["idx"])
    o = m.objects[c["order"][0]]
    assert o["type"] == 3 and o["name"] == pw.object_name(2, pnc.TREE) != pw.object_name(3, pnc.TREE)
    c = by_name["a name wrong in its last byte"]
    name, true = c["layout"][0]["name"], pw.object_name(3, pc.MID)
    assert name[:19] == true[:19] and name[19] != true[19]
    c = by_name["all four types, whole and as deltas"]
    m = pm.Model(c["pack"], c["idx"])
    assert sorted((o["type"], o["depth"]) for o in m.objects) == [(1, 0), (1, 1), (2, 0), (2, 1), (3, 0), (3, 1), (4, 0), (4, 0), (4, 1)]
    c = by_name["a wrong name in the middle of a chain"]
    m = pm.Model(c["pack"], c["idx"])
    assert [m.objects[c["order"][k]]["depth"] for k in range(5)] == [0, 1, 2, 3, 4]


def test_names_change_nothing_where_they_are_right():
    for case in pc.cases():
        c = pc.build(case)
        m = pm.Model(c["pack"], c["idx"])
        if m.rc != pm.OK:
            continue
        for verify in (False, True):
            assert [st for st, _ in pnm.read(m, None, verify)] == [st for st, _ in m.read(None, verify)], (c["name"], verify)


def test_the_pack_git_wrote():
    with open(os.path.join(GOLDEN, "git.pack"), "rb") as f:
        pack = f.read()
    with open(os.path.join(GOLDEN, "git.idx"), "rb") as f:
        idx = f.read()
    with open(os.path.join(GOLDEN, "objects.json")) as f:
        table = json.load(f)
    m = pm.Model(pack, idx)
    got = pnm.read(m, None, True)
    assert len(got) == len(table) == 31
    for o, (st, data) in zip(m.objects, got):
        assert st == pm.OK and pnm.object_name(o["type"], data) == o["name"] and o["name"].hex() in table


@pytest.mark.skipif(GIT is None, reason="no git on this machine")
def test_git_verify_pack_refuses_a_wrong_name(tmp_path):
    def verify(pack, idx, label):
        repo = str(tmp_path / label)
        assert subprocess.run([GIT, "init", "-q", "--bare", repo], env=ENV, capture_output=True).returncode == 0
        stem = os.path.join(repo, "objects", "pack", "pack-" + pack[-20:].hex())
        for ext, data in ((".pack", pack), (".idx", idx)):
            with open(stem + ext, "wb") as f:
                f.write(data)
        return subprocess.run([GIT, "verify-pack", stem + ".idx"], cwd=repo, env=ENV, capture_output=True)

    entries = [pc.blob(pc.SMALL), pc.blob(pc.MID), pc.delta(1, [("copy", 0, 100)])]
    pack, idx, layout = pw.write_pack(entries)
    r = verify(pack, idx, "good.git")
    assert r.returncode == 0, r.stderr
    assert [st for st, _ in pnm.read(pm.Model(pack, idx))] == [0, 0, 0]
    entries[0] = dict(entries[0], name=pnc.wrong(0))
    pack, idx, layout = pw.write_pack(entries)
    assert verify(pack, idx, "bad.git").returncode != 0
    m = pm.Model(pack, idx)
    order = pw.idx_order(layout)
    assert {k: pnm.read(m)[order[k]][0] for k in range(3)} == {0: pm.INVALID_CHECKSUM, 1: 0, 2: 0}
