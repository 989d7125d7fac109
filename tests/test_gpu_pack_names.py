"""Object names verified on the GPU (MD_PACK_VERIFY_NAME in md_pack_read, md_pack_verify; csrc/sha1_kernels.hip).
Needs an MI355X: `pytest -m gpu`.  Yardsticks: tests/pack_names_model.py - the reader of tests/pack_model.py and hashlib -
over the cases of tests/pack_cases.py and tests/pack_name_cases.py, and the pack git wrote (tests/golden/git_pack); never
the code under test.  ("pack_workspace" counts MiB: the small workspaces here are 0 - one selected object a round - and 1.)"""
import hashlib
import json
import os

import pytest

from tests import pack_cases as pc
from tests import pack_model as pm
from tests import pack_name_cases as pnc
from tests import pack_names_model as pnm
from tests import pack_writer as pw

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "git_pack")
CRC, NAME = 1, 2


@pytest.fixture(scope="module")
def eng():
    from decompress_amd import engine
    return engine.default_engine(0)


def _expected(m, select, flags):
    return pnm.read(m, select, bool(flags & CRC)) if flags & NAME else m.read(select, bool(flags & CRC))


@pytest.fixture(scope="module")
def built():
    """every case that opens, once: its bytes, the model, and what a read of everything gives for flags 0 .. 3"""
    out = {}
    for case in pc.cases() + pnc.cases():
        c = pc.build(case)
        c["model"] = pm.Model(c["pack"], c["idx"])
        if c["model"].rc != pm.OK:
            continue
        c["want"] = [_expected(c["model"], None, flags) for flags in range(4)]
        assert c["name"] not in out
        out[c["name"]] = c
    return out


def _open(c):
    from decompress_amd import pack as mp
    return mp.Pack(c["pack"], c["idx"])


def _read(p, m, select, flags, want, label):
    """a read held to `want`, status by status, and byte by byte where an object is Ok"""
    rc, status, off, raw, res = p.read_raw(select, bool(flags & CRC), None, bool(flags & NAME))
    assert rc == 0, label
    idx = list(range(len(m.objects)) if select is None else select)
    assert off == [sum(m.objects[i]["size"] for i in idx[:j]) for j in range(len(idx) + 1)], label
    for j, (st, data) in enumerate(want):
        assert status[j] == st, (label, j, status[j], st)
        if st == pm.OK:
            assert raw[off[j]:off[j + 1]] == data, (label, j)
    assert (res["entries"], res["failed"], res["written"]) == (len(want), sum(st != pm.OK for st, _ in want), off[-1]), label
    return status


def test_every_case_against_the_names_model(eng, built):
    assert len(built) > 50
    for name, c in built.items():
        p = _open(c)
        for flags in (NAME, NAME | CRC):
            status = _read(p, c["model"], None, flags, c["want"][flags], (name, flags))
            if "names" in c:  # and the case's own word
                want = c.get("both", c["names"]) if flags & CRC else c["names"]
                assert {k: status[c["order"][k]] for k in range(len(c["layout"])) if status[c["order"][k]] != 0} == want, (name, flags)
        hashed = eng.sha1_last()
        decoded = p.last()["objects"]
        assert hashed["messages"] == decoded and (hashed["launches"] >= 1) == (decoded > 0) and (hashed["device_ns"] > 0) == (decoded > 0), name
        p.close()


def test_the_flag_is_the_only_switch(eng, built):
    seen = 0
    for name, c in built.items():
        if "names" not in c:
            continue
        p = _open(c)
        status = _read(p, c["model"], None, 0, c["want"][0], name)
        assert not any(status), name
        _read(p, c["model"], None, CRC, c["want"][CRC], name)
        seen += bool(c["names"])
        p.close()
    assert seen >= 8
    from decompress_amd import engine
    c = built["a wrong name on a lone object"]
    p = _open(c)
    for flags in (4, 8, 7, 1 << 31):
        assert p.verify_raw(None, flags)[0] == -1
    with pytest.raises(engine.Error):
        p.verify([len(p.objects)])
    p.close()


def test_selections(eng, built):
    for name, c in built.items():
        if "select" not in c:
            continue
        p = _open(c)
        sel = [c["order"][k] for k in c["select"]]
        for flags in (NAME, NAME | CRC):
            status = _read(p, c["model"], sel, flags, _expected(c["model"], sel, flags), (name, flags))
            assert status == c["selected"], name
        p.close()
    # the deepest delta alone, its misnamed base two levels down never selected: the round decodes and hashes the whole chain
    c = built["a wrong name in the middle of a chain"]
    p = _open(c)
    assert p.read([c["order"][4]], verify_names=True) == [("Error", "Invalid delta base")]
    assert p.last()["objects"] == 5 and eng.sha1_last()["messages"] == 5
    assert p.read([c["order"][4]])[0][0] == "Ok" and p.read([c["order"][1]], verify_names=True)[0][0] == "Ok"
    p.close()


def test_rounds_of_the_workspace(eng, built):
    """with "pack_workspace" = 0 every selected object is a round of its own and a base is decoded - and hashed - in every
    round that needs it: the statuses are the same"""
    try:
        eng.set_option("pack_workspace", 0)
        for name, c in built.items():
            p = _open(c)
            _read(p, c["model"], None, NAME | CRC, c["want"][NAME | CRC], (name, "workspace 0"))
            assert p.last()["rounds"] >= 1 or not any(o["status"] == pm.OK for o in c["model"].objects), name
            p.close()
        c = built["a wrong name on a base of two"]
        p = _open(c)
        sel = [c["order"][k] for k in (2, 3, 1)]  # two deltas of one base, then the base: it stands in the second delta's round
        status = _read(p, c["model"], sel, NAME, _expected(c["model"], sel, NAME), "a base in two rounds")
        assert status == [pm.INVALID_PACK_BASE, pm.INVALID_PACK_BASE, pm.INVALID_CHECKSUM]
        assert p.last()["rounds"] == 2 and p.last()["objects"] == 4 == eng.sha1_last()["messages"]
        p.close()
    finally:
        eng.set_option("pack_workspace", 256)


def _big_chains():
    """five chains on bases of 300 KiB, one name wrong in the third: more than 1 MiB of scratch"""
    entries, tips = [], []
    for ch in range(5):
        base = pc.text(300 << 10, 80 + ch)
        first = len(entries)
        entries.append(pc.blob(base, **({"name": pnc.wrong(50)} if ch == 2 else {})))
        cur = base
        for k in range(1, 3):
            ins = pc._edit(cur, k)
            entries.append(pc.delta(first + k - 1, ins))
            cur = pw._result(cur, ins)
        tips.append(len(entries) - 1)
    return entries, tips


def test_several_rounds_of_one_mib_and_verify(eng):
    from decompress_amd import pack as mp
    entries, tips = _big_chains()
    pack, idx, layout = pw.write_pack(entries)
    order = pw.idx_order(layout)
    m = pm.Model(pack, idx)
    p = mp.Pack(pack, idx)
    sel = [order[k] for k in tips] + [order[0], order[6]]
    want = pnm.read(m, sel, True)
    assert [st for st, _ in want] == [0, 0, pm.INVALID_PACK_BASE, 0, 0, 0, pm.INVALID_CHECKSUM]
    try:
        eng.set_option("pack_workspace", 1)
        _read(p, m, sel, NAME | CRC, want, "1 MiB")
        assert 1 < p.last()["rounds"] < len(sel)
        rc, status, res = p.verify_raw(sel, NAME | CRC)
        assert rc == 0 and status == [st for st, _ in want] and res == {"entries": len(sel), "failed": 2, "written": 0}
        assert p.last()["rounds"] > 1
    finally:
        eng.set_option("pack_workspace", 256)
    rc, status, res = p.verify_raw(sel, NAME | CRC)
    assert rc == 0 and status == [st for st, _ in want] and p.last()["rounds"] == 1
    p.close()


def test_one_block_a_launch(eng, built):
    from decompress_amd import engine
    c = built["message lengths around the block"]
    p = _open(c)
    try:
        eng.set_option("sha1_launch_blocks", 1)
        _read(p, c["model"], None, NAME, c["want"][NAME], "one block a launch")
        last = eng.sha1_last()
    finally:
        eng.set_option("sha1_launch_blocks", engine.SHA1_LAUNCH_BLOCKS)
    assert last["launches"] == (pnc.message_length(3, 400) + 9 + 63) // 64 == 7 and last["messages"] == len(c["layout"])
    p.close()


def test_a_pack_git_wrote(eng):
    from decompress_amd import pack as mp
    with open(os.path.join(GOLDEN, "git.pack"), "rb") as f:
        pack = f.read()
    with open(os.path.join(GOLDEN, "git.idx"), "rb") as f:
        idx = f.read()
    with open(os.path.join(GOLDEN, "objects.json")) as f:
        table = json.load(f)
    p = mp.Pack(pack, idx)
    assert p.verify() == ["Ok"] * 31 and mp.check_trailers(pack, idx) == (True, True)
    got = p.read(verify_crc=True, verify_names=True)
    for o, (st, val) in zip(p.objects, got):
        assert st == "Ok" and hashlib.sha1(val[1]).hexdigest() == table[o["name"].hex()]["sha1"]
    assert mp.hash_objects([o["type"] for o in p.objects], [val[1] for _, val in got]) == [o["name"] for o in p.objects]
    p.close()
    # one name replaced - a whole object that deltas hang off - and the idx written again around it
    m = pm.Model(pack, idx)
    children = [sum(1 for o in m.objects if o["link"] and o["root"] == i) for i in range(len(m.objects))]
    victim = max(range(len(m.objects)), key=lambda i: children[i])
    assert children[victim] >= 2
    layout = [{"name": o["name"], "offset": o["offset"], "packed_len": o["packed_len"]} for o in m.objects]
    layout[victim]["name"] = pnc.wrong(99)
    idx2 = pw.write_idx(pack, layout)
    m2 = pm.Model(pack, idx2)
    assert m2.rc == pm.OK
    at = {o["offset"]: i for i, o in enumerate(m2.objects)}
    hit = {at[o["offset"]] for i, o in enumerate(m.objects) if i == victim or (o["link"] and o["root"] == victim)}
    p = mp.Pack(pack, idx2)
    want = pnm.read(m2, None, True)
    status = _read(p, m2, None, NAME | CRC, want, "one name replaced")
    assert {i for i, st in enumerate(status) if st != 0} == hit and len(hit) == children[victim] + 1
    assert p.verify() == [mp._status_name(st) for st in status] and mp.check_trailers(pack, idx2) == (True, True)
    p.close()


def test_verify_equals_read(eng, built):
    for name, c in built.items():
        p = _open(c)
        for flags in range(4):
            rc, status, res = p.verify_raw(None, flags)
            want = c["want"][flags]
            assert rc == 0 and status == [st for st, _ in want], (name, flags)
            assert res == {"entries": len(want), "failed": sum(st != pm.OK for st, _ in want), "written": 0}, (name, flags)
        p.close()
    c = built["a chain of 64, OFS and REF mixed"]
    p = _open(c)
    assert p.verify() == ["Ok"] * 65
    assert p.last()["objects"] == 65 and p.last()["rounds"] == 1 and p.last()["apply_launches"] == 64
    last = eng.sha1_last()
    assert last["messages"] == 65 and last["launches"] == 1
    sel = [c["order"][64], c["order"][0], c["order"][64]]  # repeats need no copy: each object once
    rc, status, res = p.verify_raw(sel, NAME | CRC)
    assert rc == 0 and status == [0, 0, 0] and res["written"] == 0 and p.last()["objects"] == 65
    assert p.verify([]) == [] and p.verify(crc=False, names=False) == ["Ok"] * 65
    p.close()


def test_python_names_interface(eng, built):
    from decompress_amd import pack as mp
    c = built["a wrong name on a base of two"]
    p = mp.Pack(c["pack"], c["idx"])
    order = c["order"]
    got = p.verify()
    assert [got[order[k]] for k in range(6)] == ["Ok", "Invalid_checksum", "Invalid delta base", "Invalid delta base", "Ok", "Ok"]
    assert p.verify(names=False) == ["Ok"] * 6
    got = p.read(verify_names=True)
    assert got[order[1]] == ("Error", "Invalid_checksum") and got[order[0]] == ("Ok", (3, c["layout"][0]["data"]))
    assert p.read([order[0]], True, True) == [("Ok", (3, c["layout"][0]["data"]))]
    p.close()
    bufs = [x["data"] for x in c["layout"]]
    assert mp.hash_objects([3] * 6, bufs) == mp.hash_objects(["blob"] * 6, bufs) == [pw.object_name(3, b) for b in bufs]
    assert mp.hash_objects(["commit", "tree", "tag"], [pc.COMMIT, pnc.TREE, pnc.TAG]) == [pw.object_name(t, b) for t, b in
                                                                                           ((1, pc.COMMIT), (2, pnc.TREE), (4, pnc.TAG))]
    with pytest.raises(ValueError):
        mp.hash_objects([0], [b"x"])
    assert mp.check_trailers(c["pack"], c["idx"]) == (True, True)
