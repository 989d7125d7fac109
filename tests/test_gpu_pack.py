"""git packfiles on the GPU (md_pack_open, md_pack_read; csrc/pack_kernels.hip).  Needs an MI355X: `pytest -m gpu`.
Yardsticks: the reader of tests/pack_model.py (checked against git itself by tests/test_pack_model.py) over the cases of
tests/pack_cases.py, hashlib for the names of the pack git wrote (tests/golden/git_pack) - never the code under test, and
no git here."""
import hashlib
import json
import os

import pytest

from tests import pack_cases as pc
from tests import pack_model as pm
from tests import pack_writer as pw

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "git_pack")
TYPE_NAMES = {1: "commit", 2: "tree", 3: "blob", 4: "tag"}


@pytest.fixture(scope="module")
def eng():
    from decompress_amd import engine
    return engine.default_engine(0)


@pytest.fixture(scope="module")
def built():
    """every case once, with its bytes and the model's reading"""
    out = {}
    for case in pc.cases():
        c = pc.build(case)
        c["model"] = pm.Model(c["pack"], c["idx"])
        out[c["name"]] = c
    return out


def _counts(p):
    """md_pack_last without the time"""
    d = p.last()
    assert (d.pop("apply_ns") > 0) == (d["apply_launches"] > 0)
    return d


def _open(pack, idx):
    from decompress_amd import pack as mp
    return mp.Pack(pack, idx)


def _check_table(p, m, label):
    assert p.info == m.info, label
    assert len(p.objects) == len(m.objects), label
    for i, (g, w) in enumerate(zip(p.objects, m.objects)):
        got = (g["name"], g["type"], g["size"], g["offset"], g["packed_len"], g["base"], g["depth"], g["status"])
        want = (w["name"], w["type"], w["size"], w["offset"], w["packed_len"], w["base"], w["depth"], w["status"])
        assert got == want, (label, i)
        assert p.find(w["name"]) == i, (label, i)
    assert p.find(hashlib.sha1(b"not in any pack").digest()) == -1


def _check_read(p, m, select, verify, label):
    rc, status, off, raw, res = p.read_raw(select, verify)
    assert rc == 0, label
    want = m.read(select, verify)
    idx = range(len(m.objects)) if select is None else select
    assert off == [sum(m.objects[i]["size"] for i in list(idx)[:j]) for j in range(len(list(idx)) + 1)], label
    for j, (st, data) in enumerate(want):
        assert status[j] == st, (label, j, status[j], st)
        if st == pm.OK:
            assert raw[off[j]:off[j + 1]] == data, (label, j)
    assert (res["entries"], res["failed"], res["written"]) == (len(want), sum(st != pm.OK for st, _ in want), off[-1]), label
    return status


def test_every_case_against_the_model(eng, built):
    from decompress_amd import engine
    for name, c in built.items():
        m = c["model"]
        assert m.rc == c["rc"], name
        if m.rc != pm.OK:
            with pytest.raises(engine.Error, match=engine.STATUS_NAMES[m.rc]):
                _open(c["pack"], c["idx"])
            continue
        p = _open(c["pack"], c["idx"])
        _check_table(p, m, name)
        for verify in (False, True):
            status = _check_read(p, m, None, verify, (name, verify))
            want = c.get("verify", c["expect"]) if verify else c["expect"]
            assert {k: status[c["order"][k]] for k in range(len(c["layout"])) if status[c["order"][k]] != 0} == want, (name, verify)
        p.close()


def test_selections_decode_every_needed_object_once(eng, built):
    c = built["a chain of 64, OFS and REF mixed"]
    m, order = c["model"], c["order"]
    p = _open(c["pack"], c["idx"])
    deepest, root = order[64], order[0]
    assert m.objects[deepest]["depth"] == 64 and m.objects[root]["depth"] == 0
    _check_read(p, m, [deepest], False, "the deepest alone")
    assert _counts(p) == {"rounds": 1, "inflate_launches": 1, "apply_launches": 64, "objects": 65, "bytes_in": len(c["pack"])}
    sub = [order[k] for k in (50, 2, 1, 33)]
    _check_read(p, m, sub, False, "a subset")
    assert p.last()["objects"] == len(m.closure(sub)) == 51 and p.last()["apply_launches"] == 50
    rep = [order[1], root, order[1], root, deepest, order[1]]  # a base and its delta, both twice; the base selected behind its delta
    _check_read(p, m, rep, True, "repeats")
    assert p.last()["objects"] == 65 and p.last()["rounds"] == 1
    _check_read(p, m, [], False, "nothing")
    rc, _, _, _, _ = p.read_raw([len(m.objects)])
    assert rc == -1
    p.close()
    c = built["a fan of 1000"]
    p = _open(c["pack"], c["idx"])
    sel = [c["order"][k] for k in range(1, 1001, 7)]  # the base comes through the closure alone
    _check_read(p, c["model"], sel, False, "a fan without its base")
    assert p.last()["objects"] == len(sel) + 1 and p.last()["apply_launches"] == 1
    p.close()


def test_room_exact_and_one_short(eng, built):
    c = built["copy lengths"]
    p = _open(c["pack"], c["idx"])
    need = c["model"].info["total_size"]
    rc, status, off, raw, res = p.read_raw(None, False, dst_cap=need)
    assert rc == 0 and status == [0, 0] and off[-1] == need
    rc, status, off, raw, res = p.read_raw(None, False, dst_cap=need - 1)
    assert rc == pm.END_OF_OUTPUT and res["written"] == need and off[-1] == need and raw == bytes(need - 1)  # (nothing was launched)
    p.close()


def test_rounds_of_the_workspace(eng):
    """the same results whatever "pack_workspace": 0 (one selected object a round), 1 MiB (several rounds; a chain that does
    not fit gets its own status) and the default"""
    entries = []
    deep = []
    for ch in range(5):
        base = pc.text(300 << 10, 50 + ch)
        first = len(entries)
        entries.append(pc.blob(base))
        cur = base
        for k in range(1, 6 if ch == 4 else 3):
            ins = pc._edit(cur, k)
            entries.append(pc.delta(first + k - 1, ins))
            cur = pw._result(cur, ins)
        deep.append(len(entries) - 1)
    pack, idx, layout = pw.write_pack(entries)
    order = pw.idx_order(layout)
    m = pm.Model(pack, idx)
    p = _open(pack, idx)
    sel = [order[k] for k in deep] + [order[0]]
    long_chain = order[deep[4]]  # four objects of 300 KiB beside it: more than 1 MiB
    try:
        eng.set_option("pack_workspace", 0)
        _check_read(p, m, sel, True, "workspace 0")
        assert p.last()["rounds"] == len(sel) and p.last()["inflate_launches"] == len(sel)
        eng.set_option("pack_workspace", 1)
        rc, status, off, raw, res = p.read_raw(sel, False)
        want = m.read(sel)
        assert rc == 0 and status == [pm.E_OUT_OF_MEMORY if i == long_chain else 0 for i in sel] and res["failed"] == 1
        for j, i in enumerate(sel):
            assert i == long_chain or raw[off[j]:off[j + 1]] == want[j][1], j
        assert 1 < p.last()["rounds"] < len(sel)
        q = _open(pack, idx)  # (md_pack_open's rounds of delta payloads)
        _check_table(q, m, "opened with 1 MiB")
        q.close()
    finally:
        eng.set_option("pack_workspace", 256)
    _check_read(p, m, sel, False, "the default")
    assert p.last()["rounds"] == 1
    p.close()


def test_a_pack_git_wrote(eng):
    with open(os.path.join(GOLDEN, "git.pack"), "rb") as f:
        pack = f.read()
    with open(os.path.join(GOLDEN, "git.idx"), "rb") as f:
        idx = f.read()
    with open(os.path.join(GOLDEN, "objects.json")) as f:
        table = json.load(f)
    p = _open(pack, idx)
    assert p.info["n"] == len(table) == 31 and p.info["failed"] == 0 and p.info["deltas"] == sum(o["depth"] > 0 for o in table.values())
    got = p.read(verify_crc=True)
    for o, (st, val) in zip(p.objects, got):
        assert st == "Ok", o["name"].hex()
        t, data = val
        want = table[o["name"].hex()]
        assert (TYPE_NAMES[t], len(data), o["depth"], hashlib.sha1(data).hexdigest()) == (want["type"], want["size"], want["depth"], want["sha1"])
        assert pw.object_name(t, data) == o["name"]  # the name, hashed again from what the GPU returned
    p.close()


def test_4096_objects_in_chains_of_8(eng):
    entries = []
    for ch in range(512):
        base = pc.text(400 + ch % 37, 1000 + ch)
        first = len(entries)
        entries.append(pc.blob(base))
        cur = base
        for k in range(1, 8):
            ins = pc._edit(cur, k)
            entries.append(pc.delta(first + k - 1, ins, "ref" if (ch + k) % 3 == 0 else "ofs"))
            cur = pw._result(cur, ins)
    pack, idx, layout = pw.write_pack(entries)
    m = pm.Model(pack, idx)
    assert m.info == {"n": 4096, "deltas": 3584, "max_depth": 7, "total_size": sum(len(x["data"]) for x in layout), "failed": 0}
    p = _open(pack, idx)
    _check_table(p, m, "4096")
    _check_read(p, m, None, True, "4096")
    assert _counts(p) == {"rounds": 1, "inflate_launches": 1, "apply_launches": 7, "objects": 4096, "bytes_in": len(pack)}
    p.close()


def test_python_pack_class(eng, built):
    from decompress_amd import pack as mp
    c = built["a root that fails its checksum"]
    ents, info = mp.index(c["idx"])
    assert info["n"] == 5 and [e["name"] for e in ents] == sorted(x["name"] for x in c["layout"])
    p = mp.Pack(c["pack"], c["idx"])
    got = p.read()
    order = c["order"]
    assert got[order[0]] == ("Error", "Invalid_checksum") and got[order[1]] == got[order[2]] == ("Error", "Invalid delta base")
    assert got[order[3]] == ("Ok", (3, pc.SMALL)) and got[order[4]] == ("Ok", (3, pc.SMALL[1:10]))
    assert p.read([order[4]]) == [("Ok", (3, pc.SMALL[1:10]))] and p.last()["objects"] == 2
    assert p.find(c["layout"][3]["name"].hex()) == order[3]
    p.close()
