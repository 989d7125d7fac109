"""The idx of a pack from the pack alone on the GPU (md_pack_index_build; csrc/pack_build_kernels.hip).  Needs an
MI355X: `pytest -m gpu`.  Yardstick: the plain-Python index-pack of tests/pack_build_model.py (checked against git itself by
tests/test_pack_build_model.py) over the cases of tests/pack_build_cases.py - never the code under test, and no git here."""
import pytest

from tests import pack_build_cases as bc
from tests import pack_build_model as bm
from tests import pack_cases as pc
from tests import pack_model as pm

pytestmark = pytest.mark.gpu
END_OF_OUTPUT = 2


@pytest.fixture(scope="module")
def eng():
    from decompress_amd import engine
    return engine.default_engine(0)


def _build(c, **kw):
    from decompress_amd import pack as mp
    return mp.build_index_raw(c["pack"], c["flags"], **kw)


def _case(name):
    return [c for c in bc.cases() if c["name"] == name][0]


def test_every_accepted_case_gets_the_models_idx_and_reads_back(eng):
    from decompress_amd import pack as mp
    for c in bc.cases():
        if not bc.accepted(c):
            continue
        m = bc.model(c["name"])
        rc, idx, offsets, status, res = _build(c)
        assert rc == 0, (c["name"], rc, res)
        assert idx == m.idx, c["name"]
        assert offsets == m.offsets and status == [0] * m.n, c["name"]
        assert res == {"n": m.n, "failed": 0, "idx_len": len(m.idx), "bad_offset": bm.NO_OFFSET, "bad_status": 0}, c["name"]
        last = mp.build_last()
        assert (last["candidates"], last["generations"], last["bytes_in"]) == (m.candidates, m.generations, len(c["pack"])), (c["name"], last)
        # pack in, idx out, md_pack_open on the result: everything read with both verify flags
        p = mp.Pack(c["pack"], idx)
        got = p.read(None, verify_crc=True, verify_names=True)
        by_offset = {o["offset"]: k for k, o in enumerate(p.objects)}
        assert len(got) == m.n, c["name"]
        for off, (t, data) in zip(m.offsets, m.objects):
            assert got[by_offset[off]] == ("Ok", (t, data)), (c["name"], off)
        p.close()


def test_every_refused_case_as_the_model_refuses_it(eng):
    from decompress_amd import engine
    from decompress_amd import pack as mp
    seen = set()
    for c in bc.cases():
        if bc.accepted(c):
            continue
        m = bc.model(c["name"])
        assert m.rc != 0
        if m.n == 0:  # refused before any object has a status: the call's checks, the trailer, the walk
            rc, idx, offsets, status, res = mp.build_index_raw(c["pack"], c["flags"], idx_cap=4096, cap=16)
            assert (rc, offsets, status) == (m.rc, [], []), (c["name"], rc, res)
            assert (res["n"], res["failed"], res["bad_offset"]) == (0, 0, m.bad_offset), (c["name"], res)
            assert (res["bad_status"] != 0) == (m.bad_status != 0), (c["name"], res)
            if m.bad_status not in (0, pm.DECODER_ERROR):
                assert res["bad_status"] == m.bad_status, (c["name"], res)
            assert idx == bytes(4096), c["name"]
        else:
            rc, idx, offsets, status, res = mp.build_index_raw(c["pack"], c["flags"], idx_cap=8 + 1024 + 28 * m.n + 40, cap=m.n)
            assert rc == m.rc and offsets == m.offsets, (c["name"], rc, res)
            assert status == m.status, (c["name"], status, m.status)
            assert res == {"n": m.n, "failed": sum(st != 0 for st in m.status), "idx_len": 8 + 1024 + 28 * m.n + 40, "bad_offset": m.bad_offset,
                           "bad_status": 0}, (c["name"], res)
            assert idx == bytes(len(idx)), c["name"]  # no idx byte written
        with pytest.raises(engine.Error, match=engine.STATUS_NAMES[m.rc]):
            mp.build_index(c["pack"], check_trailer=bool(c["flags"] & 1))
        seen.add(m.rc)
    assert {pm.INVALID_PACK, pm.UNSUPPORTED, pm.INVALID_CHECKSUM, pm.INVALID_SIZE, pm.INVALID_DELTA, pm.MISSING_BASE} <= seen
    rc, _, _, _, _ = mp.build_index_raw(_case("copy lengths")["pack"], 2, idx_cap=4096, cap=4)
    assert rc == pm.E_INVALID_ARGUMENT  # an unknown flag


def test_generations(eng):
    from decompress_amd import pack as mp
    for name, want in (("a fan of 1000", 2), ("copy lengths", 1), ("1 REF links, bases behind", 2), ("2 REF links, bases in front", 3),
                       ("3 REF links, bases behind", 4)):
        c = _case(name)
        assert mp.build_index(c["pack"]) == bc.model(name).idx
        assert mp.build_last()["generations"] == bc.model(name).generations == want, name


def test_a_small_workspace_gives_the_same_idx(eng):
    """"pack_workspace" counts MiB: 0 is one selected object a round, so a generation takes several rounds"""
    from decompress_amd import pack as mp
    try:
        for name, mib in (("a chain of 64, OFS and REF mixed", 0), ("the golden pack", 0), ("a fan of 1000", 1)):
            c = _case(name)
            eng.set_option("pack_workspace", 256)
            want = mp.build_index(c["pack"])
            wide = mp.build_last()
            eng.set_option("pack_workspace", mib)
            assert mp.build_index(c["pack"]) == want == bc.model(name).idx, name
            narrow = mp.build_last()
            assert narrow["generations"] == wide["generations"] and narrow["rounds"] >= wide["rounds"], (name, wide, narrow)
            if mib == 0:
                assert narrow["rounds"] > narrow["generations"] and narrow["rounds"] > wide["rounds"], (name, wide, narrow)
    finally:
        eng.set_option("pack_workspace", 256)


def test_room_exact_and_one_short_and_no_arrays(eng):
    from decompress_amd import pack as mp
    c = _case("copy lengths")
    m = bc.model(c["name"])
    rc, idx, offsets, status, res = _build(c, idx_cap=len(m.idx), cap=m.n)
    assert rc == 0 and idx == m.idx and offsets == m.offsets and status == [0] * m.n
    rc, idx, offsets, status, res = _build(c, idx_cap=len(m.idx) - 1, cap=m.n)
    assert rc == END_OF_OUTPUT and idx == bytes(len(m.idx) - 1) and offsets == m.offsets
    assert (res["n"], res["idx_len"]) == (m.n, len(m.idx))
    rc, idx, offsets, status, res = _build(c, idx_cap=len(m.idx), cap=0)
    assert rc == 0 and idx == m.idx and offsets == [] and status == [] and res["n"] == m.n
    rc, idx, offsets, status, res = _build(c, idx_cap=len(m.idx), cap=1)
    assert rc == 0 and offsets == m.offsets[:1] and status == [0]


def test_pack_without_an_idx_in_python(eng):
    from decompress_amd import pack as mp
    c = _case("the golden pack")
    p = mp.Pack(c["pack"])
    assert p.idx == c["idx"] and p.info["n"] == 31 and p.info["failed"] == 0
    assert p.verify() == ["Ok"] * 31
    assert p.build_last()["generations"] == bc.model(c["name"]).generations
    p.close()


def test_open_and_read_are_what_they_were(eng):
    """the table builder was factored for the index builder: two existing cases through md_pack_open and md_pack_read"""
    from decompress_amd import pack as mp
    for name in ("a chain of 64, OFS and REF mixed", "a REF base that is missing"):
        c = pc.build([c for c in pc.cases() if c["name"] == name][0])
        m = pm.Model(c["pack"], c["idx"])
        p = mp.Pack(c["pack"], c["idx"])
        assert p.info == m.info
        assert [(o["name"], o["type"], o["size"], o["base"], o["depth"], o["status"]) for o in p.objects] == \
            [(o["name"], o["type"], o["size"], o["base"], o["depth"], o["status"]) for o in m.objects]
        rc, status, off, raw, _ = p.read_raw(None, True)
        want = m.read(None, True)
        assert rc == 0 and status == [st for st, _ in want]
        assert all(raw[off[j]:off[j + 1]] == data for j, (st, data) in enumerate(want) if st == 0)
        p.close()
