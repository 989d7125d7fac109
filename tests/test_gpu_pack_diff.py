"""Trees of a git pack diffed on the GPU (md_pack_diff; csrc/pack_diff_kernels.hip).  Needs an MI355X: `pytest -m gpu`.
Yardstick: tests/pack_diff_model.py - the header's rules in Python, held to `git diff-tree` on the CPU
(test_pack_diff_model.py) - held to exactly: every record in its order, the names blob, every status and count.  No tolerance
anywhere."""
import ctypes
import faulthandler

import pytest

from tests import pack_diff_cases as dc
from tests import pack_diff_model as dm
from tests import pack_graph_model as gm

pytestmark = pytest.mark.gpu
TIME_LIMIT = 120  # seconds a test may take before the process is ended (each takes a few)
COUNTS = ("pairs", "changes", "name_bytes", "levels", "opaque", "failed", "trees_read", "launches")


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(TIME_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def eng():
    from decompress_amd import engine
    return engine.default_engine(0)


@pytest.fixture(scope="module")
def built():
    """every case built once, with the model's graph and its pairs as indices: [(case, graph model, pairs)]"""
    out = []
    for c in dc.cases():
        b = dc.build(c)
        g = gm.Graph(b["pack"], b["idx"])
        out.append((b, g, dm.commit_pairs(g)[1] if b["commits"] else b["ipairs"]))
    return out


def _open(c):
    from decompress_amd import pack as mp
    return mp.Pack(c["pack"], c["idx"])


def _same(got, m, label):
    rc, recs, names, status, info = got
    assert rc == 0, label
    assert status == m.status, label
    assert len(recs) == len(m.records), label
    for k, (r, w) in enumerate(zip(recs, m.records)):
        assert r == w, (label, k)
    assert names == m.names, label
    assert {k: info[k] for k in COUNTS} == {k: m.info[k] for k in COUNTS}, label


def test_every_case_is_the_models_diff(eng, built):
    for c, g, pairs in built:
        if c["workspace"] is not None:
            continue
        p = _open(c)
        gr = p.graph()
        for recursive in (True, False):
            _same(p.diff_raw(pairs, recursive, gr), dm.Diff(g, pairs, recursive), (c["name"], recursive))
        gr.close(), p.close()


def test_launches_do_not_grow_with_the_pairs(eng, built):
    one = [b for b in built if b[0]["name"] == "the same two trees as one pair"][0]
    many = [b for b in built if b[0]["name"] == "200 pairs that share their trees"][0]
    infos = []
    for c, g, pairs in (one, many):
        p = _open(c)
        infos.append(p.diff_raw(pairs)[4])
        p.close()
    assert (infos[0]["pairs"], infos[1]["pairs"]) == (1, 200) and infos[1]["changes"] == 200 * infos[0]["changes"]
    assert infos[0]["launches"] == infos[1]["launches"] == 10 and infos[0]["trees_read"] == infos[1]["trees_read"] == 4


def test_a_tree_a_round_gives_the_same_records(eng, built):
    seen = most = 0
    for c, g, pairs in built:
        if c["workspace"] is None:
            continue
        p = _open(c)
        gr = p.graph()
        try:
            eng.set_option("pack_workspace", c["workspace"])
            got = p.diff_raw(pairs, True, gr)
            rounds = p.last()["rounds"]
        finally:
            eng.set_option("pack_workspace", 256)
        _same(got, dm.Diff(g, pairs), c["name"])
        most = max(most, rounds)  # (of the last level's read: a round a tree)
        gr.close(), p.close()
        seen += 1
    assert seen >= 3 and most >= 4


def test_changes_of_a_history_are_the_models(eng, built):
    from decompress_amd import pack as mp
    seen = 0
    for c, g, pairs in built:
        if not c["commits"]:
            continue
        p = _open(c)
        commits, got = p.changes()
        want_commits, want_pairs = dm.commit_pairs(g)
        assert commits == want_commits and want_pairs == pairs and len(commits) == 300, c["name"]
        want = [(tag, recs) if tag == "Ok" else (mp._status_name(tag), None) for tag, recs in dm.Diff(g, pairs).per_pair()]
        assert got == want, c["name"]
        last = p.diff_last()
        for key, value in c["stats"].items():
            assert last[key] == value, (c["name"], key)
        # a few commits alone are those commits of the whole
        some = commits[5:300:37]
        assert p.changes(some)[1] == [got[commits.index(k)] for k in some], c["name"]
        p.close()
        seen += 1
    assert seen == 2


def test_caps_and_invalid_arguments(eng, built):
    from decompress_amd import engine
    c, g, pairs = [b for b in built if b[0]["name"] == "a file becomes a directory"][0]
    p = _open(c)
    gr = p.graph()
    rc, recs, names, status, info = p.diff_raw(pairs, True, gr)
    assert rc == 0 and info["changes"] == 6 and info["name_bytes"] == len(names) > 0
    assert p.diff_raw(pairs, True, gr, cap=info["changes"] - 1)[0] == 2
    assert p.diff_raw(pairs, True, gr, names_cap=info["name_bytes"] - 1)[0] == 2
    lib, h = eng.lib, ctypes.c_void_p()
    n = len(p.objects)
    a, b = (ctypes.c_uint32 * 1)(pairs[0][0]), (ctypes.c_uint32 * 1)(pairs[0][1])
    args = (eng.ctx, p._h, gr._h, p._pack, len(p._pack), 1, a, b)
    assert lib.md_pack_diff(*args, 1, ctypes.byref(h)) == 0 and h.value
    assert lib.md_pack_diff_changes(h, None, 0, None, 0) == 0  # cap == 0 only asks
    assert lib.md_pack_diff_changes(h, None, 3, None, 0) == -1
    lib.md_pack_diff_free(h)
    assert lib.md_pack_diff(*args, 2, ctypes.byref(h)) == -1 and not h.value
    assert lib.md_pack_diff(eng.ctx, p._h, gr._h, p._pack, len(p._pack), 1, (ctypes.c_uint32 * 1)(n), b, 1, ctypes.byref(h)) == -1
    assert lib.md_pack_diff(eng.ctx, p._h, gr._h, p._pack, len(p._pack), 1, None, b, 1, ctypes.byref(h)) == -1
    assert lib.md_pack_diff(eng.ctx, p._h, None, p._pack, len(p._pack), 1, a, b, 1, ctypes.byref(h)) == -1
    other = [x for x in built if x[0]["name"] == "every change of mode"][0][0]
    assert lib.md_pack_diff(eng.ctx, p._h, gr._h, other["pack"], len(other["pack"]), 1, a, b, 1, ctypes.byref(h)) == 21
    q = _open(other)
    gq = q.graph()
    assert lib.md_pack_diff(eng.ctx, p._h, gq._h, p._pack, len(p._pack), 1, a, b, 1, ctypes.byref(h)) == 21  # a graph of another table
    with pytest.raises(engine.Error):
        p.diff([(n, None)], graph=gr)
    # both sides the empty tree, and no pair at all
    assert p.diff([(None, None)], graph=gr) == [("Ok", [])] and p.diff([], graph=gr) == []
    gq.close(), q.close(), gr.close(), p.close()


def test_a_diff_disturbs_no_other_call_of_the_context(eng, built):
    """the device-resident form of the read shares the read's scratch: what md_pack_read, md_pack_graph_build and
    md_pack_reachable gave before a diff on the same context they give after it"""
    c, g, pairs = [b for b in built if b[0]["name"] == "the history of 300 through changes()"][0]
    p = _open(c)

    def everything():
        gr = p.graph()
        top = [i for i, o in enumerate(p.objects) if o["type"] == 1][-1]
        out = (p.read_raw(), gr.first.tolist(), gr.to.tolist(), gr.kind.tolist(), gr.status.tolist(), gr.reachable([top]).tolist(), p.verify())
        gr.close()
        return out

    before = everything()
    _, got = p.changes()
    assert all(tag == "Ok" for tag, _ in got)
    assert everything() == before
    p.close()
