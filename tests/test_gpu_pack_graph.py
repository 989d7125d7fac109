"""The object graph of a git pack on the GPU (md_pack_graph_build, md_pack_reachable; csrc/pack_graph_kernels.hip).
Needs an MI355X: `pytest -m gpu`.  Yardstick: tests/pack_graph_model.py - the header's rules in Python, held to git on the
CPU (test_pack_graph_model.py) - held to exactly: every edge, kind, flag, status and count, the marks of every walk, the
objects it expanded and the launches it took.  No tolerance anywhere."""
import ctypes
import faulthandler

import numpy as np
import pytest

from tests import pack_graph_cases as gc
from tests import pack_graph_model as gm

pytestmark = pytest.mark.gpu
TIME_LIMIT = 120  # seconds a test may take before the process is ended (each takes a few)
COUNTS = ("n", "edges", "absent", "mistyped", "malformed", "failed", "parsed", "rounds", "parse_launches")


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
    """every case built once, with the model's graph: [(case, model)]"""
    return [(gc.build(c), gm.Graph(gc.build(c)["pack"], gc.build(c)["idx"])) for c in gc.cases()]


def _open(c):
    from decompress_amd import pack as mp
    return mp.Pack(c["pack"], c["idx"])


def _same_graph(g, m, label):
    assert g.first.tolist() == m.first, label
    assert g.to.tolist() == m.to, label
    assert g.kind.tolist() == m.kind, label
    assert g.status.tolist() == m.status, label


def test_every_case_is_the_models_graph(eng, built):
    for c, m in built:
        if c["workspace"] is not None:
            continue
        p = _open(c)
        for crc in (False, True):
            g = p.graph(verify_crc=crc)
            _same_graph(g, m, c["name"])
            assert {k: g.info[k] for k in COUNTS} == m.info, c["name"]
            assert g.connected() == (not m.info["absent"] and not m.info["mistyped"] and not any(m.status)), c["name"]
            assert len(g.missing()) == m.info["absent"] and len(g.mistyped()) == m.info["mistyped"], c["name"]
            for e in g.missing()[:5]:
                assert e[2] is None and e[3] & gm.ABSENT and g.edges_of(e[0])[e[1]] == e, c["name"]
            g.close()
        p.close()


def test_rounds_of_the_workspace_give_the_same_graph(eng, built):
    seen = deltas = 0
    for c, m in built:
        if c["workspace"] is None:
            continue
        p = _open(c)
        try:
            eng.set_option("pack_workspace", c["workspace"])
            g = p.graph()
        finally:
            eng.set_option("pack_workspace", 256)
        _same_graph(g, m, c["name"])
        assert g.info["rounds"] >= 3 and g.info["parsed"] >= m.info["parsed"] and g.info["parse_launches"] >= g.info["rounds"], c["name"]
        if m.model.info["deltas"]:  # a base stands in its own round and in those of what hangs off it: decoded and parsed again
            assert g.info["parsed"] > m.info["parsed"], c["name"]
            deltas += 1
        assert {k: g.info[k] for k in COUNTS[:6]} == {k: m.info[k] for k in COUNTS[:6]}, c["name"]
        one = p.graph()
        _same_graph(one, m, c["name"])
        assert one.info["rounds"] == 1 and one.info["parsed"] == m.info["parsed"]
        g.close(), one.close(), p.close()
        seen += 1
    assert seen >= 3 and deltas >= 2


def test_walks_are_the_models(eng, built):
    seen = 0
    for c, m in built:
        if not c["walks"]:
            continue
        p = _open(c)
        g = p.graph()
        for roots, exclude in c["walks"]:
            r, x = [c["order"][k] for k in roots], [c["order"][k] for k in exclude]
            marks, expanded, rounds = m.reachable(r, x)
            got = g.reachable(r, x)
            assert got.tolist() == [i for i, v in enumerate(marks) if v], (c["name"], roots, exclude)
            last = g.reach_last()
            assert {k: last[k] for k in m.stats} == m.stats, (c["name"], roots, exclude)
            assert (last["expanded"], last["rounds"]) == (expanded, rounds)
            seen += 1
        # roots by name are roots by index
        if c["walks"][0][0]:
            k = c["order"][c["walks"][0][0][0]]
            assert g.reachable([p.objects[k]["name"]]).tolist() == g.reachable([k]).tolist()
        g.close(), p.close()
    assert seen >= 20


def test_a_history_takes_launches_by_tree_depth_not_by_generation(eng, built):
    c, m = [b for b in built if b[0]["name"] == "a linear history of 300"][0]
    p = _open(c)
    g = p.graph()
    top = c["order"][c["walks"][0][0][0]]
    got = g.reachable([top])
    last = g.reach_last()
    d = m.tree_depth(top)
    assert d == 4 and last["rounds"] <= d + 2 and last["rounds"] < 20 and last["host_closed"] == 300
    assert len(got) == g.info["n"] == last["marked"]
    g.close(), p.close()


def test_invalid_arguments(eng, built):
    from decompress_amd import engine
    c, m = built[0]
    p = _open(c)
    lib, h = eng.lib, ctypes.c_void_p()
    assert lib.md_pack_graph_build(eng.ctx, p._h, p._pack, len(p._pack), 2, ctypes.byref(h)) == -1 and not h.value
    assert lib.md_pack_graph_build(eng.ctx, p._h, p._pack, len(p._pack), 4, ctypes.byref(h)) == -1
    assert lib.md_pack_graph_build(eng.ctx, p._h, None, 0, 0, ctypes.byref(h)) == -1
    assert lib.md_pack_graph_build(eng.ctx, None, p._pack, len(p._pack), 0, ctypes.byref(h)) == -1
    other = gc.build(gc.cases()[3])["pack"]
    assert lib.md_pack_graph_build(eng.ctx, p._h, other, len(other), 0, ctypes.byref(h)) == 21
    g = p.graph()
    n = g.info["n"]
    with pytest.raises(engine.Error):
        g.reachable([n])
    with pytest.raises(engine.Error):
        g.reachable([0], [n])
    with pytest.raises(KeyError):
        g.reachable([b"\x07" * 20])
    mark, count, one = np.zeros(n, dtype=np.uint8), ctypes.c_uint64(0), (ctypes.c_uint64 * 1)(0)
    assert lib.md_pack_reachable(eng.ctx, g._h, None, 1, None, 0, mark.ctypes.data, ctypes.byref(count)) == -1
    assert lib.md_pack_reachable(eng.ctx, g._h, one, 1, None, 1, mark.ctypes.data, ctypes.byref(count)) == -1
    assert lib.md_pack_reachable(eng.ctx, g._h, one, 1, None, 0, None, ctypes.byref(count)) == -1
    assert lib.md_pack_reachable(eng.ctx, g._h, one, 1, None, 0, mark.ctypes.data, None) == -1
    assert lib.md_pack_reachable(eng.ctx, g._h, one, 1, None, 0, mark.ctypes.data, ctypes.byref(count)) == 0 and count.value >= 1
    # the size query, and a cap that is too small
    first = np.zeros(n + 1, dtype=np.uint64)
    assert lib.md_pack_graph_edges(g._h, None, None, None, 0) == 0
    assert lib.md_pack_graph_edges(g._h, first.ctypes.data, g.to.ctypes.data, g.kind.ctypes.data, g.info["edges"] - 1) == 2
    g.close(), p.close()


def test_extract_writes_the_pack_of_what_is_reachable(eng, built):
    from decompress_amd import pack as mp
    c, m = [b for b in built if b[0]["name"] == "a linear history of 300"][0]
    p = _open(c)
    k_mid = [k for k, e in enumerate(c["entries"]) if e.get("type") == gc.COMMIT][150]
    for roots, exclude in (([c["order"][k_mid]], []), ([c["order"][c["walks"][0][0][0]]], [c["order"][k_mid]])):
        marks, _, _ = m.reachable(roots, exclude)
        want = sorted((p.objects[i]["name"], p.objects[i]["type"], m.model.read([i])[0][1]) for i, v in enumerate(marks) if v)
        pack, idx = p.extract(roots, exclude)
        assert mp.build_index(pack) == idx
        q = mp.Pack(pack, idx)
        got = sorted((o["name"], t, data) for o, (tag, (t, data)) in zip(q.objects, q.read()))
        assert got == want and 0 < len(got) < len(p.objects)
        q.close()
    p.close()
