"""The yardstick of the object-graph tests against git itself, on the CPU: what tests/pack_graph_model.py reads out of the
packs of tests/pack_graph_cases.py is what git reads - the entries of every well-formed tree, a refusal for every malformed
tree, commit and tag, the object set of `git rev-list --objects --missing=print` for the walks - and the list of cases
holds every edge it is meant to hold.  Needs git (skipped where there is none); no device."""
import pytest

from tests import pack_graph_cases as gc
from tests import pack_graph_model as gm
from tests import pack_model as pm
from tests import pack_writer as pw
from tests.test_pack_model import _git, _repo_with, needs_git


@pytest.fixture(scope="module")
def built():
    return [(gc.build(c), gm.Graph(gc.build(c)["pack"], gc.build(c)["idx"])) for c in gc.cases()]


def _ls_tree(repo, name):
    """git ls-tree -> (exit status, [the entries' 20-byte names])"""
    r = _git(repo, "ls-tree", "-z", name.hex())
    names = [bytes.fromhex(rec.split(b"\t")[0].split(b" ")[2].decode()) for rec in r.stdout.split(b"\0") if rec]
    return r.returncode, names


@needs_git
def test_trees_commits_and_tags_as_git_reads_them(built, tmp_path):
    trees = refused = 0
    for c, g in built:
        repo, _ = _repo_with(str(tmp_path), c["pack"], c["idx"])
        objs = g.model.objects
        by_name = {o["name"]: i for i, o in enumerate(objs)}
        data = dict(enumerate(g.model.read()))
        for i, o in enumerate(objs):
            if data[i][0] == pm.OK and pw.object_name(o["type"], data[i][1]) != o["name"]:
                continue  # (a forged name: git hashes a tree, a commit and a tag that it parses)
            if o["type"] == gm.TREE and g.status[i] == pm.OK:
                rc, names = _ls_tree(repo, o["name"])
                want = [objs[t]["name"] if t != gm.NO_LINK else None for t in g.to[g.first[i]:g.first[i + 1]]]
                assert rc == 0 and len(names) == len(want), (c["name"], i)
                for got, w, k in zip(names, want, g.kind[g.first[i]:g.first[i + 1]]):
                    assert (got == w) if w is not None else (k & gm.ABSENT or k & 0x3f == gm.TREE_GITLINK) and (got not in by_name or k & 0x3f == gm.TREE_GITLINK), (c["name"], i)
                trees += 1
            elif g.status[i] == gm.INVALID_OBJECT:
                r = _git(repo, "ls-tree", o["name"].hex()) if o["type"] == gm.TREE else _git(repo, "rev-list", "--objects", o["name"].hex())
                assert r.returncode != 0, (c["name"], i, o["type"])
                refused += 1
        assert {c["order"][k] for k in c["bad"]} == {i for i, st in enumerate(g.status) if st == gm.INVALID_OBJECT}, c["name"]
    assert trees >= 100 and refused >= 25


@needs_git
def test_walks_as_git_rev_list_walks_them(built, tmp_path):
    """every walk of every case that the rule covers - no MISTYPED edge in the graph, no exclusion, a root at all -, but for
    the cases that say why they are exempt: the objects rev-list lists are the marked ones, and the names on its `?` lines
    are the names of the ABSENT edges of the marked objects"""
    exempt = [c["name"] for c, _ in built if c["exempt"]]
    assert len(exempt) <= 2 and all(len(c["exempt"]) > 20 for c, _ in built if c["exempt"])
    seen = with_missing = 0
    for c, g in built:
        if c["exempt"] or g.info["mistyped"]:
            continue
        repo, _ = _repo_with(str(tmp_path), c["pack"], c["idx"])
        objs = g.model.objects
        for roots, exclude in c["walks"]:
            if exclude or not roots:
                continue
            marks, _, _ = g.reachable([c["order"][k] for k in roots])
            r = _git(repo, "rev-list", "--objects", "--missing=print", *[objs[c["order"][k]]["name"].hex() for k in roots])
            assert r.returncode == 0, (c["name"], r.stderr)
            lines = [w.split(b" ")[0] for w in r.stdout.split(b"\n") if w]
            got = {bytes.fromhex(w.decode()) for w in lines if not w.startswith(b"?")}
            missing = {bytes.fromhex(w[1:].decode()) for w in lines if w.startswith(b"?")}
            assert got == {objs[i]["name"] for i, m in enumerate(marks) if m}, c["name"]
            met = {nm for i, m in enumerate(marks) if m for (_, k), nm in zip(g.edges[i], g.names[i]) if k & gm.ABSENT}
            assert missing == met, c["name"]
            seen += 1
            with_missing += bool(met)
    assert seen >= 12 and with_missing >= 2


def test_the_model_reads_every_case_as_the_case_says(built):
    for c, g in built:
        bad = {c["order"][k] for k in c["bad"]}
        assert bad == {i for i, st in enumerate(g.status) if st == gm.INVALID_OBJECT}, c["name"]
        for i in range(g.info["n"]):
            if g.status[i] != pm.OK or g.model.objects[i]["type"] == gm.BLOB:
                assert g.first[i] == g.first[i + 1], (c["name"], i)
        for roots, exclude in c["walks"]:
            marks, expanded, rounds = g.reachable([c["order"][k] for k in roots], [c["order"][k] for k in exclude])
            assert exclude or all(marks[c["order"][k]] for k in roots), c["name"]
            assert not any(marks[c["order"][k]] for k in exclude), c["name"]


def test_the_cases_hold_every_edge():
    cases = gc.cases()
    assert len({c["name"] for c in cases}) == len(cases)
    held = set().union(*[c["edges"] for c in cases])
    assert gc.REQUIRED_EDGES <= held, gc.REQUIRED_EDGES - held
    b = {c["name"]: (gc.build(c), gm.Graph(gc.build(c)["pack"], gc.build(c)["idx"])) for c in cases}
    # edges the bytes themselves show
    c, g = b["tree shapes at the window and lane limits"]
    degrees = {g.first[i + 1] - g.first[i] for i in range(g.info["n"])}
    assert {0, 1, 63, 64, 65, 1000} <= degrees
    sizes = {o["size"] for o in g.model.objects if o["type"] == gm.TREE}
    assert any(s > 4096 + 60 for s in sizes)
    c, g = b["every mode"]
    kinds = [k & 0x3f for k in g.kind]
    assert kinds.count(gm.TREE_GITLINK) == 3 and kinds.count(gm.TREE_TREE) == 2 and kinds.count(gm.TREE_BLOB) == 5 and not g.info["mistyped"]
    c, g = b["commits"]
    assert 18 in {g.first[i + 1] - g.first[i] for i in range(g.info["n"])} and g.info["absent"] == 15
    c, g = b["edges with flags"]
    assert g.info["mistyped"] == 6 and g.info["absent"] == 4
    for kind in ("OFS", "REF"):
        c, g = b["trees and commits as %s deltas" % kind]
        assert g.model.info["max_depth"] == 3 and g.model.info["deltas"] == 6 and g.info["failed"] == 0 and g.info["absent"] == 0
    c, g = b["damaged streams"]
    assert sorted(st for st in g.status if st) == [pm.INVALID_CHECKSUM, pm.INVALID_SIZE, pm.INVALID_PACK_BASE]
    assert g.info["parsed"] == 5 and g.info["failed"] == 3 and g.info["n"] == 7
    c, g = b["a linear history of 300"]
    top = c["order"][c["walks"][0][0][0]]
    marks, expanded, rounds = g.reachable([top])
    assert g.tree_depth(top) == 4 and rounds == 4 + 2 and sum(marks) == g.info["n"] and g.stats["host_closed"] == 300
    c, g = b["200 trees name one subtree"]
    marks, expanded, rounds = g.reachable([c["order"][k] for k in c["walks"][1][0]])
    assert expanded == 201 and rounds == 2
    c, g = b["a forged-name cycle"]
    assert g.reachable([c["order"][c["walks"][0][0][0]]])[0] == [1, 1, 1]
