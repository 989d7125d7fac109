"""The yardstick of the tree-diff tests against git itself, on the CPU: what tests/pack_diff_model.py makes of the pairs of
tests/pack_diff_cases.py is what every case claims, and - for every case the rule covers: all trees sound and sorted, no
doubled key, no opaque record - what `git diff-tree` prints: the records without the TREE flag are the lines of `-r`, all
records those of `-r -t`, the top level alone those of the command without -r, compared as sorted sets.  Needs git for that
(skipped where there is none); no device."""
import pytest

from tests import pack_diff_cases as dc
from tests import pack_diff_model as dm
from tests import pack_graph_model as gm
from tests import pack_model as pm
from tests.test_pack_model import _git, _repo_with, needs_git

EMPTY_TREE = "4b825dc642cb6eb9a060e54bf8d69288fbee4904"


@pytest.fixture(scope="module")
def built():
    """every case built once with the model's graph: [(case, graph model)]"""
    out = []
    for c in dc.cases():
        b = dc.build(c)
        out.append((b, gm.Graph(b["pack"], b["idx"])))
    return out


def claims(d):
    """a model's output as the cases state it: per pair the sorted "K path" list, or the status"""
    out = [[] for _ in d.status]
    for c, path in zip(d.records, d.paths()):
        out[c["pair"]].append("%s %s%s%s" % (c["kind"], path.decode(), "/" if c["flags"] & dm.TREE else "", "!" if c["flags"] & dm.OPAQUE else ""))
    return [sorted(o) if st == pm.OK else st for o, st in zip(out, d.status)]


def pairs_of(c, g):
    return dm.commit_pairs(g)[1] if c["commits"] else c["ipairs"]


def test_the_model_gives_what_every_case_claims(built):
    for c, g in built:
        d = dm.Diff(g, pairs_of(c, g))
        if not c["commits"]:
            assert claims(d) == c["want"], c["name"]
        for key, value in c["stats"].items():
            assert d.info[key] == value, (c["name"], key, d.info)
        # what holds of every output
        assert all(r["parent"] is None or r["parent"] < k for k, r in enumerate(d.records)), c["name"]
        at = 0
        for r in d.records:
            assert r["name_off"] == at, c["name"]
            at += r["name_len"]
        assert at == len(d.names) == d.info["name_bytes"]
        top = dm.Diff(g, pairs_of(c, g), recursive=False)
        assert top.records == [dict(r, flags=r["flags"] & ~dm.OPAQUE) for r in d.records if r["parent"] is None], c["name"]
        assert top.info["levels"] <= 1 and top.info["opaque"] == 0


def test_the_cases_hold_every_edge(built):
    cases = dc.cases()
    assert len({c["name"] for c in cases}) == len(cases)
    held = set().union(*[c["edges"] for c in cases])
    assert dc.REQUIRED_EDGES <= held, dc.REQUIRED_EDGES - held
    assert sum(bool(c["exempt"]) for c in cases) <= 4 and all(len(c["exempt"]) > 20 for c in cases if c["exempt"])
    # the model's tree rules are the graph model's
    for c, g in built[:12]:
        for i, (st, data) in enumerate(g.model.read()):
            if st == pm.OK and g.model.objects[i]["type"] == gm.TREE:
                assert (dm.entries(data) is None) == (gm.parse_tree(data) is None)
    assert [dm.canon(m) for m in (0o100664, 0o100600, 0o100755, 0o100700, 0o120777, 0o40755, 0, 0o160000, 0xFFFFFFFF)] == \
        [0o100644, 0o100644, 0o100755, 0o100755, 0o120000, 0o40000, 0o160000, 0o160000, 0o160000]


def _git_lines(repo, a, b, *flags):
    r = _git(repo, "diff-tree", *flags, "--raw", "--no-renames", "--no-abbrev", "-z", a, b)
    assert r.returncode == 0, r.stderr
    f, out = r.stdout.split(b"\0"), []
    for k in range(0, len(f) - 1, 2):  # ":<mode> <mode> <name> <name> <kind>", then the path
        a_mode, b_mode, a_name, b_name, kind = f[k][1:].split(b" ")
        out.append((kind.decode(), int(a_mode, 8), int(b_mode, 8), a_name.decode(), b_name.decode(), f[k + 1]))
    return sorted(out)


def _model_lines(d, q, want_tree=None, top_only=False):
    return sorted((c["kind"], c["a_mode"], c["b_mode"], c["a_name"].hex(), c["b_name"].hex(), path) for c, path in zip(d.records, d.paths())
                  if c["pair"] == q and (want_tree is None or bool(c["flags"] & dm.TREE) == want_tree) and not (top_only and c["parent"] is not None))


@needs_git
def test_the_model_is_git_diff_tree(built, tmp_path):
    seen = lines = 0
    for c, g in built:
        if c["exempt"] or c["workspace"] is not None:
            continue
        repo, _ = _repo_with(str(tmp_path), c["pack"], c["idx"])
        assert _git(repo, "hash-object", "-t", "tree", "-w", "--stdin", input=b"").stdout.decode().strip() == EMPTY_TREE
        pairs = pairs_of(c, g)
        d, top = dm.Diff(g, pairs), dm.Diff(g, pairs, recursive=False)
        assert d.info["opaque"] == 0 and d.info["failed"] == 0, c["name"]  # the rule covers the case
        name = lambda t: EMPTY_TREE if t is None else g.model.objects[t]["name"].hex()
        done = {}
        for q, (a, b) in enumerate(pairs):
            if (a, b) in done:  # (a pair that repeats is held to git once)
                assert _model_lines(d, q) == _model_lines(d, done[(a, b)])
                continue
            done[(a, b)] = q
            assert _model_lines(d, q, want_tree=False) == _git_lines(repo, name(a), name(b), "-r"), (c["name"], q)
            assert _model_lines(d, q) == _git_lines(repo, name(a), name(b), "-r", "-t"), (c["name"], q)
            assert _model_lines(top, q) == _model_lines(d, q, top_only=True) == _git_lines(repo, name(a), name(b)), (c["name"], q)
            lines += len(_model_lines(d, q))
        seen += 1
    assert seen >= 9 and lines > 3000
