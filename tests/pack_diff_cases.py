"""The packs and pairs of the tree-diff tests (md_pack_diff), built with the helpers of tests/pack_graph_cases.py: trees at the
diff kernel's lane stride and the table kernel's window limits, every order of the keys git's rule tells apart, every mode
change, shared and unreadable subtrees, delta-stored trees and a history.

A case: name, entries (the writer's), pairs ([(a, b)] as entry numbers, None = the empty tree), want (per pair the claim the
case makes about the model's output: the sorted list of "K path" - K the kind, the path ending in "/" for a directory's
own record and in "/!" for an opaque one -, or the status number of a pair that is refused), stats (claims about the
model's info: key -> value), exempt (None, or why git diff-tree is not held to the case), workspace (a "pack_workspace" in
MiB for the GPU run, or None), edges (the labels of REQUIRED_EDGES it holds)."""
from tests import pack_graph_cases as gc
from tests.pack_graph_cases import COMMIT, TREE, absent, commit, entry, history, tree

INVALID_OBJECT = 27
REQUIRED_EDGES = {
    "0 1 63 64 65 129 entries on either side", "one change first, last, at row 63, at row 64", "name ends at 255 and 256", "name of 256 and more",
    "fo foo foo.d foo/ foo0 in every combination", "file to directory with a neighbour between", "foo as file and as directory",
    "100664 is 100644", "644 to 755 is M", "file to symlink is T", "file to gitlink is T", "mode 0 and a wrapped mode are gitlinks",
    "same subtree is not read", "NONE against 3 deep", "3 deep against NONE", "A == B", "both NONE", "200 pairs share one tree",
    "absent subtree", "subtree is a blob", "malformed subtree", "unsorted subtree", "doubled key", "refused at level 0",
    "OFS deltas", "REF deltas", "history of 300",
}


def _key(e):
    mode, name, _ = e
    return name + b"/" if int(mode, 8) & 0o170000 == 0o040000 else name


def stree(ents):
    """a tree of the entries in git's order"""
    return tree(sorted(ents, key=_key))


def _case(name, pack, pairs, want, edges, stats=None, exempt=None, workspace=None, commits=False):
    return {"name": name, "entries": pack.entries, "pairs": list(pairs), "want": list(want), "edges": set(edges), "stats": stats or {},
            "exempt": exempt, "workspace": workspace, "commits": commits}


def _sizes():
    p = gc.Pack()
    b = p.blob(b"of the sizes\n")
    sizes = (0, 1, 63, 64, 65, 129)
    k = {n: p.add(TREE, tree([(b"100644", b"e%03d" % i, b) for i in range(n)]))[0] for n in sizes}
    pairs, want = [], []
    for na in sizes:
        for nb in sizes:
            pairs.append((k[na], k[nb]))
            want.append(sorted(["D e%03d" % i for i in range(nb, na)] + ["A e%03d" % i for i in range(na, nb)]))
        pairs += [(None, k[na]), (k[na], None)]
        want += [sorted("A e%03d" % i for i in range(na)), sorted("D e%03d" % i for i in range(na))]
    return _case("trees of 0 .. 129 entries on either side", p, pairs, want, ["0 1 63 64 65 129 entries on either side"])


def _one_change():
    p = gc.Pack()
    b, c = p.blob(b"before\n"), p.blob(b"after\n")
    base = [(b"100644", b"e%03d" % i, b) for i in range(129)]
    k0 = p.add(TREE, tree(base))[0]
    pairs, want = [], []
    for at in (0, 63, 64, 128):
        k = p.add(TREE, tree(base[:at] + [(b"100644", b"e%03d" % at, c)] + base[at + 1:]))[0]
        pairs += [(k0, k), (k, k0)]
        want += [["M e%03d" % at]] * 2
    return _case("one changed entry of 129", p, pairs, want, ["one change first, last, at row 63, at row 64"])


def _windows():
    p = gc.Pack()
    b, c = p.blob(b"in the window\n"), p.blob(b"changed in the window\n")
    pairs, want = [], []
    for nul in (254, 255, 256, 257, 511, 512):  # the second entry's NUL stands at this byte of the tree
        first = b"a" * (nul - 28 - 7 - 2)
        second = b"zz"
        ents = [(b"100644", first, b), (b"100644", second, b), (b"100644", b"zzz", b)]
        assert tree(ents).index(b"\0", len(entry(*ents[0]))) == nul
        ka = p.add(TREE, tree(ents))[0]
        kb = p.add(TREE, tree([ents[0], (b"100644", second, c), ents[2]]))[0]
        pairs.append((ka, kb))
        want.append(["M zz"])
    for n in (255, 256, 257, 300, 1000):  # and names as long as a window and longer, told apart in their last byte
        x, y = b"n" * (n - 1) + b"x", b"n" * (n - 1) + b"y"
        ka = p.add(TREE, tree([(b"100644", b"a", b), (b"100644", x, b)]))[0]
        kb = p.add(TREE, tree([(b"100644", b"a", b), (b"100644", x, c), (b"100644", y, b)]))[0]
        pairs.append((ka, kb))
        want.append(sorted(["M " + x.decode(), "A " + y.decode()]))
    return _case("names at the window's end and longer than a window", p, pairs, want, ["name ends at 255 and 256", "name of 256 and more"])


def _key_order():
    p = gc.Pack()
    f = p.blob(b"a file of the keys\n")
    sub = p.add(TREE, tree([(b"100644", b"x", f)]))[1]
    names = [b"fo", b"foo", b"foo.d", b"foo0"]
    ks = []
    for bits in range(16):  # name k is a directory iff bit k is set
        ks.append(p.add(TREE, stree([(b"40000", nm, sub) if bits >> k & 1 else (b"100644", nm, f) for k, nm in enumerate(names)]))[0])
    pairs, want = [], []
    for i in range(16):
        for j in (0, 15, (i + 1) % 16, (i + 5) % 16):
            pairs.append((ks[i], ks[j]))
            w = []
            for k, nm in enumerate(names):
                da, db, s = i >> k & 1, j >> k & 1, nm.decode()
                if da != db:
                    w += ["D %s/" % s, "D %s/x" % s, "A " + s] if da else ["D " + s, "A %s/" % s, "A %s/x" % s]
            want.append(sorted(w))
    both = p.add(TREE, stree([(b"100644", b"foo", f), (b"40000", b"foo", sub), (b"100644", b"foo.d", f)]))[0]
    only_file = p.add(TREE, stree([(b"100644", b"foo", f), (b"100644", b"foo.d", f)]))[0]
    only_dir = p.add(TREE, stree([(b"40000", b"foo", sub), (b"100644", b"foo.d", f)]))[0]
    out = [_case("fo, foo, foo.d, foo/ and foo0 as files and directories", p, pairs, want, ["fo foo foo.d foo/ foo0 in every combination"])]
    out.append(_case("a file becomes a directory", p, [(only_file, only_dir), (only_dir, only_file)],
                     [["A foo/", "A foo/x", "D foo"], ["A foo", "D foo/", "D foo/x"]], ["file to directory with a neighbour between"]))
    out.append(_case("one name as file and as directory in one tree", p, [(both, only_file), (only_dir, both), (both, both)],
                     [["D foo/", "D foo/x"], ["A foo"], []], ["foo as file and as directory"]))
    return out


def _modes():
    p = gc.Pack()
    f, c = p.blob(b"a file of the modes\n"), p.add(COMMIT, commit(absent(1)))[1]
    k = {m: p.add(TREE, tree([(b"100644", b"a", f), (m, b"m", f), (b"100644", b"z", f)]))[0]
         for m in (b"100644", b"100664", b"100755", b"120000", b"160000", b"0", b"7" * 13, b"100600")}
    pairs = [(k[b"100644"], k[b"100664"]), (k[b"100664"], k[b"100600"]), (k[b"100644"], k[b"100755"]), (k[b"100755"], k[b"100644"]),
             (k[b"100644"], k[b"120000"]), (k[b"100644"], k[b"160000"]), (k[b"120000"], k[b"160000"]), (k[b"160000"], k[b"0"]),
             (k[b"0"], k[b"7" * 13]), (k[b"100644"], k[b"0"])]
    want = [[], [], ["M m"], ["M m"], ["T m"], ["T m"], ["T m"], [], [], ["T m"]]
    return _case("every change of mode", p, pairs, want, ["100664 is 100644", "644 to 755 is M", "file to symlink is T", "file to gitlink is T",
                                                          "mode 0 and a wrapped mode are gitlinks"])


def _nesting():
    p = gc.Pack()
    f, g = p.blob(b"nested\n"), p.blob(b"nested, changed\n")
    d3 = p.add(TREE, tree([(b"100644", b"leaf", f)]))[1]
    d2 = p.add(TREE, stree([(b"40000", b"c", d3), (b"100644", b"f2", f)]))[1]
    d1 = p.add(TREE, stree([(b"40000", b"b", d2), (b"100644", b"f1", f)]))[1]
    top = p.add(TREE, stree([(b"40000", b"a", d1), (b"100644", b"f0", f)]))[0]
    all_of = ["a/", "a/b/", "a/b/c/", "a/b/c/leaf", "a/b/f2", "a/f1", "f0"]
    same = p.add(TREE, stree([(b"40000", b"a", d1), (b"100644", b"f0", g)]))[0]
    out = [_case("the empty tree against trees nested 3 deep", p, [(None, top), (top, None), (top, top), (None, None), (top, same)],
                 [sorted("A " + x for x in all_of), sorted("D " + x for x in all_of), [], [], ["M f0"]],
                 ["NONE against 3 deep", "3 deep against NONE", "A == B", "both NONE", "same subtree is not read"],
                 stats={"trees_read": 2 + 1 + 1 + 1, "levels": 4, "launches": 20})]  # (the pairs advance together: top and same, then a, b, c)
    # one pair alone: its counts are the claim
    out.append(_case("a subtree both sides share", p, [(top, same)], [["M f0"]], ["same subtree is not read"], stats={"trees_read": 2, "levels": 1, "launches": 5}))
    q = gc.Pack()
    f, g = q.blob(b"shared\n"), q.blob(b"shared, changed\n")
    sa = q.add(TREE, tree([(b"100644", b"x", f)]))[1]
    sb = q.add(TREE, tree([(b"100644", b"x", g)]))[1]
    ka = q.add(TREE, stree([(b"40000", b"d", sa), (b"100644", b"f", f)]))[0]
    kb = q.add(TREE, stree([(b"40000", b"d", sb), (b"100644", b"f", f)]))[0]
    out.append(_case("200 pairs that share their trees", q, [(ka, kb)] * 200, [["M d/", "M d/x"]] * 200, ["200 pairs share one tree"],
                     stats={"trees_read": 4, "levels": 2, "launches": 10, "changes": 400}))
    out.append(_case("the same two trees as one pair", q, [(ka, kb)], [["M d/", "M d/x"]], ["200 pairs share one tree"],
                     stats={"trees_read": 4, "levels": 2, "launches": 10, "changes": 2}))
    return out


def _unreadable():
    p = gc.Pack()
    f, g = p.blob(b"under the unreadable\n"), p.blob(b"under the unreadable, changed\n")
    good = p.add(TREE, tree([(b"100644", b"x", f)]))[1]
    forms = {  # label -> (entry number or None, the name a directory entry holds)
        "absent subtree": (None, absent(40)),
        "subtree is a blob": (0, f),
        "malformed subtree": p.add(TREE, entry(b"100648", b"x", f)),
        "unsorted subtree": p.add(TREE, tree([(b"100644", b"b", f), (b"100644", b"a", f)])),
        "doubled key": p.add(TREE, tree([(b"100644", b"a", f), (b"100644", b"a", g)])),
    }
    pairs, want = [], []
    base = p.add(TREE, stree([(b"40000", b"d", good), (b"100644", b"f", f)]))[0]
    for label, (_, name) in forms.items():
        k = p.add(TREE, stree([(b"40000", b"d", name), (b"100644", b"f", g)]))[0]
        pairs += [(base, k), (k, base), (None, k), (k, None)]
        want += [["M d/!", "M f"], ["M d/!", "M f"], ["A d/!", "A f"], ["D d/!", "D f"]]
    for label, (k, _) in forms.items():  # the same objects as sides of a pair of the call
        if k is not None:
            pairs += [(k, base), (base, k), (None, k), (k, k)]
            want += [INVALID_OBJECT] * 3 + [[]]
    return _case("subtrees that cannot be read", p, pairs, want, list(forms) + ["refused at level 0"],
                 exempt="git diff-tree dies on a tree it cannot read or that the pack lacks; here the directory's record is opaque")


def _deltas(kind):
    """four trees, each the one before and five entries more, stored as a chain of deltas (as pack_graph_cases' are, with names in order)"""
    p = gc.Pack()
    b = p.blob(b"under the deltas\n")
    ents = [(b"100644", b"file %02d" % k, b) for k in range(40)]
    data = [tree(ents[:20 + 5 * d]) for d in range(4)]
    k = p.add(TREE, data[0])[0]
    ks = [k]
    for d in range(1, 4):
        more = data[d][len(data[d - 1]):]
        p.entries.append({"delta": kind, "base": k, "ins": [("copy", 0, len(data[d - 1]))] + [("insert", more[a:a + 100]) for a in range(0, len(more), 100)]})
        k = len(p.entries) - 1
        ks.append(k)
    files = lambda lo, hi: ["file %02d" % k for k in range(lo, hi)]
    pairs = [(ks[0], ks[1]), (ks[1], ks[2]), (ks[2], ks[3]), (ks[0], ks[3]), (ks[3], ks[1])]
    want = [sorted("A " + x for x in files(20, 25)), sorted("A " + x for x in files(25, 30)), sorted("A " + x for x in files(30, 35)),
            sorted("A " + x for x in files(20, 35)), sorted("D " + x for x in files(25, 35))]
    return _case("trees stored as %s deltas" % kind.upper(), p, pairs, want, ["%s deltas" % kind.upper()])


def sorted_history(commits=300):
    """pack_graph_cases' history with every tree in git's order: a linear history over trees nested 4 deep, most subtrees shared
    between commits -> (pack, entry numbers of the commits)"""
    p = gc.Pack()
    blobs = [p.blob(b"blob %d\n" % k) for k in range(12)]
    made = {}

    def add_tree(ents):
        data = stree(ents)
        if data not in made:
            made[data] = p.add(TREE, data)[1]
        return made[data]

    def nested(depth, salt):
        ents = [(b"100644", b"file%d" % k, blobs[(salt + k) % len(blobs)]) for k in range(2)]
        if depth:
            ents.append((b"40000", b"sub", nested(depth - 1, salt)))
        return add_tree(ents)

    parents, cs = [], []
    for c in range(commits):
        root = add_tree([(b"40000", b"lib", nested(3, c % 5)), (b"40000", b"src", nested(3, c % 3)), (b"100644", b"README", blobs[c % 12]),
                         (b"100644", b"version", p.blob(b"version %d\n" % c))])
        k, name = p.add(COMMIT, commit(root, parents, b"commit %d\n" % c))
        parents = [name]
        cs.append(k)
    return p, cs


def _history():
    """changes() over two histories of 300: pack_graph_cases' own, whose root trees hold README behind lib and src - not git's
    order, so every pair is refused -, and the same history with its trees in order"""
    p, _ = history()
    q, _ = sorted_history()
    return [_case("the unsorted history of 300 through changes()", p, [], [], ["history of 300"], stats={"failed": 300, "changes": 0}, commits=True,
                  exempt="git diff-tree walks a tree that is out of order as it lies; here it is refused"),
            _case("the history of 300 through changes()", q, [], [], ["history of 300"], stats={"failed": 0, "levels": 5}, commits=True)]


def cases():
    out = [_sizes(), _one_change(), _windows()] + _key_order() + [_modes()] + _nesting() + [_unreadable(), _deltas("ofs"), _deltas("ref")] + _history()
    for c in (out[0], _nesting()[0], _deltas("ofs")):
        out.append(dict(c, name=c["name"] + ", a tree a round", workspace=0))
    return out


_BUILT = {}


def build(c):
    """-> the case with pack, idx, layout, order (entry number -> index in the idx) and ipairs (the pairs as indices); built once"""
    key = c["name"].split(", a tree a round")[0]
    if key not in _BUILT:
        pack, idx, layout = gc.pw.write_pack(c["entries"])
        _BUILT[key] = dict(pack=pack, idx=idx, layout=layout, order=gc.pw.idx_order(layout))
    b = dict(c, **_BUILT[key])
    b["ipairs"] = [tuple(None if x is None else b["order"][x] for x in pr) for pr in c["pairs"]]
    return b
