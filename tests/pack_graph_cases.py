"""The packs of the object-graph tests (md_pack_graph_build, md_pack_reachable), written with tests/pack_writer.py: trees at
the tree kernel's window and lane limits, every mode, every malformed form between two sound trees, commits and tags at
their size limits, edges with every flag, delta chains, damaged streams, and the histories the walks are held to.

A case: name, entries (the writer's), edges (the labels of REQUIRED_EDGES it holds), bad (entries whose status is
INVALID_OBJECT), walks ([(roots, exclude)] as entry numbers), workspace (a "pack_workspace" in MiB that cuts the read
into rounds, or None), exempt (None, or the reason why git rev-list is not held to the case's walks although the rule
asks for it - no MISTYPED edge in the graph, no exclusion in the walk; at most 2 cases may say one)."""
from tests import pack_writer as pw

COMMIT, TREE, BLOB, TAG = 1, 2, 3, 4
WHO = b" a <a@example.org> 1700000000 +0000\n"
REQUIRED_EDGES = {
    "0 entries", "1 entry", "63 entries", "64 entries", "65 entries", "1000 entries", "starts around 256 and 512", "name lengths",
    "NUL at every position of a target", "all-zero target", "space and digit targets", "target ends in a fake entry",
    "every mode", "mode 0", "mode wraps", "mode 100664",
    "empty mode", "8 in the mode", "no space", "empty name", "1 spare byte", "22 spare bytes", "spare fake entry", "name cut to 19", "no NUL",
    "fault in entry 0", "fault in entry 70", "fault in the last entry",
    "0 parents", "1 parent", "2 parents", "17 parents", "commit of 46", "commit of 47", "upper-case hex", "g in the tree line",
    "g in the second parent", "space for the newline", "39-digit parent", "parent at the end", "parent in the message",
    "tag of a commit", "tag of a tree", "tag of a blob", "tag of a tag", "tag of 63", "tag of 64", "tag of 66", "unknown tag type", "no tag line",
    "dir mode names a blob", "file mode names a tree", "commit's tree is a blob", "parent is a tree", "tag says blob of a commit",
    "absent blob", "absent tree", "absent parent",
    "OFS deltas depth 3", "REF deltas depth 3", "base with a bad Adler-32", "tree with a bad stream", "blob with a bad stream", "three rounds",
    "history of 300", "diamond", "200 trees name one subtree", "roots of every type", "exclusions cut a history", "root also excluded",
    "cycle", "empty roots",
}


def absent(k):
    """a name no pack of the tests holds"""
    return pw.hashlib.sha1(b"absent %d" % k).digest()


def entry(mode, name, target):
    return mode + b" " + name + b"\0" + target


def tree(ents):
    return b"".join(entry(*e) for e in ents)


def commit(tree_name, parents=(), message=b"a message\n"):
    return (b"tree " + tree_name.hex().encode() + b"\n" + b"".join(b"parent " + p.hex().encode() + b"\n" for p in parents) +
            b"author" + WHO + b"committer" + WHO + b"\n" + message)


def tag(target, type_name, label=b"v1"):
    return b"object " + target.hex().encode() + b"\ntype " + type_name + b"\ntag " + label + b"\ntagger" + WHO + b"\nmessage\n"


class Pack:
    """the entries of one pack; add() -> (entry number, the object's name)"""

    def __init__(self):
        self.entries = []

    def add(self, type_, data, **knobs):
        self.entries.append(dict({"type": type_, "data": data}, **knobs))
        return len(self.entries) - 1, knobs.get("name") or pw.object_name(type_, data)

    def blob(self, data, **knobs):
        return self.add(BLOB, data, **knobs)[1]


def _case(name, pack, edges, bad=(), walks=(), workspace=None, exempt=None):
    return {"name": name, "entries": pack.entries, "edges": set(edges), "bad": set(bad), "walks": list(walks),
            "workspace": workspace, "exempt": exempt}


def _tree_shapes():
    p = Pack()
    b = p.blob(b"a blob\n")
    for n in (0, 1, 63, 64, 65, 1000):
        p.add(TREE, tree([(b"100644", b"%c" % (33 + k % 90) if n <= 90 else b"f%d" % k, b if k % 3 else absent(k)) for k in range(n)]))
    # the second entry starts at 255 .. 257 and 511 .. 513, and the first name has every length mod 4 and more
    for start in list(range(29, 70)) + [255, 256, 257, 511, 512, 513, 767, 768, 769]:
        first = entry(b"100644", b"n" * (start - 28), absent(start))
        assert len(first) == start
        p.add(TREE, first + tree([(b"40000", b"d%d" % k, absent(k)) for k in range(12)]))
    for n in [1] + list(range(230, 261)) + [4096]:
        p.add(TREE, tree([(b"100644", b"x", b), (b"100755", b"y" * n, absent(n)), (b"40000", b"z", absent(n + 1))]))
    return _case("tree shapes at the window and lane limits", p,
                 ["0 entries", "1 entry", "63 entries", "64 entries", "65 entries", "1000 entries", "starts around 256 and 512", "name lengths"])


def _tree_targets():
    p = Pack()
    ents = []
    for k in range(20):  # a NUL at every position, between bytes that are none
        t = bytearray(b"\x11" * 20)
        t[k] = 0
        ents.append((b"100644", b"nul%d" % k, bytes(t)))
    ents.append((b"100644", b"zero", bytes(20)))
    ents.append((b"40000", b"digits", b" 01234567 01234567 0"))
    ents.append((b"100644", b"spaces", b" " * 20))
    ents.append((b"100644", b"fake", b"\x01" * 11 + b"40000 ab\0"))
    ents.append((b"100644", b"fake2", b"100644 a\0" + b"\0" * 11))
    ents.append((b"100644", b"last", absent(1)))
    p.add(TREE, tree(ents))
    # and some of those names held by the pack: blobs with forged names
    q = Pack()
    names = [bytes(20), b" 01234567 01234567 0", b"\x01" * 11 + b"40000 ab\0", b"\x11" * 19 + b"\0", b"\0" + b"\x11" * 19]
    for k, nm in enumerate(names):
        q.add(BLOB, b"forged %d\n" % k, name=nm)
    q.add(TREE, tree([(b"100644", b"f%d" % k, nm) for k, nm in enumerate(names)] + [(b"100644", b"gone", absent(2))]))
    return [_case("target names that look like structure", p, ["NUL at every position of a target", "all-zero target", "space and digit targets",
                                                                "target ends in a fake entry"]),
            _case("forged names in the pack", q, ["NUL at every position of a target", "all-zero target"])]


def _modes():
    p = Pack()
    b, t = p.blob(b"mode blob\n"), p.add(TREE, b"")[1]
    ents = [(b"100644", b"a", b), (b"100755", b"b", b), (b"120000", b"c", b), (b"40000", b"d", t), (b"040000", b"e", t),
            (b"160000", b"f", absent(3)), (b"0", b"g", b), (b"7" * 13, b"h", b), (b"100664", b"i", b), (b"00000000000100644", b"j", b)]
    p.add(TREE, tree(ents))
    return _case("every mode", p, ["every mode", "mode 0", "mode wraps", "mode 100664"])


def _malformed_trees():
    p = Pack()
    b = p.blob(b"under the malformed trees\n")
    sound = [(b"100644", b"s%d" % k, b) for k in range(3)]
    good = tree(sound)
    many = [(b"100644", b"m%d" % k, b) for k in range(100)]
    forms = {
        "empty mode": entry(b"", b"x", b),
        "8 in the mode": entry(b"100648", b"x", b),
        "no space": b"100644x\0" + b,
        "empty name": entry(b"100644", b"", b),
        "1 spare byte": good + b"1",
        "22 spare bytes": good + b"1" * 22,
        "spare fake entry": good + entry(b"100644", b"n", b[:19]),
        "name cut to 19": tree(sound[:2]) + entry(b"100644", b"n", b)[:-1],
        "no NUL": b"100644 " + b"n" * 40,
        "fault in entry 0": entry(b"10x644", b"n", b) + good,
        "fault in entry 70": tree(many[:70]) + entry(b"100644", b"", b) + tree(many[70:]),
        "fault in the last entry": tree(many) + entry(b"9", b"n", b),
        "a NUL in the mode": entry(b"100\x00644", b"n", b) + good,
        "a space alone": entry(b" ", b"n", b),
    }
    bad, k = [], 0
    for label, data in forms.items():
        p.add(TREE, tree(sound + [(b"100644", b"before %d" % k, b)]))
        bad.append(p.add(TREE, data)[0])
        k += 1
    p.add(TREE, tree(sound + [(b"100644", b"behind", b)]))
    return _case("malformed trees between sound ones", p, [e for e in forms if e in REQUIRED_EDGES], bad)


def _commits():
    p = Pack()
    t = p.add(TREE, tree([(b"100644", b"f", p.blob(b"of the commits\n"))]))[1]
    th = t.hex().encode()
    c0 = p.add(COMMIT, commit(t))[1]
    c1 = p.add(COMMIT, commit(t, [c0]))[1]
    p.add(COMMIT, commit(t, [c0, c1]))
    p.add(COMMIT, commit(t, [c0, c1] + [absent(100 + k) for k in range(15)]))
    bad = []
    bad.append(p.add(COMMIT, b"tree " + th + b"\n")[0])  # 46 bytes
    p.add(COMMIT, b"tree " + th + b"\n\n")  # 47
    p.add(COMMIT, commit(t, [c0]).replace(th, th.upper()).replace(c0.hex().encode(), c0.hex().upper().encode()))
    bad.append(p.add(COMMIT, commit(t).replace(th, b"g" + th[1:]))[0])
    bad.append(p.add(COMMIT, commit(t, [c0, c1]).replace(c1.hex().encode(), c1.hex().encode()[:-1] + b"g"))[0])
    bad.append(p.add(COMMIT, b"tree " + th + b" author\n\nm\n")[0])
    bad.append(p.add(COMMIT, commit(t, [c0]).replace(b"parent " + c0.hex().encode(), b"parent " + c0.hex().encode()[:-1]))[0])
    bad.append(p.add(COMMIT, b"tree " + th + b"\nparent " + c0.hex().encode()[:-1] + b"\nauthor" + WHO)[0])
    # a parent line at the end: without its newline (no parent from it), with it and nothing behind (malformed), with one byte behind
    line = b"tree " + th + b"\nparent " + c0.hex().encode()
    p.add(COMMIT, line)
    bad.append(p.add(COMMIT, line + b"\n")[0])
    p.add(COMMIT, line + b"\n\n")
    p.add(COMMIT, commit(t, [c0], b"parent " + c1.hex().encode() + b"\nis no parent\n"))
    return _case("commits", p, ["0 parents", "1 parent", "2 parents", "17 parents", "commit of 46", "commit of 47", "upper-case hex",
                                "g in the tree line", "g in the second parent", "space for the newline", "39-digit parent", "parent at the end",
                                "parent in the message", "absent parent"], bad)


def _tags():
    p = Pack()
    b = p.blob(b"of the tags\n")
    t = p.add(TREE, tree([(b"100644", b"f", b)]))[1]
    c = p.add(COMMIT, commit(t))[1]
    k1, t1 = p.add(TAG, tag(c, b"commit"))
    k2, t2 = p.add(TAG, tag(t1, b"tag", b"v2"))
    k3, t3 = p.add(TAG, tag(t2, b"tag", b"v3"))
    kt = p.add(TAG, tag(t, b"tree"))[0]
    kb = p.add(TAG, tag(b, b"blob"))[0]
    head = b"object " + c.hex().encode() + b"\ntype commit\ntag "  # 64 bytes
    assert len(head) == 64
    bad = [p.add(TAG, head[:63])[0], p.add(TAG, head)[0]]
    bad.append(p.add(TAG, b"object " + c.hex().encode() + b"\ntype tag\ntag ab")[0])  # 63 bytes, and all of them sound
    p.add(TAG, b"object " + c.hex().encode() + b"\ntype tag\ntag abc")  # 64: the shortest tag there is (its type says tag: mistyped)
    p.add(TAG, head + b"ab")  # 66
    p.add(TAG, head + b"\n")  # 65: the shortest whose type says commit
    bad.append(p.add(TAG, tag(c, b"commit").replace(b"type commit", b"type bundle"))[0])
    bad.append(p.add(TAG, b"object " + c.hex().encode() + b"\ntype commit\ntagger" + WHO + b"\nmessage\n")[0])
    bad.append(p.add(TAG, tag(c, b"commit").replace(b"object ", b"objekt "))[0])
    p.add(TAG, tag(c, b"blob", b"wrong"))
    p.add(TAG, tag(absent(7), b"commit", b"gone"))
    walks = [([k3], []), ([kt], []), ([kb], []), ([k1, k2], [])]
    return _case("tags", p, ["tag of a commit", "tag of a tree", "tag of a blob", "tag of a tag", "tag of 63", "tag of 64", "tag of 66",
                             "unknown tag type", "no tag line", "tag says blob of a commit"], bad, walks)


def _flags():
    p = Pack()
    b = p.blob(b"of the flags\n")
    t = p.add(TREE, tree([(b"100644", b"f", b)]))[1]
    c = p.add(COMMIT, commit(t))[1]
    k = p.add(TREE, tree([(b"40000", b"dir is a blob", b), (b"100644", b"file is a tree", t), (b"100644", b"gone", absent(11)),
                          (b"40000", b"gone dir", absent(12)), (b"160000", b"sub", c), (b"120000", b"link is a commit", c)]))[0]
    p.add(COMMIT, commit(b))
    p.add(COMMIT, commit(t, [t, absent(13), c]))
    p.add(COMMIT, commit(absent(14)))
    p.add(TAG, tag(c, b"blob"))
    return _case("edges with flags", p, ["dir mode names a blob", "file mode names a tree", "commit's tree is a blob", "parent is a tree",
                                         "tag says blob of a commit", "absent blob", "absent tree", "absent parent"], walks=[([k], [])])


def _deltas(kind):
    p = Pack()
    b = p.blob(b"under the deltas\n")
    ents = [(b"100644", b"file %d" % k, b) for k in range(40)]
    data = [tree(ents[:20 + 5 * d]) for d in range(4)]
    k = p.add(TREE, data[0])[0]
    names = [pw.object_name(TREE, data[0])]
    for d in range(1, 4):
        more = data[d][len(data[d - 1]):]
        ins = [("copy", 0, len(data[d - 1]))] + [("insert", more[a:a + 100]) for a in range(0, len(more), 100)]
        p.entries.append({"delta": kind, "base": k, "ins": ins})
        k = len(p.entries) - 1
        names.append(pw.object_name(TREE, data[d]))
    text = [commit(names[0])]
    for d in range(1, 4):
        text.append(commit(names[d], [pw.object_name(COMMIT, text[d - 1])]))
    k = p.add(COMMIT, text[0])[0]
    for d in range(1, 4):
        head = b"tree " + names[d].hex().encode() + b"\nparent " + pw.object_name(COMMIT, text[d - 1]).hex().encode() + b"\n"
        at = len(b"tree " + names[d - 1].hex().encode() + b"\n") + (48 if d > 1 else 0)
        p.entries.append({"delta": kind, "base": k, "ins": [("insert", head[:100]), ("insert", head[100:])][:1 + (len(head) > 100)] +
                          [("copy", at, len(text[d - 1]) - at)]})
        k = len(p.entries) - 1
    return _case("trees and commits as %s deltas" % kind.upper(), p, ["%s deltas depth 3" % kind.upper()], walks=[([k], [])])


def _damage():
    p = Pack()
    b = p.blob(b"under the damage\n")
    base = tree([(b"100644", b"f%d" % k, b) for k in range(10)])
    k0 = p.add(TREE, base, bad_adler=True)[0]
    p.entries.append({"delta": "ofs", "base": k0, "ins": [("copy", 0, len(base)), ("insert", entry(b"100644", b"more", b))]})
    p.add(TREE, tree([(b"100644", b"sized wrong", b)]), hsize=45)
    p.add(TREE, tree([(b"100644", b"sound", b)]))
    p.add(BLOB, b"a blob whose stream is damaged\n", bad_adler=True)
    p.add(COMMIT, commit(pw.object_name(TREE, tree([(b"100644", b"sound", b)]))))
    return _case("damaged streams", p, ["base with a bad Adler-32", "tree with a bad stream", "blob with a bad stream"])


def history(commits=300):
    """a linear history over trees nested 4 deep, most subtrees shared between commits -> (pack, entry numbers of the commits)"""
    p = Pack()
    blobs = [p.blob(b"blob %d\n" % k) for k in range(12)]
    made = {}

    def add_tree(ents):
        data = tree(ents)
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


def _reach():
    out = []
    p, cs = history()
    out.append(_case("a linear history of 300", p, ["history of 300", "exclusions cut a history", "root also excluded", "empty roots"],
                     walks=[([cs[-1]], []), ([cs[150]], []), ([cs[-1]], [cs[150]]), ([cs[10], cs[20]], [cs[20]]), ([cs[5]], [cs[5]]), ([], []),
                            ([], [cs[3]])]))
    p = Pack()
    b = [p.blob(b"diamond %d\n" % k) for k in range(4)]
    t = [p.add(TREE, tree([(b"100644", b"f", x)]))[1] for x in b]
    c0 = p.add(COMMIT, commit(t[0]))[1]
    c1 = p.add(COMMIT, commit(t[1], [c0]))[1]
    c2 = p.add(COMMIT, commit(t[2], [c0]))[1]
    km = p.add(COMMIT, commit(t[3], [c1, c2]))[0]
    out.append(_case("a diamond merge", p, ["diamond"], walks=[([km], []), ([km], [2 * 4 + 1])]))
    p = Pack()
    leaf = p.add(TREE, tree([(b"100644", b"f%d" % k, p.blob(b"shared %d\n" % k)) for k in range(70)]))[1]
    tops = [p.add(TREE, tree([(b"40000", b"same", leaf), (b"40000", b"again", leaf), (b"100644", b"own", absent(300 + k))]))[1] for k in range(200)]
    ktop = p.add(TREE, tree([(b"40000", b"t%d" % k, x) for k, x in enumerate(tops)]))[0]
    out.append(_case("200 trees name one subtree", p, ["200 trees name one subtree"], walks=[([ktop], []), (list(range(71, 271)), [])]))
    def sound_roots():  # a blob, a tree of it, a commit of that, a tag of that: entries 0 .. 3
        p = Pack()
        b = p.blob(b"a root blob\n")
        c = p.add(COMMIT, commit(p.add(TREE, tree([(b"100644", b"f", b)]))[1]))[1]
        p.add(TAG, tag(c, b"commit"))
        return p, b

    kb, kt, kg = 0, 1, 3
    p, b = sound_roots()
    out.append(_case("roots that are a tree, a blob and a tag", p, ["roots of every type"], walks=[([kt, kb, kg], []), ([kb], []), ([kg], []), ([kt], [])]))
    p, b = sound_roots()
    kbad = p.add(TREE, entry(b"", b"x", b))[0]
    out.append(_case("a root that is a malformed tree", p, ["roots of every type"], bad=[kbad], walks=[([kt, kb, kg, kbad], []), ([kbad], [])],
                     exempt="git rev-list dies on a root it cannot parse; here a malformed object is marked and has no edges"))
    p = Pack()
    b = p.blob(b"on the cycle\n")
    own = pw.hashlib.sha1(b"a tree that names itself").digest()
    other = pw.hashlib.sha1(b"and one that names it back").digest()
    k1 = p.add(TREE, tree([(b"40000", b"me", own), (b"40000", b"you", other), (b"100644", b"f", b)]), name=own)[0]
    p.add(TREE, tree([(b"40000", b"back", own)]), name=other)
    out.append(_case("a forged-name cycle", p, ["cycle"], walks=[([k1], [])],
                     exempt="a cycle needs names that are no SHA-1 of their object, and git refuses such a tree: hash mismatch"))
    return out


def _rounds():
    """a workspace of 0 puts one selected object and its chain of bases in a round: the history in many rounds, and the
    delta chains with every base decoded - and parsed - again in the rounds of what hangs off it"""
    p, cs = history(40)
    out = [_case("the history at a workspace of three rounds and more", p, ["three rounds"], walks=[([cs[-1]], [])], workspace=0)]
    for kind in ("ofs", "ref"):
        c = _deltas(kind)
        out.append(dict(c, name=c["name"] + ", a chain a round", edges={"three rounds"}, workspace=0))
    return out


def cases():
    return ([_tree_shapes()] + _tree_targets() + [_modes(), _malformed_trees(), _commits(), _tags(), _flags(), _deltas("ofs"), _deltas("ref"),
                                                   _damage()] + _reach() + _rounds())


_BUILT = {}


def build(c):
    """-> the case with pack, idx, layout and order (entry number -> index in the idx); built once"""
    if c["name"] not in _BUILT:
        pack, idx, layout = pw.write_pack(c["entries"])
        _BUILT[c["name"]] = dict(c, pack=pack, idx=idx, layout=layout, order=pw.idx_order(layout))
    return _BUILT[c["name"]]
