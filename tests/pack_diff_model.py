"""md_pack_diff in plain Python, written from the rules include/mdeflate.h states for it: canonical modes, keys and their order,
what makes a tree unreadable for the diff, what a pair of entries gives, the records breadth first, the statuses and the
counts.  The objects' bytes come from the reader of tests/pack_model.py and the entries' targets from the edges of
tests/pack_graph_model.py; nothing is shared with decompress_amd/pack.py or the C++."""
from tests import pack_graph_model as gm
from tests import pack_model as pm

NONE = None  # the empty tree as a side of a pair
TREE, OPAQUE = 1, 2
INVALID_OBJECT = gm.INVALID_OBJECT
DIR = 0o040000
ZERO = bytes(20)


def canon(mode):
    fmt = mode & 0o170000
    if fmt == 0o100000:
        return 0o100755 if mode & 0o100 else 0o100644
    if fmt == 0o120000:
        return 0o120000
    if fmt == 0o040000:
        return DIR
    return 0o160000


def entries(b):
    """a tree's entries -> [(canonical mode, name, the 20 bytes)] or None: the tree rules refuse it"""
    size, s, out = len(b), 0, []
    while size - s != 0:
        if size - s < 23 or b[size - 21] != 0:
            return None
        sp = s
        while 0x30 <= b[sp] <= 0x37:
            sp += 1
        if sp == s or b[sp] != 0x20:
            return None
        mode = 0
        for c in b[s:sp]:
            mode = ((mode << 3) + (c - 0x30)) & 0xFFFFFFFF
        nul = b.index(0, sp + 1)
        if nul == sp + 1 or nul + 21 > size:
            return None
        out.append((canon(mode), b[sp + 1:nul], b[nul + 1:nul + 21]))
        s = nul + 21
    return out


def key(mode, name):
    return name + b"/" if mode == DIR else name


def is_sorted(ents):
    keys = [key(m, nm) for m, nm, _ in ents]
    return all(x < y for x, y in zip(keys, keys[1:]))  # (bytes compare bytewise, a proper prefix first)


def diff_entries(ea, eb):
    """two sorted trees' entries -> [(kind, flags, a's position or None, b's position or None)] in the records' order"""
    at = {(key(m, nm), m == DIR): j for j, (m, nm, _) in enumerate(eb)}
    out, met = [], set()
    for i, (m, nm, sha) in enumerate(ea):
        j = at.get((key(m, nm), m == DIR))
        if j is None:
            out.append(("D", TREE if m == DIR else 0, i, None))
            continue
        met.add(j)
        mb, _, shb = eb[j]
        if m == DIR:
            if sha != shb:
                out.append(("M", TREE, i, j))
        elif m != mb or sha != shb:
            out.append(("T" if (m ^ mb) & 0o170000 else "M", 0, i, j))
    ka = {(key(m, nm), m == DIR) for m, nm, _ in ea}
    for j, (m, nm, _) in enumerate(eb):
        if (key(m, nm), m == DIR) not in ka:
            out.append(("A", TREE if m == DIR else 0, None, j))
    return out


class Diff:
    """md_pack_diff of `pairs` = [(a, b)] (indices in idx order, or None) over the graph model g: records (dicts, in order),
    names (the blob), status (one per pair), info"""

    def __init__(self, g, pairs, recursive=True):
        self.g, m = g, g.model
        n = len(m.objects)
        eligible = lambda o: g.status[o] == pm.OK and m.objects[o]["type"] == gm.TREE
        refusal = lambda o: g.status[o] if g.status[o] != pm.OK else INVALID_OBJECT
        self.status = [pm.OK] * len(pairs)
        self.records, self.names = [], b""
        info = {"pairs": len(pairs), "levels": 0, "trees_read": 0, "launches": 0}
        level = []
        for q, (a, b) in enumerate(pairs):
            assert all(x is None or 0 <= x < n for x in (a, b))
            if a == b:
                continue
            bad = [x for x in (a, b) if x is not None and not eligible(x)]
            if bad:
                self.status[q] = refusal(bad[0])
            else:
                level.append((a, b, q, None))
        while level:
            trees = sorted({x for a, b, _, _ in level for x in (a, b) if x is not None})
            info["levels"] += 1
            info["trees_read"] += len(trees)
            info["launches"] += 4
            table, rstatus = {}, {}
            for t, (st, data) in zip(trees, m.read(trees)):
                rstatus[t] = st
                ents = entries(data) if st == pm.OK else None
                table[t] = ents if ents is not None and is_sorted(ents) else None
            base = len(self.records)
            for a, b, q, parent in level:
                bad = [x for x in (a, b) if x is not None and table[x] is None]
                if bad:
                    if parent is None:
                        self.status[q] = rstatus[bad[0]] if rstatus[bad[0]] != pm.OK else INVALID_OBJECT
                    else:
                        self.records[parent]["flags"] |= OPAQUE
                    continue
                ea, eb = table[a] if a is not None else [], table[b] if b is not None else []
                for kind, flags, i, j in diff_entries(ea, eb):
                    nm = ea[i][1] if i is not None else eb[j][1]
                    self.records.append({
                        "pair": q, "parent": parent, "kind": kind, "flags": flags,
                        "a_mode": ea[i][0] if i is not None else 0, "b_mode": eb[j][0] if j is not None else 0,
                        "a_obj": self._to(a, i), "b_obj": self._to(b, j), "name_len": len(nm), "name_off": len(self.names),
                        "a_name": ea[i][2] if i is not None else ZERO, "b_name": eb[j][2] if j is not None else ZERO})
                    self.names += nm
            info["launches"] += len(self.records) > base
            nxt = []
            for r in range(base, len(self.records)) if recursive else ():
                c = self.records[r]
                if not c["flags"] & TREE:
                    continue
                in_a, in_b = c["kind"] != "A", c["kind"] != "D"
                if (in_a and (c["a_obj"] is None or not eligible(c["a_obj"]))) or (in_b and (c["b_obj"] is None or not eligible(c["b_obj"]))):
                    c["flags"] |= OPAQUE
                    continue
                if in_a and in_b and c["a_obj"] == c["b_obj"]:
                    continue
                nxt.append((c["a_obj"] if in_a else None, c["b_obj"] if in_b else None, c["pair"], r))
            level = nxt
        info.update(changes=len(self.records), name_bytes=len(self.names), opaque=sum(bool(c["flags"] & OPAQUE) for c in self.records),
                    failed=sum(st != pm.OK for st in self.status))
        self.info = info

    def _to(self, tree, pos):
        if tree is None or pos is None:
            return None
        t = self.g.to[self.g.first[tree] + pos]
        return None if t == gm.NO_LINK else t

    def paths(self):
        out = []
        for c in self.records:
            nm = self.names[c["name_off"]:c["name_off"] + c["name_len"]]
            out.append(nm if c["parent"] is None else out[c["parent"]] + b"/" + nm)
        return out

    def per_pair(self):
        """as decompress_amd.pack.Pack.diff returns it, with pm's status numbers for what is not Ok"""
        out, paths = [[] for _ in self.status], self.paths()
        for c, path in zip(self.records, paths):
            out[c["pair"]].append((c["kind"], c["a_mode"], c["b_mode"], c["a_name"], c["b_name"], path, c["flags"]))
        return [("Ok", out[q]) if st == pm.OK else (st, None) for q, st in enumerate(self.status)]


def commit_pairs(g, commits=None):
    """every commit (default: all whose status is Ok, idx order) against its first parent's tree -> (commits, pairs)"""
    objs = g.model.objects
    if commits is None:
        commits = [i for i, o in enumerate(objs) if o["type"] == gm.COMMIT and g.status[i] == pm.OK]

    def tree_of(c):
        e = g.edges[c]
        return e[0][0] if e and e[0][0] != gm.NO_LINK else None

    pairs = []
    for c in commits:
        e = g.edges[c]
        parent = e[1][0] if len(e) >= 2 and e[1][0] != gm.NO_LINK else None
        pairs.append((tree_of(parent) if parent is not None else None, tree_of(c)))
    return list(commits), pairs
