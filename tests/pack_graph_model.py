"""The object graph of a git pack in plain Python, written from the rules include/mdeflate.h states for md_pack_graph_build
and md_pack_reachable: how a tree, a commit and a tag name other objects, the edges' kinds and flags, the statuses, the
counts, and the walk from roots - the host's closure over parents and tag targets, then the frontiers level by level.  The
objects' bytes come from the reader of tests/pack_model.py; nothing is shared with decompress_amd/pack.py."""
from tests import pack_model as pm

NO_LINK = 0xFFFFFFFF
COMMIT_TREE, COMMIT_PARENT, TAG_TARGET, TREE_BLOB, TREE_TREE, TREE_GITLINK = 1, 2, 3, 4, 5, 6
ABSENT, MISTYPED = 0x40, 0x80
INVALID_OBJECT = 27
COMMIT, TREE, BLOB, TAG = 1, 2, 3, 4
WANTED = {COMMIT_TREE: TREE, COMMIT_PARENT: COMMIT, TREE_BLOB: BLOB, TREE_TREE: TREE}
HEX = b"0123456789abcdefABCDEF"
TAG_TYPES = {b"blob": BLOB, b"tree": TREE, b"commit": COMMIT, b"tag": TAG}


def parse_tree(b):
    """-> [(kind, the target's 20 bytes, the type it has to have)] in the entries' order, or None: malformed"""
    size, s, out = len(b), 0, []
    while size - s != 0:
        if size - s < 23 or b[size - 21] != 0:
            return None
        sp = s
        while 0x30 <= b[sp] <= 0x37:  # (the NUL at size - 21 ends it)
            sp += 1
        if sp == s or b[sp] != 0x20:
            return None
        mode = 0
        for c in b[s:sp]:
            mode = ((mode << 3) + (c - 0x30)) & 0xFFFFFFFF
        nul = b.index(0, sp + 1)
        if nul == sp + 1 or nul + 21 > size:
            return None
        fmt = mode & 0o170000
        kind = TREE_BLOB if fmt in (0o100000, 0o120000) else TREE_TREE if fmt == 0o040000 else TREE_GITLINK
        out.append((kind, b[nul + 1:nul + 21], WANTED.get(kind)))
        s = nul + 21
    return out


def _hex40(b, at):
    h = b[at:at + 40]
    return bytes.fromhex(h.decode()) if len(h) == 40 and all(c in HEX for c in h) else None


def parse_commit(b):
    size = len(b)
    if not size > 46 or b[:5] != b"tree " or _hex40(b, 5) is None or b[45] != 0x0a:
        return None
    out, p = [(COMMIT_TREE, _hex40(b, 5), TREE)], 46
    while p + 47 < size and b[p:p + 7] == b"parent ":
        if not size > p + 48 or _hex40(b, p + 7) is None or b[p + 47] != 0x0a:
            return None
        out.append((COMMIT_PARENT, _hex40(b, p + 7), COMMIT))
        p += 48
    return out


def parse_tag(b):
    size = len(b)
    if size < 64 or b[:7] != b"object " or _hex40(b, 7) is None or b[47] != 0x0a or b[48:53] != b"type ":
        return None
    nl = b.find(b"\n", 53)
    if nl < 0 or b[53:nl] not in TAG_TYPES:
        return None
    p = nl + 1
    if not p + 4 < size or b[p:p + 4] != b"tag ":
        return None
    return [(TAG_TARGET, _hex40(b, 7), TAG_TYPES[b[53:nl]])]


PARSERS = {COMMIT: parse_commit, TREE: parse_tree, TAG: parse_tag}


def links(type_, data, by_name, types):
    """one object's edges -> [(to, kind with its flags, the 20 bytes the edge names)] or None: malformed.  by_name: name ->
    index; types: index -> type"""
    parsed = PARSERS[type_](data)
    if parsed is None:
        return None
    out = []
    for kind, name, wanted in parsed:
        if kind == TREE_GITLINK:
            out.append((NO_LINK, kind, name))
        elif name not in by_name:
            out.append((NO_LINK, kind | ABSENT, name))
        else:
            t = types[by_name[name]]
            out.append((by_name[name], kind | (MISTYPED if 1 <= t <= 4 and t != wanted else 0), name))
    return out


class Graph:
    """md_pack_graph_build of the pack: first, to, kind, status (idx order) and info, as one round of the read gives them"""

    def __init__(self, pack, idx, verify_crc=False):
        m = pm.Model(pack, idx)
        assert m.rc == pm.OK
        self.model, objs = m, m.objects
        n = len(objs)
        by_name = {o["name"]: i for i, o in enumerate(objs)}
        types = [o["type"] for o in objs]
        select = [i for i, o in enumerate(objs) if o["status"] == pm.OK and o["type"] in PARSERS]
        self.status = [o["status"] for o in objs]
        self.edges = [[] for _ in range(n)]
        self.names = [[] for _ in range(n)]  # the 20 bytes every edge names, beside self.edges
        for i, (st, data) in zip(select, m.read(select, verify_crc)):
            self.status[i] = st
            if st == pm.OK:
                got = links(types[i], data, by_name, types)
                if got is None:
                    self.status[i] = INVALID_OBJECT
                else:
                    self.edges[i] = [(t, k) for t, k, _ in got]
                    self.names[i] = [nm for _, _, nm in got]
        self.first = [0]
        for e in self.edges:
            self.first.append(self.first[-1] + len(e))
        self.to = [t for e in self.edges for t, _ in e]
        self.kind = [k for e in self.edges for _, k in e]
        launches = int(any(types[i] == TREE for i in select)) + int(any(types[i] != TREE for i in select))
        self.info = {"n": n, "edges": len(self.to), "absent": sum(bool(k & ABSENT) for k in self.kind),
                     "mistyped": sum(bool(k & MISTYPED) for k in self.kind), "malformed": self.status.count(INVALID_OBJECT),
                     "failed": sum(st not in (pm.OK, INVALID_OBJECT) for st in self.status), "parsed": len(m.closure(select)),
                     "rounds": int(bool(select)), "parse_launches": launches}

    def _walk(self, roots):
        closed, seen = [], set()
        for r in roots:
            if r not in seen:
                seen.add(r)
                closed.append(r)
        for o in closed:  # (it grows as it is walked)
            for t, k in self.edges[o]:
                if k & 0x3f in (COMMIT_PARENT, TAG_TARGET) and t != NO_LINK and t not in seen:
                    seen.add(t)
                    closed.append(t)
        frontier = [o for o in closed if self.edges[o]]
        stats = {"host_closed": len(closed), "seeds": len(frontier), "rounds": 0, "expanded": 0}
        while frontier:
            stats["rounds"] += 1
            stats["expanded"] += len(frontier)
            nxt = []
            for o in frontier:
                for t, _ in self.edges[o]:
                    if t != NO_LINK and t not in seen:
                        seen.add(t)
                        if self.edges[t]:
                            nxt.append(t)
            frontier = nxt
        return seen, stats

    def reachable(self, roots, exclude=()):
        """-> (marks, expanded, rounds), summed over the exclude walk and the root walk; self.stats: md_pack_reach_last"""
        out, stats = set(), {"host_closed": 0, "seeds": 0, "rounds": 0, "expanded": 0}
        gone = set()
        for k, what in enumerate((exclude, roots)):
            if k == 0 and not exclude:
                continue
            got, st = self._walk(list(what))
            for key in stats:
                stats[key] += st[key]
            if k == 0:
                gone = got
            else:
                out = got - gone
        marks = [int(i in out) for i in range(len(self.edges))]
        stats["marked"] = sum(marks)
        self.stats = stats
        return marks, stats["expanded"], stats["rounds"]

    def tree_depth(self, root):
        """the deepest nesting of trees below the trees that the commits reached from `root` name"""
        def below(t, guard):
            kids = [x for x, k in self.edges[t] if k & 0x3f == TREE_TREE and x != NO_LINK and x not in guard]
            return 1 + max(below(x, guard | {x}) for x in kids) if kids else 0
        seen, _ = self._walk([root])
        tops = [t for o in seen for t, k in self.edges[o] if k & 0x3f == COMMIT_TREE and t != NO_LINK]
        return max([below(t, {t}) for t in tops] or [0])
