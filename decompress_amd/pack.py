"""git packfiles (pack v2 / v3 with an idx v2) through the C ABI's md_pack_* entry points: the idx is read on the host, the
table of all objects - type, size, base, depth, status - is built once on the GPU, and a read decodes every selected object
and the bases it hangs off in one inflate launch a round, then applies the deltas level by level.  A pack without an idx
gets one from the GPU (`build_index`, git index-pack's bytes).  `write` makes a pack and its idx from objects and the
bases the caller chooses - or, with bases="search", the bases `choose_bases` finds by content sketches -, the deltas made
by a batched kernel (`make_deltas` is that kernel alone).  `Pack.graph` reads what every commit, tree and tag names - the
object graph, on the GPU -, `Graph.reachable` walks it from roots, and `Pack.extract` writes the pack of what is reachable.
`Pack.diff` diffs pairs of trees on the GPU, all pairs at once and level by level, and `Pack.changes` every commit against
its first parent's tree."""
import ctypes

import numpy as _np

from . import engine as _engine
from ._lib import PackBuildResult, PackBuildStats, PackIndexEntry, PackIndexInfo, PackInfo, PackObject, PackResult, PackStats
from ._lib import PackDiffInfo, PackGraphInfo, PackReachStats, PackSource, PackWriteResult
from ._lib import load as _load

TYPE_NAMES = {0: None, 1: "commit", 2: "tree", 3: "blob", 4: "tag"}
_TYPE_OF = {v: k for k, v in TYPE_NAMES.items() if v}
VERIFY_CRC = 1
VERIFY_NAMES = 2
NO_BASE = (1 << 64) - 1
BUILD_CHECK_TRAILER = 1
WRITE_NO_DELTA = 1
_WRITE_RESULT_KEYS = ("n", "deltas", "max_depth")
_INFO_KEYS = ("n", "deltas", "max_depth", "total_size", "failed")
_OBJECT_KEYS = ("size", "offset", "packed_len", "base", "depth", "type", "status")
_STATS_KEYS = ("rounds", "inflate_launches", "apply_launches", "objects", "bytes_in", "apply_ns")
_BUILD_RESULT_KEYS = ("n", "failed", "idx_len", "bad_offset", "bad_status")
_GRAPH_INFO_KEYS = ("n", "edges", "absent", "mistyped", "malformed", "failed", "parsed", "rounds", "parse_launches", "device_ns")
_REACH_STATS_KEYS = ("host_closed", "seeds", "rounds", "expanded", "marked", "device_ns")
NO_LINK = 0xFFFFFFFF
INVALID_OBJECT = 27
# an edge's kind (its low bits) and its two flags
COMMIT_TREE, COMMIT_PARENT, TAG_TARGET, TREE_BLOB, TREE_TREE, TREE_GITLINK = 1, 2, 3, 4, 5, 6
EDGE_ABSENT, EDGE_MISTYPED = 0x40, 0x80
# the graph's own status: engine.STATUS_NAMES and md_status_string end at 26
_GRAPH_STATUS_NAMES = {INVALID_OBJECT: "Invalid object"}
# trees diffed: the empty tree as a side of a pair, md_pack_diff's flag, a record's two flags
TREE_NONE = 0xFFFFFFFF
DIFF_RECURSIVE = 1
CHANGE_TREE, CHANGE_OPAQUE = 1, 2
# md_tree_change of include/mdeflate.h as numpy reads it (tests/test_pack_diff_abi.py holds it to the ctypes mirror)
_CHANGE_DTYPE = _np.dtype({"names": ["pair", "parent", "kind", "flags", "a_mode", "b_mode", "a_obj", "b_obj", "name_len", "name_off", "a_name", "b_name"],
                           "formats": ["<u4", "<u4", "u1", "u1", "<u4", "<u4", "<u4", "<u4", "<u4", "<u8", ("u1", 20), ("u1", 20)],
                           "offsets": [0, 4, 8, 9, 12, 16, 20, 24, 28, 32, 40, 60], "itemsize": 80})
_DIFF_INFO_KEYS = ("pairs", "changes", "name_bytes", "levels", "opaque", "failed", "trees_read", "launches", "device_ns")
_BUILD_STATS_KEYS = ("candidates", "generations", "rounds", "inflate_launches", "apply_launches", "objects", "bytes_in")


def _raw(src):
    return src if isinstance(src, bytes) else bytes(src)


def _status_name(st):
    if st in _GRAPH_STATUS_NAMES:
        return _GRAPH_STATUS_NAMES[st]
    return _engine.STATUS_NAMES.get(st, _load().md_status_string(st).decode())


def _flags(crc, names):
    return (VERIFY_CRC if crc else 0) | (VERIFY_NAMES if names else 0)


def _type(t):
    return _TYPE_OF[t] if isinstance(t, str) else int(t)


def _sources(objects, bases=None):
    """objects = [(type, bytes)] laid out back to back -> (the md_pack_source rows, that blob); bases[i]: an index or None"""
    src, at = (PackSource * max(len(objects), 1))(), 0
    for i, (s, (t, b)) in enumerate(zip(src, objects)):
        s.off, s.len, s.type = at, len(b), _type(t)
        s.base = NO_BASE if bases is None or bases[i] is None else int(bases[i])
        at += len(b)
    return src, b"".join(bytes(b) for _, b in objects)


def _select(select, k):
    return None if select is None else (ctypes.c_uint64 * max(k, 1))(*[int(i) for i in select])


def index(idx):
    """md_pack_index (host arithmetic, no device needed) -> (entries, info): one dict per object in the idx's order - name
    (20 bytes), offset, crc32 - and a dict of the idx's: n, has_64bit_table, pack_checksum.  Raises `Error` ("Invalid
    index", "Unsupported pack") for what is no idx version 2."""
    lib, idx = _load(), _raw(idx)
    info = PackIndexInfo()
    st = lib.md_pack_index(idx, len(idx), ctypes.byref(info), None, 0)
    if st != 0:
        raise _engine.Error(lib.md_status_string(st).decode())
    ents = (PackIndexEntry * max(info.n, 1))()
    st = lib.md_pack_index(idx, len(idx), ctypes.byref(info), ents, info.n)
    if st != 0:
        raise _engine.Error(lib.md_status_string(st).decode())
    out = [{"name": bytes(e.name), "offset": e.offset, "crc32": e.crc32} for e in ents[:info.n]]
    return out, {"n": info.n, "has_64bit_table": info.has_64bit_table, "pack_checksum": bytes(info.pack_checksum)}


def hash_objects(types, bufs, device=0):
    """`git hash-object` for a batch: the 20-byte names of the objects whose contents are `bufs` and whose types are `types`
    (1 commit, 2 tree, 3 blob, 4 tag, or those words), hashed on the GPU (md_sha1_batch_host)"""
    types = [_type(t) for t in types]
    if any(not 1 <= t <= 4 for t in types):
        raise ValueError("a git object is a commit, a tree, a blob or a tag")
    return _engine.default_engine(device).sha1_batch(bufs, types)


def check_trailers(pack, idx):
    """md_pack_check_trailers (host, no device needed) -> (pack_ok, idx_ok): each file's last 20 bytes are the SHA-1 of what
    is in front of them.  Raises `Error` ("Invalid pack", "Invalid index") for a file too short to be one."""
    lib, pack, idx = _load(), _raw(pack), _raw(idx)
    pack_ok, idx_ok = ctypes.c_int(0), ctypes.c_int(0)
    st = lib.md_pack_check_trailers(pack, len(pack), idx, len(idx), ctypes.byref(pack_ok), ctypes.byref(idx_ok))
    if st != 0:
        raise _engine.Error(lib.md_status_string(st).decode())
    return bool(pack_ok.value), bool(idx_ok.value)


def write_index(entries, pack_checksum):
    """md_pack_index_write (host arithmetic, no device needed), the inverse of `index`: entries - dicts with name (20 bytes),
    offset, crc32, in any order - and the pack's 20-byte checksum -> the idx version 2.  Raises `Error` ("Invalid index")
    for two entries with one name."""
    lib, n = _load(), len(entries)
    ents = (PackIndexEntry * max(n, 1))()
    for e, d in zip(ents, entries):
        e.offset, e.crc32 = d["offset"], d["crc32"]
        e.name[:] = bytes(d["name"])
    need = ctypes.c_size_t(0)
    st = lib.md_pack_index_write(ents, n, bytes(pack_checksum), None, 0, ctypes.byref(need))
    if st != 2:  # (no idx fits 0 bytes: MD_UNEXPECTED_END_OF_OUTPUT says how long it is)
        raise _engine.Error(lib.md_status_string(st).decode())
    idx = ctypes.create_string_buffer(need.value)
    st = lib.md_pack_index_write(ents, n, bytes(pack_checksum), idx, need.value, ctypes.byref(need))
    if st != 0:
        raise _engine.Error(lib.md_status_string(st).decode())
    return idx.raw[:need.value]


def build_index_raw(pack, flags=BUILD_CHECK_TRAILER, idx_cap=None, cap=None, device=0):
    """md_pack_index_build as it is: (return value, the bytes of idx, offsets, statuses, md_pack_build_result as a dict).
    idx_cap None: room for the idx of as many objects as the pack's header states (bounded by the pack's length: no object
    has fewer than 9 bytes), and what comes back is the idx alone; a given idx_cap: those bytes, NUL where nothing was
    written.  cap None: every object."""
    eng, pack = _engine.default_engine(device), _raw(pack)
    res = PackBuildResult()
    count = min(int.from_bytes(pack[8:12], "big"), len(pack) // 8) if len(pack) >= 12 else 0
    room = 8 + 1024 + 36 * count + 40 if idx_cap is None else idx_cap
    cap = count if cap is None else cap
    idx = ctypes.create_string_buffer(max(room, 1))
    off, status = (ctypes.c_uint64 * max(cap, 1))(), (ctypes.c_int32 * max(cap, 1))()
    rc = eng.lib.md_pack_index_build(eng.ctx, pack, len(pack), flags, idx if room else None, room, off if cap else None, status if cap else None, cap,
                                     ctypes.byref(res))
    k = min(cap, res.n)
    got = idx.raw[:room] if idx_cap is not None else idx.raw[:res.idx_len] if rc == 0 else b""
    return rc, got, list(off[:k]), list(status[:k]) if rc != 2 else [], {k: getattr(res, k) for k in _BUILD_RESULT_KEYS}


def build_index(pack, check_trailer=True, device=0):
    """md_pack_index_build: the idx version 2 of a pack that has none - what `git index-pack` writes, byte for byte - with
    the objects found, decoded, hashed and checksummed on the GPU.  Raises `Error` with the status name and the offset
    where the pack or one of its objects fails."""
    rc, idx, _, _, res = build_index_raw(pack, BUILD_CHECK_TRAILER if check_trailer else 0, device=device)
    if rc != 0:
        where = "" if res["bad_offset"] == NO_BASE else " at offset %d" % res["bad_offset"]
        raise _engine.Error(_status_name(rc) + where)
    return idx[:res["idx_len"]]


def build_last(device=0):
    """md_pack_build_last: candidates, generations, rounds, inflate_launches, apply_launches, objects, bytes_in of the
    engine's last `build_index`"""
    eng = _engine.default_engine(device)
    s = PackBuildStats()
    eng._check(eng.lib.md_pack_build_last(eng.ctx, ctypes.byref(s)))
    return {k: getattr(s, k) for k in _BUILD_STATS_KEYS}


def make_deltas(pairs, device=0):
    """md_pack_delta_batch_host for pairs = [(base bytes, target bytes)] -> [delta bytes]: the deltas of mdeflate.h's
    definition, made on the GPU, one wavefront a pair; any reader of git's delta format applies them.  A base object shared
    by several pairs (the same bytes object) is laid out and indexed once."""
    blob, place, rows = bytearray(), {}, []
    for base, target in pairs:
        for b in (base, target):
            if id(b) not in place:
                place[id(b)] = len(blob)
                blob += bytes(b)
        rows.append((place[id(base)], len(base), place[id(target)], len(target)))
    got = _engine.default_engine(device).pack_deltas(bytes(blob), rows)
    for st, _ in got:
        if st != 0:
            raise _engine.Error(_status_name(st))
    return [d for _, d in got]


def write_raw(objects, bases=None, level=6, max_depth=50, flags=0, pack_cap=None, device=0):
    """md_pack_write as it is: objects = [(type, bytes)] -> (return value, pack bytes, pack_len, entries as dicts,
    md_pack_write_result as a dict).  pack_cap None: md_pack_write_bound's."""
    eng, n = _engine.default_engine(device), len(objects)
    src, blob = _sources(objects, bases)
    cap = int(eng.lib.md_pack_write_bound(n, src)) if pack_cap is None else pack_cap
    out = ctypes.create_string_buffer(max(cap, 1))
    ents, need, res = (PackIndexEntry * max(n, 1))(), ctypes.c_size_t(0), PackWriteResult()
    rc = eng.lib.md_pack_write(eng.ctx, level, flags, max_depth, n, src, blob, len(blob), out if cap else None, cap, ctypes.byref(need), ents,
                               ctypes.byref(res))
    entries = [{"name": bytes(e.name), "offset": e.offset, "crc32": e.crc32} for e in ents[:n]] if rc == 0 else []
    return rc, out.raw[:need.value] if rc == 0 else b"", need.value, entries, {k: getattr(res, k) for k in _WRITE_RESULT_KEYS}


def choose_bases_raw(objects, window=4, max_depth=50, device=0):
    """md_pack_choose_bases as it is: objects = [(type, bytes)] -> (return value, order, bases): order[r] = the input index at
    rank r of the pack order, bases[r] = the RANK of the base chosen for the object at rank r, or None."""
    eng, n = _engine.default_engine(device), len(objects)
    (src, blob), out = _sources(objects), (PackSource * max(n, 1))()
    order = (ctypes.c_uint64 * max(n, 1))()
    rc = eng.lib.md_pack_choose_bases(eng.ctx, window, max_depth, n, src, blob, len(blob), out, order)
    if rc != 0:
        return rc, [], []
    return rc, list(order[:n]), [None if o.base == NO_BASE else o.base for o in out[:n]]


def choose_bases(objects, window=4, max_depth=50, device=0):
    """md_pack_choose_bases: for a bag of objects = [(type, bytes)] -> (order, bases): the pack order - by type, longest
    first - as input indices, and for the object at every rank the rank of the base that gives it the smallest delta among
    the at most 4 * window objects in front of it that share one of its four content features, or None.
    `write([objects[i] for i in order], bases, max_depth=max_depth)` keeps every one of these deltas; `write(objects,
    bases="search")` is both steps.  Sketches and delta sizes are the GPU's, order, grouping and choice the host's."""
    rc, order, bases = choose_bases_raw(objects, window, max_depth, device)
    if rc != 0:
        _engine.default_engine(device)._check(rc)
    return order, bases


def search_last(device=0):
    """md_pack_search_last: featured, pairs, fitted, chosen, launches, sketch_ns, score_ns, host_ns of the engine's last
    `choose_bases`"""
    return _engine.default_engine(device).pack_search_last()


def write(objects, bases=None, level=6, max_depth=50, deltas=True, device=0, window=4):
    """md_pack_write and md_pack_index_write: objects = [(type, bytes)] in pack order, type 1 commit, 2 tree, 3 blob, 4 tag (or
    those words); bases[i] = the index of an EARLIER object of the same type whose content object i may be a delta against,
    or None -> (pack, idx): a pack version 2 with OFS_DELTAs and its idx version 2.  Names, deltas, zlib streams and CRCs are
    the GPU's.  max_depth 0: no limit; deltas False: every object whole.  bases="search": the objects come in any order,
    `choose_bases(objects, window, max_depth)` orders them and chooses, and the pack holds them in that order.  Raises
    `Error` ("Invalid index") for two objects with one name, and for what the call refuses."""
    if isinstance(bases, str):
        if bases != "search":
            raise ValueError('bases is a list or "search"')
        order, bases = choose_bases(objects, window, max_depth, device)
        objects = [objects[i] for i in order]
    rc, pack, _, entries, _ = write_raw(objects, bases, level, max_depth, 0 if deltas else WRITE_NO_DELTA, device=device)
    if rc != 0:
        _engine.default_engine(device)._check(rc)
    return pack, write_index(entries, pack[-20:])


def write_last(device=0):
    """md_pack_write_last: pairs, kept, dropped_size, dropped_depth, payload_before, payload_after, launches, delta_ns of the
    engine's last `write` or `make_deltas`"""
    return _engine.default_engine(device).pack_write_last()


class Pack:
    """md_pack_open: the table of a pack's objects.  `info`: n, deltas, max_depth, total_size, failed.  `objects`: one dict
    per object in idx order - name, type (1 commit, 2 tree, 3 blob, 4 tag: the chain's root's), size, offset, packed_len,
    base (an index, or None), depth, status (0 = Ok).  Raises `Error` for a pack or idx the call refuses.  idx None: the pack
    came without one and `build_index` makes it (`self.idx` keeps its bytes)."""

    def __init__(self, pack, idx=None, device=0):
        self._eng = _engine.default_engine(device)
        self._pack = _raw(pack)
        self._device = device
        idx = build_index(self._pack, device=device) if idx is None else _raw(idx)
        self.idx = idx
        h = ctypes.c_void_p()
        st = self._eng.lib.md_pack_open(self._eng.ctx, self._pack, len(self._pack), idx, len(idx), ctypes.byref(h))
        if st != 0:
            self._eng._check(st)
        self._h = h
        lib = self._eng.lib
        info = PackInfo()
        lib.md_pack_get(self._h, ctypes.byref(info))
        self.info = {k: getattr(info, k) for k in _INFO_KEYS}
        objs = (PackObject * max(info.n, 1))()
        lib.md_pack_objects(self._h, objs, info.n)
        self.objects = []
        for o in objs[:info.n]:
            d = {k: getattr(o, k) for k in _OBJECT_KEYS}
            d["name"] = bytes(o.name)
            d["base"] = None if o.base == NO_BASE else o.base
            self.objects.append(d)

    def find(self, name):
        """the index of the object named by 20 bytes (or 40 hex digits), or -1"""
        name = bytes.fromhex(name) if isinstance(name, str) else bytes(name)
        if len(name) != 20:
            raise ValueError("a name has 20 bytes")
        return self._eng.lib.md_pack_find(self._h, name)

    def read_raw(self, select=None, verify_crc=False, dst_cap=None, verify_names=False):
        """md_pack_read as it is: (return value, statuses, out_off, bytes of dst, md_pack_result as a dict)"""
        k = len(self.objects) if select is None else len(select)
        sel = _select(select, k)
        need = sum(self.objects[i]["size"] for i in (range(k) if select is None else select) if 0 <= i < len(self.objects))
        cap = need if dst_cap is None else dst_cap
        dst = ctypes.create_string_buffer(max(cap, 1))
        out_off, status, res = (ctypes.c_uint64 * (k + 1))(), (ctypes.c_int32 * max(k, 1))(), PackResult()
        rc = self._eng.lib.md_pack_read(self._eng.ctx, self._h, self._pack, len(self._pack), sel, k, _flags(verify_crc, verify_names), dst, cap,
                                        out_off, status, ctypes.byref(res))
        return rc, list(status[:k]), list(out_off), dst.raw[:cap], {"entries": res.entries, "failed": res.failed, "written": res.written}

    def read(self, select=None, verify_crc=False, verify_names=False):
        """md_pack_read: every object (or the indices in `select`, in idx order, repeats allowed) ->
        [("Ok", (type, bytes)) | ("Error", status name)].  Objects are independent: a damaged one has its own status, and
        so have the deltas that hang off it; the others are whole.  verify_names: every decoded object's SHA-1 is held
        against its name in the idx ("Invalid_checksum" where it differs).  Raises `Error` for a selection out of range."""
        rc, status, off, raw, _ = self.read_raw(select, verify_crc, None, verify_names)
        if rc != 0:
            self._eng._check(rc)
        idx = range(len(self.objects)) if select is None else select
        return [("Ok", (self.objects[i]["type"], raw[off[j]:off[j + 1]])) if status[j] == 0 else ("Error", _status_name(status[j]))
                for j, i in enumerate(idx)]

    def verify_raw(self, select=None, flags=VERIFY_CRC | VERIFY_NAMES):
        """md_pack_verify as it is: (return value, statuses, md_pack_result as a dict)"""
        k = len(self.objects) if select is None else len(select)
        sel = _select(select, k)
        status, res = (ctypes.c_int32 * max(k, 1))(), PackResult()
        rc = self._eng.lib.md_pack_verify(self._eng.ctx, self._h, self._pack, len(self._pack), sel, k, flags, status, ctypes.byref(res))
        return rc, list(status[:k]), {"entries": res.entries, "failed": res.failed, "written": res.written}

    def verify(self, select=None, crc=True, names=True):
        """md_pack_verify: every object (or those in `select`) decoded and checked on the device - the idx's CRC-32 of its
        packed bytes, the SHA-1 of its content against its name - with nothing copied back -> [status name], "Ok" for a
        sound object.  Raises `Error` for a selection out of range."""
        rc, status, _ = self.verify_raw(select, _flags(crc, names))
        if rc != 0:
            self._eng._check(rc)
        return [_status_name(st) for st in status]

    def last(self):
        """md_pack_last: rounds, inflate_launches, apply_launches, objects, bytes_in, apply_ns of the engine's last read"""
        s = PackStats()
        self._eng._check(self._eng.lib.md_pack_last(self._eng.ctx, ctypes.byref(s)))
        return {k: getattr(s, k) for k in _STATS_KEYS}

    def build_last(self):
        """md_pack_build_last of this pack's engine"""
        return build_last(self._device)

    def graph(self, verify_crc=False):
        """md_pack_graph_build -> `Graph`: what every commit, tree and tag of the pack names, read on the GPU"""
        return Graph(self, verify_crc)

    def extract(self, roots, exclude=(), **write_kw):
        """the pack of what is reachable from `roots` and not from `exclude` (`Graph.reachable`): those objects read and
        written again with bases="search" -> (pack, idx) as `write` returns them; write_kw: `write`'s level, max_depth, window"""
        g = self.graph()
        try:
            keep = [int(i) for i in g.reachable(roots, exclude)]
        finally:
            g.close()
        objects = []
        for i, (tag, got) in zip(keep, self.read(keep)):
            if tag != "Ok":
                raise _engine.Error("object %s: %s" % (self.objects[i]["name"].hex(), got))
            objects.append(got)
        return write(objects, bases="search", device=self._device, **write_kw)

    def _diff_call(self, pairs, recursive, graph, cap=None, names_cap=None):
        """md_pack_diff and its getters -> (return value, the records as a numpy array of _CHANGE_DTYPE, names, statuses, info)"""
        eng, lib = self._eng, self._eng.lib
        g = graph or self.graph()
        try:
            k = len(pairs)
            a = _np.array([TREE_NONE if x is None else int(x) for x, _ in pairs], dtype=_np.int64).astype(_np.uint32)
            b = _np.array([TREE_NONE if y is None else int(y) for _, y in pairs], dtype=_np.int64).astype(_np.uint32)
            h = ctypes.c_void_p()
            rc = lib.md_pack_diff(eng.ctx, self._h, g._h, self._pack, len(self._pack), k, a.ctypes.data if k else None, b.ctypes.data if k else None,
                                  DIFF_RECURSIVE if recursive else 0, ctypes.byref(h))
        finally:
            if graph is None:
                g.close()
        none = _np.zeros(0, dtype=_CHANGE_DTYPE)
        if rc != 0:
            return rc, none, b"", [], {}
        try:
            info = PackDiffInfo()
            lib.md_pack_diff_get(h, ctypes.byref(info))
            self._diff_last = {key: getattr(info, key) for key in _DIFF_INFO_KEYS}
            cap = info.changes if cap is None else cap
            names_cap = info.name_bytes if names_cap is None else names_cap
            recs, names = _np.zeros(cap, dtype=_CHANGE_DTYPE), _np.zeros(names_cap, dtype=_np.uint8)
            status = _np.zeros(k, dtype=_np.int32)
            lib.md_pack_diff_status(h, status.ctypes.data if k else None)
            rc = lib.md_pack_diff_changes(h, recs.ctypes.data if cap else None, cap, names.ctypes.data if names_cap else None, names_cap)
            if rc != 0:
                return rc, none, b"", status.tolist(), dict(self._diff_last)
            return 0, recs[:info.changes], names[:info.name_bytes].tobytes(), status.tolist(), dict(self._diff_last)
        finally:
            lib.md_pack_diff_free(h)

    def diff_raw(self, pairs, recursive=True, graph=None, cap=None, names_cap=None):
        """md_pack_diff as it is: pairs = [(a, b)], indices of trees or None for the empty tree -> (return value, records as
        dicts in their order, the names blob, statuses, md_pack_diff_info as a dict).  cap / names_cap None: what the call needs."""
        rc, recs, names, status, info = self._diff_call(pairs, recursive, graph, cap, names_cap)
        out = [{"pair": int(r["pair"]), "parent": None if r["parent"] == TREE_NONE else int(r["parent"]), "kind": chr(r["kind"]), "flags": int(r["flags"]),
                "a_mode": int(r["a_mode"]), "b_mode": int(r["b_mode"]), "a_obj": None if r["a_obj"] == NO_LINK else int(r["a_obj"]),
                "b_obj": None if r["b_obj"] == NO_LINK else int(r["b_obj"]), "name_len": int(r["name_len"]), "name_off": int(r["name_off"]),
                "a_name": r["a_name"].tobytes(), "b_name": r["b_name"].tobytes()} for r in recs]
        return rc, out, names, status, info

    def diff(self, pairs, recursive=True, graph=None):
        """md_pack_diff: pairs = [(a, b)] of trees - indices, or None for the empty tree - diffed on the GPU, all pairs at once
        and level by level -> per pair ("Ok", [(kind, a_mode, b_mode, a_name, b_name, path, flags)]) or (status name, None).
        kind: "A", "D", "M", "T"; modes canonical, 0 and twenty zero bytes on the side that has no entry; path: the names
        from the pair's root down, joined with "/"; flags: CHANGE_TREE for a directory's own record (`git diff-tree -t`'s
        lines), CHANGE_OPAQUE for a directory that could not be descended.  recursive False: the top level alone
        (`git diff-tree` without -r).  graph: a `Graph` of this pack to use (else one is built for the call).  No renames."""
        rc, recs, names, status, _ = self._diff_call(pairs, recursive, graph)
        if rc != 0:
            self._eng._check(rc)
        out, paths = [[] for _ in pairs], []
        col = {key: recs[key].tolist() for key in ("pair", "parent", "kind", "flags", "a_mode", "b_mode", "name_len", "name_off")}
        an, bn = recs["a_name"].tobytes(), recs["b_name"].tobytes()
        for k, (pair, parent, kind, flags, am, bm, ln, off) in enumerate(zip(*col.values())):
            name = names[off:off + ln]
            paths.append(name if parent == TREE_NONE else paths[parent] + b"/" + name)
            out[pair].append((chr(kind), am, bm, an[20 * k:20 * k + 20], bn[20 * k:20 * k + 20], paths[-1], flags))
        return [("Ok", out[q]) if st == 0 else (_status_name(st), None) for q, st in enumerate(status)]

    def changes(self, commits=None, graph=None):
        """what every commit changed: each commit of `commits` (indices; None: every commit of the pack, in idx order) against
        its first parent's tree, a commit without a parent in the pack against the empty tree - the shape of `git log --raw
        --no-renames -m --first-parent` -> (commits, `diff`'s list).  A commit whose tree the pack does not hold is diffed
        as the empty tree.  The trees come from the graph's COMMIT_TREE and COMMIT_PARENT edges."""
        g = graph or self.graph()
        try:
            if commits is None:
                commits = [i for i, o in enumerate(self.objects) if o["type"] == 1 and g.status[i] == 0]
            commits = [int(c) for c in commits]
            # a commit's edges are its tree, then its parents (a malformed commit has none)
            first, to = g.first.astype(_np.int64), _np.append(g.to, _np.uint32(NO_LINK)).astype(_np.int64)
            none = len(to) - 1

            def tree_of(c):
                ok = (c >= 0) & (first[_np.maximum(c, 0)] < first[_np.maximum(c, 0) + 1])
                return _np.where(ok, to[_np.where(ok, first[_np.maximum(c, 0)], none)], NO_LINK)

            c = _np.array(commits, dtype=_np.int64).reshape(-1)
            has_parent = first[c + 1] - first[c] >= 2 if len(c) else _np.zeros(0, dtype=bool)
            parent = _np.where(has_parent, to[_np.where(has_parent, first[c] + 1, none)], NO_LINK)
            ta, tb = tree_of(_np.where(parent == NO_LINK, -1, parent)), tree_of(c)
            pairs = [(None if x == NO_LINK else x, None if y == NO_LINK else y) for x, y in zip(ta.tolist(), tb.tolist())]
            return commits, self.diff(pairs, True, g)
        finally:
            if graph is None:
                g.close()

    def diff_last(self):
        """md_pack_diff_get of this pack's last `diff` / `changes`: pairs, changes, name_bytes, levels, opaque, failed,
        trees_read, launches, device_ns"""
        return dict(getattr(self, "_diff_last", {}))

    def close(self):
        if getattr(self, "_h", None):
            self._eng.lib.md_pack_free(self._h)
            self._h = None

    __del__ = close


class Graph:
    """md_pack_graph_build: the object graph of a `Pack`.  `first` (n + 1), `to`, `kind`: the edges as a CSR over the objects
    in idx order - object i's are to[first[i]:first[i + 1]], NO_LINK where the name is not in the pack or is a gitlink's;
    kind: COMMIT_TREE .. TREE_GITLINK, with EDGE_ABSENT / EDGE_MISTYPED or-ed in.  `status`: one per object, INVALID_OBJECT
    for a commit, tree or tag whose links cannot be read (it has no edges).  `info`: n, edges, absent, mistyped, malformed,
    failed, parsed, rounds, parse_launches, device_ns.  Blobs are not decoded."""

    def __init__(self, pack, verify_crc=False):
        self._pack, self._eng = pack, pack._eng
        lib, h = self._eng.lib, ctypes.c_void_p()
        st = lib.md_pack_graph_build(self._eng.ctx, pack._h, pack._pack, len(pack._pack), VERIFY_CRC if verify_crc else 0, ctypes.byref(h))
        if st != 0:
            self._eng._check(st)
        self._h = h
        info = PackGraphInfo()
        lib.md_pack_graph_get(h, ctypes.byref(info))
        self.info = {k: getattr(info, k) for k in _GRAPH_INFO_KEYS}
        n, e = info.n, info.edges
        self.first, self.to = _np.zeros(n + 1, dtype=_np.uint64), _np.zeros(e, dtype=_np.uint32)
        self.kind, self.status = _np.zeros(e, dtype=_np.uint8), _np.zeros(n, dtype=_np.int32)
        self._eng._check(lib.md_pack_graph_edges(h, self.first.ctypes.data, self.to.ctypes.data, self.kind.ctypes.data, e))
        self._eng._check(lib.md_pack_graph_status(h, self.status.ctypes.data))

    def edges_of(self, i):
        """object i's edges -> [(from, position, to or None, kind)]"""
        a, b = int(self.first[i]), int(self.first[i + 1])
        return [(i, k - a, None if self.to[k] == NO_LINK else int(self.to[k]), int(self.kind[k])) for k in range(a, b)]

    def _flagged(self, flag):
        own = _np.searchsorted(self.first, _np.nonzero(self.kind & flag)[0], side="right") - 1
        return [e for i in dict.fromkeys(own.tolist()) for e in self.edges_of(i) if e[3] & flag]

    def missing(self):
        """the edges whose name the pack does not hold"""
        return self._flagged(EDGE_ABSENT)

    def mistyped(self):
        """the edges whose target is of another type than the edge calls for"""
        return self._flagged(EDGE_MISTYPED)

    def connected(self):
        """no edge is absent or mistyped and every object's status is Ok"""
        return self.info["absent"] == 0 and self.info["mistyped"] == 0 and not self.status.any()

    def _indices(self, what):
        out = []
        for r in what:
            if isinstance(r, (bytes, bytearray)):
                i = self._pack.find(r)
                if i < 0:
                    raise KeyError(bytes(r).hex())
                r = i
            out.append(int(r))
        return out

    def reachable(self, roots, exclude=()):
        """md_pack_reachable: roots / exclude - indices or 20-byte names (`KeyError` for a name the pack does not hold) ->
        the sorted indices of what is reached from the roots and not from `exclude`.  Raises `Error` for an index out of range."""
        roots, exclude, n = self._indices(roots), self._indices(exclude), int(self.info["n"])
        r, x = (ctypes.c_uint64 * max(len(roots), 1))(*roots), (ctypes.c_uint64 * max(len(exclude), 1))(*exclude)
        mark, count = _np.zeros(max(n, 1), dtype=_np.uint8), ctypes.c_uint64(0)
        st = self._eng.lib.md_pack_reachable(self._eng.ctx, self._h, r if roots else None, len(roots), x if exclude else None, len(exclude),
                                             mark.ctypes.data, ctypes.byref(count))
        if st != 0:
            self._eng._check(st)
        got = _np.nonzero(mark[:n])[0]
        assert len(got) == count.value
        return got

    def reach_last(self):
        """md_pack_reach_last: host_closed, seeds, rounds, expanded, marked, device_ns of the engine's last `reachable`"""
        s = PackReachStats()
        self._eng._check(self._eng.lib.md_pack_reach_last(self._eng.ctx, ctypes.byref(s)))
        return {k: getattr(s, k) for k in _REACH_STATS_KEYS}

    def close(self):
        if getattr(self, "_h", None):
            self._eng.lib.md_pack_graph_free(self._h)
            self._h = None

    __del__ = close
