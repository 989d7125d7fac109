"""The cases of the base search's tests (md_pack_sketch_*, md_pack_choose_bases): every case states its edge as a claim about
the model's trace (tests/pack_search_model.py), so a case that stops hitting its edge fails on the CPU.

sketch_cases(): [{"name", "edges", "data": bytes, "claim": f(features, positions) -> bool}]
search_cases(): [{"name", "edges", "objects": [(type, bytes)], "window", "runs": [max_depth], "claim": f(traces, one per run) -> bool}]
Filler bytes are random (numpy, fixed seeds).  A minimum is put where a case wants it by a planted block: 16 bytes whose
value for one feature is 0 (pack_search_model.planted), which no other window undercuts."""
import functools

import numpy as np

from tests import pack_delta_model as dm
from tests import pack_search_model as sm
from tests import pack_write_cases as wc

SEG = sm.SEG_POSITIONS
SKETCH_EDGES = {
    "lengths 0 15 16 17", "a step of 64 positions -1 0 +1", "a segment of 4096 positions -1 0 +1", "minimum at p = 0", "minimum at p = len - 16",
    "minimum in lane 0 of a step", "minimum in lane 63 of a step", "minimum in the last partial step", "minimum on a window that straddles a segment boundary",
    "minimum on either side of a segment boundary", "several segments",
}
SEARCH_EDGES = {
    "a group larger than window", "one candidate through two features", "equal lengths by index", "two types never paired", "target below 64, base below 16",
    "two identical objects", "max_depth 1 2 0 on a chain", "equal delta lengths", "nothing fits", "n = 0", "shuffled version chains",
    "one base of three targets, two bases of equal bytes",
}
ALIGNMENTS = wc.ALIGNMENTS
rnd = wc.rnd


def with_block(n, seed, i, p, value=0):
    """n random bytes with a block planted at p whose feature i is `value`"""
    data = bytearray(rnd(n, seed))
    data[p:p + 16] = sm.planted(i, seed + 1, value)
    return bytes(data)


@functools.lru_cache(maxsize=None)
def sketch_cases():
    out = []
    for n in (0, 15, 16, 17):
        out.append({"name": "length %d" % n, "edges": {"lengths 0 15 16 17"}, "data": rnd(n, 700 + n),
                    "claim": lambda f, p, n=n: (p is None and f == sm.NONE) if n < 16 else (max(p) <= n - 16 and f != sm.NONE)})
    # 79 bytes are exactly 64 positions, 4111 exactly a segment: the last position holds the minimum of feature n mod 4
    for step, edge in ((64, "a step of 64 positions -1 0 +1"), (SEG, "a segment of 4096 positions -1 0 +1")):
        for npos in (step - 1, step, step + 1):
            n = npos + 15
            out.append({"name": "%d positions" % npos, "edges": {edge, "minimum at p = len - 16"}, "data": with_block(n, 710 + n, n % 4, n - 16),
                        "claim": lambda f, p, n=n: p[n % 4] == n - 16 and f[n % 4] == 0})
    # where the minimum stands, for every feature: 300 bytes are 285 positions, four whole steps and one of 29
    for i in range(sm.FEATURES):
        for p, edge in ((0, "minimum at p = 0"), (284, "minimum at p = len - 16"), (128, "minimum in lane 0 of a step"), (191, "minimum in lane 63 of a step"),
                        (256 + 5 * i, "minimum in the last partial step")):
            out.append({"name": "feature %d at %d of 300" % (i, p), "edges": {edge}, "data": with_block(300, 730 + 10 * p + i, i, p),
                        "claim": lambda f, q, i=i, p=p: q[i] == p and f[i] == 0 and all(f[k] != 0 for k in range(4) if k != i)})
    # the segment boundary: positions [0, 4096) are segment 0's; a window from 4081 .. 4095 reaches into bytes that segment 1
    # starts in.  9000 bytes are three segments.
    for i, (p, edge) in enumerate(((SEG - 16, "minimum on either side of a segment boundary"), (SEG - 6, "minimum on a window that straddles a segment boundary"),
                                   (SEG - 1, "minimum on a window that straddles a segment boundary"), (SEG, "minimum on either side of a segment boundary"))):
        out.append({"name": "feature %d at %d of 9000" % (i, p), "edges": {edge, "several segments"}, "data": with_block(9000, 800 + i, i, p),
                    "claim": lambda f, q, i=i, p=p: q[i] == p and f[i] == 0})
    # four segments, every feature's minimum in another one (planted values 3 .. 0: none is reached by chance)
    data = bytearray(rnd(3 * SEG + 100 + 15, 810))
    where = (3 * SEG + 50, 2 * SEG + 77, SEG + 4000, 9)
    for i, p in enumerate(where):
        data[p:p + 16] = sm.planted(i, 811 + i, 3 - i)
    out.append({"name": "four segments", "edges": {"several segments"}, "data": bytes(data),
                "claim": lambda f, q: q == where and f == (3, 2, 1, 0)})
    assert set().union(*[c["edges"] for c in out]) == SKETCH_EDGES
    return out


@functools.lru_cache(maxsize=None)
def sketch_model():
    """[(features, positions)] of sketch_cases()"""
    return [sm.sketch(c["data"]) for c in sketch_cases()]


def laid_out(datas):
    """every buffer once in one blob, buffer k at an address that is ALIGNMENTS[k mod 5] mod 16, the gaps (never empty) 0xff,
    and the last buffer ending on the blob's last byte -> (blob, [(off, len)])"""
    blob, at = bytearray(), []
    for k, d in enumerate(datas):
        blob += b"\xff"
        blob += b"\xff" * ((ALIGNMENTS[k % len(ALIGNMENTS)] - len(blob)) % 16)
        at.append((len(blob), len(d)))
        blob += d
    return bytes(blob), at


def _chain():
    """five versions, each the one before with 12 new bytes at another place: the nearest version gives the smallest delta"""
    vs = [rnd(1500, 602)]
    for k in range(4):
        vs.append(vs[-1][:300 * k + 100] + rnd(12, 603 + k) + vs[-1][300 * k + 100:])
    return vs


def shuffled_chains():
    """tests/pack_write_cases.version_chains() in shuffled order -> (objects, the chain of every input index)"""
    objects, _ = wc.version_chains()
    perm = np.random.default_rng(7).permutation(len(objects))
    return [objects[i] for i in perm], [int(i) // 8 for i in perm]


def plan_objects():
    """Seven blobs for window 1, where a target is scored against the nearest object in front of it in each of its four groups.
    S carries a planted block for each of the features 0, 1 and 2, and T0, T1, T2 are its three thirds, one block in each
    and no window in common: S is the base of all three, and none of them of another.  C stands twice, and D is C's first 400 bytes: the second C is scored against the first, D
    against the second - two bases of equal bytes at two addresses."""
    parts = [rnd(150, 940 + k) for k in range(4)]
    S = parts[0] + sm.planted(0, 944) + parts[1] + sm.planted(1, 945) + parts[2] + sm.planted(2, 946) + parts[3]
    C = rnd(200, 947) + sm.planted(3, 948) + rnd(500, 949)
    return [(3, S), (3, S[:216]), (3, S[216:432]), (3, S[432:]), (3, C), (3, C), (3, C[:400])]


@functools.lru_cache(maxsize=None)
def search_cases():
    out = []
    # -- six objects that share one feature and nothing else, window 2: the cut keeps the two nearest; nothing fits
    objs = [(3, rnd(50 + k, 900 + k) + sm.planted(0, 899) + rnd(334 - 11 * k, 910 + k)) for k in range(6)]
    out.append({"name": "a group of six", "edges": {"a group larger than window", "nothing fits"}, "objects": objs, "window": 2, "runs": [50],
                "claim": lambda ts: ts[0]["order"] == list(range(6)) and ts[0]["pairs"] == [(1, 0), (2, 0), (2, 1), (3, 1), (3, 2), (4, 2), (4, 3), (5, 3), (5, 4)] and
                ts[0]["last"]["fitted"] == 0 and ts[0]["bases"] == [None] * 6 and all(st == dm.MD_UNEXPECTED_END_OF_OUTPUT for st, _ in ts[0]["scores"])})
    # -- two objects that share two planted features, and two that share all four by content: one pair each
    a = bytearray(rnd(500, 910))
    b = bytearray(rnd(480, 911))
    for buf in (a, b):
        buf[100:116], buf[300:316] = sm.planted(1, 912), sm.planted(3, 913)
    v = rnd(2000, 914)
    objs = [(3, bytes(a)), (3, bytes(b)), (3, v + b"tail"), (3, v)]
    out.append({"name": "through several features", "edges": {"one candidate through two features"}, "objects": objs, "window": 4, "runs": [50],
                "claim": lambda ts: ts[0]["pairs"] == [(1, 0), (3, 2)] and ts[0]["order"] == [2, 3, 0, 1] and
                sum(x == y for x, y in zip(ts[0]["features"][0], ts[0]["features"][1])) == 2 and ts[0]["features"][2] == ts[0]["features"][3] and
                ts[0]["bases"] == [None, 0, None, None]})
    # -- equal lengths: the input index decides, and with it which of two equal deltas is taken
    x = rnd(1000, 920)
    objs = [(3, rnd(40, 921) + x), (3, x), (3, rnd(40, 922) + x), (3, rnd(40, 923) + x)]
    out.append({"name": "equal lengths", "edges": {"equal lengths by index", "equal delta lengths"}, "objects": objs, "window": 4, "runs": [50],
                "claim": lambda ts: ts[0]["order"] == [0, 2, 3, 1] and [p for p in ts[0]["pairs"] if p[0] == 3] == [(3, 0), (3, 1), (3, 2)] and
                len({s for p, s in zip(ts[0]["pairs"], ts[0]["scores"]) if p[0] == 3}) == 1 and ts[0]["bases"][3] == 0 and ts[0]["scores"][-1][0] == dm.MD_OK})
    # -- the same bytes as a commit and as a blob: candidates only within a type
    typed = wc._typed_objects()
    objs = typed + [(3, typed[0][1]), (3, typed[4][1])]
    out.append({"name": "two types", "edges": {"two types never paired"}, "objects": objs, "window": 4, "runs": [50],
                "claim": lambda ts, objs=objs: all(objs[ts[0]["order"][t]][0] == objs[ts[0]["order"][b]][0] for t, b in ts[0]["pairs"]) and
                ts[0]["features"][0] == ts[0]["features"][8] and ts[0]["features"][4] == ts[0]["features"][9] and
                [objs[i][0] for i in ts[0]["order"]] == sorted(o[0] for o in objs) and ts[0]["last"]["chosen"] >= 4 and
                {objs[ts[0]["order"][t]][0] for t, _ in ts[0]["pairs"]} == {1, 2, 3, 4}})
    # -- one shared feature at the front of everything: 63 bytes are no target, 15 bytes nothing at all
    s = sm.planted(2, 930) + rnd(200, 931)
    objs = [(3, s[:15]), (3, s[:63]), (3, s[:16]), (3, s[:100]), (3, s[:64]), (3, s[:16] * 5), (3, b"")]
    out.append({"name": "too small", "edges": {"target below 64, base below 16"}, "objects": objs, "window": 4, "runs": [50],
                "claim": lambda ts: ts[0]["order"] == [3, 5, 4, 1, 2, 0, 6] and ts[0]["pairs"] == [(1, 0), (2, 0), (2, 1)] and ts[0]["last"]["featured"] == 5 and
                ts[0]["features"][0] == sm.NONE == ts[0]["features"][6] and all(ts[0]["features"][i][2] == 0 for i in (1, 2, 3, 4, 5)) and ts[0]["bases"][2] == 0})
    # -- one object twice
    B = rnd(4000, 600)
    out.append({"name": "one object twice", "edges": {"two identical objects"}, "objects": [(3, B), (3, B)], "window": 4, "runs": [50],
                "claim": lambda ts: ts[0]["pairs"] == [(1, 0)] and ts[0]["bases"] == [None, 0] and ts[0]["scores"][0] == (dm.MD_OK, 7)})
    # -- a chain under max_depth 1, 2 and 0: the nearest version is passed over for the next best
    vs = _chain()
    out.append({"name": "a chain of five", "edges": {"max_depth 1 2 0 on a chain"}, "objects": [(3, v) for v in vs], "window": 4, "runs": [1, 2, 0],
                "claim": lambda ts: all(t["order"] == [4, 3, 2, 1, 0] and len(t["pairs"]) == 10 and t["last"]["fitted"] == 10 for t in ts) and
                [t["bases"] for t in ts] == [[None, 0, 0, 0, 0], [None, 0, 1, 1, 1], [None, 0, 1, 2, 3]] and
                [t["depth"] for t in ts] == [[0, 1, 1, 1, 1], [0, 1, 2, 2, 2], [0, 1, 2, 3, 4]] and
                (2, 1) in ts[0]["skipped"] and (3, 2) in ts[1]["skipped"] and ts[2]["skipped"] == []})
    # -- what the plan of a delta batch is made of: a base shared by three pairs, equal bytes at two addresses (window 1)
    out.append({"name": "one base, three targets", "edges": {"one base of three targets, two bases of equal bytes"}, "objects": plan_objects(), "window": 1,
                "runs": [50], "claim": lambda ts: ts[0]["order"] == [4, 5, 0, 6, 1, 2, 3] and ts[0]["pairs"] == [(1, 0), (3, 1), (4, 2), (5, 2), (6, 2)] and
                all(st == dm.MD_OK for st, _ in ts[0]["scores"]) and ts[0]["bases"] == [None, 0, None, 1, 2, 2, 2]})
    out.append({"name": "nothing", "edges": {"n = 0"}, "objects": [], "window": 4, "runs": [50],
                "claim": lambda ts: ts[0]["order"] == [] and ts[0]["last"] == {"featured": 0, "pairs": 0, "fitted": 0, "chosen": 0}})
    objs, chain = shuffled_chains()
    out.append({"name": "shuffled version chains", "edges": {"shuffled version chains"}, "objects": objs, "window": 4, "runs": [50],
                "claim": lambda ts, chain=chain: ts[0]["last"]["chosen"] == 280 and
                all(b is None or chain[ts[0]["order"][r]] == chain[ts[0]["order"][b]] for r, b in enumerate(ts[0]["bases"]))})
    assert set().union(*[c["edges"] for c in out]) == SEARCH_EDGES
    return out


def case(name):
    return next(c for c in search_cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def search_model(name):
    """the model's traces of a case's runs, computed once"""
    c = case(name)
    return tuple(sm.search(c["objects"], c["window"], d) for d in c["runs"])


@functools.lru_cache(maxsize=None)
def pack_model(name, level=6):
    """the model's packs of a case's runs at a level (pack_delta_model.write_pack's dicts), computed once"""
    c = case(name)
    return tuple(sm.write_pack(c["objects"], t, level=level, max_depth=d) for t, d in zip(search_model(name), c["runs"]))
