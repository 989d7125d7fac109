"""The sketch of an object and the search for delta bases as md_pack_sketch_* and md_pack_choose_bases define them
(include/mdeflate.h), in plain Python written from those definitions: the four features with the position of
each minimum, the pack order, the candidates, the scores through tests/pack_delta_model.make_delta, the choice, and the pack
through write_pack.  Nothing here touches the code under test; numpy only hashes every position of an object at once."""
import struct

import numpy as np

from tests import pack_delta_model as dm

SEEDS = (0, 0x85EBCA6B, 0xC2B2AE35, 0x27D4EB2F)
FEATURES = 4
NONE = (0xFFFFFFFF,) * FEATURES  # what is stored for an object without features
SEG_POSITIONS = 4096  # the kernel's segment; the features do not depend on it
MASK = 0xFFFFFFFF
MUL_INV = pow(dm.MUL, -1, 1 << 32)


def position_hashes(data):
    """h(p) for every p with p + 16 <= len(data), as a uint64 array"""
    t = np.frombuffer(data, dtype=np.uint8).astype(np.uint64)
    npos = len(data) - dm.BLOCK + 1
    x = np.zeros(npos, dtype=np.uint64)
    for w in range(4):
        word = sum(t[4 * w + b:4 * w + b + npos] << np.uint64(8 * b) for b in range(4))
        x = ((x + word) * np.uint64(dm.MUL)) & np.uint64(MASK)
    return x


def feature_value(b16, i):
    return ((dm.block_hash(b16) ^ SEEDS[i]) * dm.MUL) & MASK


def sketch(data):
    """-> (features, positions): F_i and the first position whose window attains it; (NONE, None) below 16 bytes"""
    if len(data) < dm.BLOCK:
        return NONE, None
    h = position_hashes(bytes(data))
    feats, where = [], []
    for s in SEEDS:
        v = ((h ^ np.uint64(s)) * np.uint64(dm.MUL)) & np.uint64(MASK)
        p = int(np.argmin(v))
        feats.append(int(v[p]))
        where.append(p)
    return tuple(feats), tuple(where)


def planted(i, seed, value=0):
    """a block of 16 bytes whose value for feature i is `value` (0: no window has a lower one): three random words, the
    fourth solved for"""
    w = [int(v) for v in np.random.default_rng(seed).integers(0, 1 << 32, 3, dtype=np.uint64)]
    h = ((value * MUL_INV) & MASK) ^ SEEDS[i]
    x = 0
    for v in w:
        x = ((x + v) * dm.MUL) & MASK
    w.append((h * MUL_INV - x) & MASK)
    block = struct.pack("<4I", *w)
    assert feature_value(block, i) == value
    return block


def pack_order(objects):
    """the input indices by (type, len descending, index)"""
    return sorted(range(len(objects)), key=lambda i: (objects[i][0], -len(objects[i][1]), i))


def candidates(objects, order, feats, window):
    """per rank the ranks that are scored against it, ascending"""
    out, seen = [], {}
    for r, i in enumerate(order):
        t, data = objects[i]
        found = set()
        if len(data) >= dm.BLOCK:
            for k in range(FEATURES):
                group = seen.setdefault((t, k, feats[i][k]), [])
                if len(data) >= dm.DELTA_MIN_TARGET:
                    found.update(group[-window:])
                group.append(r)
        out.append(sorted(found))
    return out


def choose(cand, score_of, max_depth):
    """the choice in pack order: cand[r] = the ranks scored against rank r, ascending; score_of(r, b) -> (status, length) ->
    (bases, depth, pairs, scores, skipped)"""
    n = len(cand)
    pairs, scores, skipped = [], [], []
    bases, depth = [None] * n, [0] * n
    for r in range(n):
        best = None
        for b in cand[r]:
            st, length = score_of(r, b)
            pairs.append((r, b))
            scores.append((st, length))
            if st != dm.MD_OK:
                continue
            if max_depth and depth[b] >= max_depth:
                skipped.append((r, b))
                continue
            if best is None or length < best:
                best, bases[r], depth[r] = length, b, depth[b] + 1
    return bases, depth, pairs, scores, skipped


def search(objects, window=4, max_depth=50):
    """objects = [(type, bytes)] -> a dict: order, bases (ranks or None), depth, pairs [(target rank, base rank)], scores
    [(status, length)] per pair, skipped [(target rank, base rank)] - fitted, but the base stood at max_depth -, features,
    positions, and `last`, what md_pack_search_last counts but launches and times"""
    sk = [sketch(d) for _, d in objects]
    feats = [s[0] for s in sk]
    order = pack_order(objects)
    cand = candidates(objects, order, feats, window)

    def score_of(r, b):
        assert b < r and objects[order[b]][0] == objects[order[r]][0]
        target = objects[order[r]][1]
        return dm.delta_result(objects[order[b]][1], target, dm.delta_cap(len(target)))[:2]
    bases, depth, pairs, scores, skipped = choose(cand, score_of, max_depth)
    last = {"featured": sum(len(d) >= dm.BLOCK for _, d in objects), "pairs": len(pairs), "fitted": sum(st == dm.MD_OK for st, _ in scores),
            "chosen": sum(b is not None for b in bases)}
    return {"order": order, "bases": bases, "depth": depth, "pairs": pairs, "scores": scores, "skipped": skipped, "features": feats,
            "positions": [s[1] for s in sk], "last": last}


def launches(trace):
    """the kernel launches md_pack_search_last counts: the sketch if an object has features, the index and the sizes if a
    pair is scored"""
    return (1 if trace["last"]["featured"] else 0) + (2 if trace["pairs"] else 0)


def write_pack(objects, trace, level=6, max_depth=50, **kw):
    """the pack of the searched objects in pack order: pack_delta_model.write_pack's dict"""
    return dm.write_pack([objects[i] for i in trace["order"]], trace["bases"], level=level, max_depth=max_depth, **kw)
