"""The cases of the pack writer's tests (md_pack_delta_batch_*, md_pack_write): every case states its edge as a claim about
the model's trace (tests/pack_delta_model.py), so a case that stops hitting its edge fails on the CPU.

delta_cases(): [{"name", "edges", "bufs": [bytes], "pairs": [(base buffer, target buffer)], "claim": f(traces, deltas) -> bool}]
pack_cases():  [{"name", "edges", "objects": [(type, bytes)], "bases", "level" (default: the test's), "runs": [kwargs of the
                 model's write_pack], "claim": f(model results, one per run) -> bool}]
Filler bytes are random (numpy, fixed seeds) and a filler's byte next to a copied region is made to differ from the base's
neighbour, so every match is exactly as long as the case says."""
import functools

import numpy as np

from tests import pack_delta_model as dm

DELTA_EDGES = {
    "sizes 0 15 16 17 63 64", "match at p = 0", "match ends at nt", "match ends at nb", "match ends at both", "first hit in lane 0",
    "first hit in lane 63", "first hit in lane 64", "no hit in several steps", "forward 16 17", "forward 1023 1024 1025", "forward 2048 +- 1",
    "mismatch in every byte of a lane", "backward stopped by lit", "backward stopped by the base's start", "backward stopped by a byte",
    "backward 0 and 15", "copies 0xffff 0x10000 0x10001 0x20000", "one-byte copy op", "offsets 0 0x100 0x10000", "offsets 0x1000000 0x00ff00ff",
    "inserts 126 127 128 254 255", "varints 127 128", "varints 16383 16384", "two blocks in one slot", "occupied slot, other bytes",
    "one repeated block", "k 10 and 11", "several targets on one base", "a base that is a target", "identical", "shares nothing",
}
PACK_EDGES = {
    "keep bound exact and one over", "max_depth 1 2 0 on a chain of 4", "ofs varint 127 128", "ofs varint 16511 16512", "every type", "level 0",
    "n = 0", "version chains", "no delta below 64 or base below 16", "equal names",
}
ALIGNMENTS = (0, 1, 3, 8, 15)  # of bases and targets in src, mod 16


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _not(byte):
    return bytes([byte ^ 0xFF])


def fill_before(n, seed, base, a):
    """n filler bytes to stand in front of a copy of base[a ..): the last differs from base[a - 1]"""
    f = rnd(n, seed)
    return f[:-1] + _not(base[a - 1]) if n and a > 0 else f


def fill_after(n, seed, base, end):
    """n filler bytes to stand behind a copy of base[.. end): the first differs from base[end]"""
    f = rnd(n, seed)
    return _not(base[end]) + f[1:] if n and end < len(base) else f


def _ops(trace):
    return [(o[0], len(o[1])) if o[0] == "insert" else o for o in trace["ops"]]


def _one(name, edges, base, target, claim):
    return {"name": name, "edges": set(edges), "bufs": [base, target], "pairs": [(0, 1)], "claim": lambda tr, dl: claim(tr[0], dl[0])}


def _lost_base():
    """a base of 576 blocks (k = 11): 500 random ones, then 66 whose slots lower blocks hold, then 10 that own their slots
    -> (base, the index of the first block behind the 66)"""
    blocks = [rnd(16, 5000 + j) for j in range(500)]
    taken = {dm.slot_of(b, 11) for b in blocks}
    seed = 6000
    for want_lost in [True] * 66 + [False] * 10:
        while (dm.slot_of(rnd(16, seed), 11) in taken) != want_lost:
            seed += 1
        blocks.append(rnd(16, seed))
        taken.add(dm.slot_of(blocks[-1], 11))
        seed += 1
    return b"".join(blocks), 566


@functools.lru_cache(maxsize=None)
def delta_cases():
    out = []
    B = rnd(6000, 1)
    # -- sizes
    for nb in (0, 15, 16, 17, 63, 64):
        for nt in (0, 15, 16, 17, 63, 64):
            base = B[:nb]
            target = (base + rnd(64, 2))[:nt]
            out.append(_one("sizes nb %d nt %d" % (nb, nt), ["sizes 0 15 16 17 63 64"], base, target,
                            lambda t, d, nb=nb, nt=nt: (len(t["matches"]) == 1) == (min(nb, nt) >= 16) and len(t["matches"]) <= 1))
    # -- where a match begins and ends
    out.append(_one("identical", ["identical", "match at p = 0", "match ends at both"], B[:1000], B[:1000],
                    lambda t, d: _ops(t) == [("copy", 0, 1000)] and t["matches"][0]["p"] == 0))
    out.append(_one("a prefix of the base", ["match at p = 0", "match ends at nt"], B, B[:500],
                    lambda t, d: _ops(t) == [("copy", 0, 500)]))
    tail = B[-512:] + fill_after(100, 3, B, len(B))
    out.append(_one("the base's end, then more", ["match at p = 0", "match ends at nb"], B, tail,
                    lambda t, d: _ops(t) == [("copy", len(B) - 512, 512), ("insert", 100)]))
    out.append(_one("shares nothing", ["shares nothing"], B, rnd(3000, 4), lambda t, d: not t["matches"] and len(d) == 4 + 3000 + 24))
    # -- the scan
    for p, edge in ((0, "first hit in lane 0"), (63, "first hit in lane 63"), (64, "first hit in lane 64"), (64 * 5 + 7, "no hit in several steps")):
        target = fill_before(p, 5 + p, B, 160) + B[160:224] + fill_after(50, 6, B, 224)
        out.append(_one("first hit at %d" % p, [edge], B, target,
                        lambda t, d, p=p: t["matches"][0]["p"] == p and t["matches"][0]["e"] == 0 and t["scan_steps"][0] == p // 64 and t["matches"][0]["L"] == 64))
    # -- forward lengths behind the block
    fwd = [(0, "forward 16 17"), (1, "forward 16 17"), (1023, "forward 1023 1024 1025"), (1024, "forward 1023 1024 1025"),
           (1025, "forward 1023 1024 1025"), (2047, "forward 2048 +- 1"), (2048, "forward 2048 +- 1"), (2049, "forward 2048 +- 1")]
    fwd += [(x, "mismatch in every byte of a lane") for x in range(32, 48)]
    for x, edge in fwd:
        a = 320
        target = fill_before(10, 7, B, a) + B[a:a + 16 + x] + fill_after(40, 8 + x, B, a + 16 + x)
        out.append(_one("forward %d" % x, [edge], B, target, lambda t, d, x=x: [m["L"] for m in t["matches"]] == [16 + x] and t["matches"][0]["e"] == 0))
    # -- backward
    # (the first whole block of a copied region is always found, so e < 16 - unless it has lost its slot to a lower block:
    # `lost` has 66 such blocks in a row in front of block 566, which owns its slot)
    lost, first = _lost_base()
    for e in [0, 8, 15] + list(range(16, 32)) + [1023, 1024, 1025, 1056]:
        base, j = (B, 128) if e < 16 else (lost, first)
        a = 16 * j - e
        edges = ["backward 0 and 15"] if e in (0, 15) else ["backward stopped by a byte"] + (["mismatch in every byte of a lane"] if e < 32 else [])
        target = fill_before(1100, 9, base, a) + base[a:16 * j + 48] + fill_after(20, 10, base, 16 * j + 48)
        out.append(_one("backward %d" % e, edges, base, target,
                        lambda t, d, e=e, j=j: [(m["p"], m["j"], m["e"], m["L"]) for m in t["matches"]] == [(1100 + e, j, e, 48)]))
    # (block 0 always owns its slot, so a match that reaches the base's start is one on block 0: nothing is in front of it
    # in the base, whatever stands in front of it in the target)
    target = rnd(30, 11) + B[0:100] + fill_after(10, 12, B, 100)
    out.append(_one("backward to the base's start", ["backward stopped by the base's start"], B, target,
                    lambda t, d: [(m["p"], m["j"], m["e"], m["lit"]) for m in t["matches"]] == [(30, 0, 0, 0)]))
    # (the 8 bytes in front of the second region are also the 8 bytes that end the first copy)
    X = rnd(8, 13)
    base = B[:56] + X + B[64:992] + X + B[1000:2000]
    base = base[:64] + _not(base[1000]) + base[65:]  # (the first copy ends at 64)
    target = base[0:64] + base[1000:1080] + fill_after(10, 14, base, 1080)
    out.append(_one("backward to lit", ["backward stopped by lit"], base, target,
                    lambda t, d: [(m["p"], m["j"], m["e"], m["lit"]) for m in t["matches"]] == [(0, 0, 0, 0), (72, 63, 8, 64)]))
    # -- copy sizes and the one-byte op
    big = rnd(0x20000 + 64, 15)
    for size in (0xFFFF, 0x10000, 0x10001, 0x20000):
        target = fill_before(5, 16, big, 32) + big[32:32 + size] + fill_after(5, 17, big, 32 + size)
        want = [("insert", 5)] + [("copy", 32 + i, min(0x10000, size - i)) for i in range(0, size, 0x10000)] + [("insert", 5)]
        out.append(_one("a copy of 0x%x" % size, ["copies 0xffff 0x10000 0x10001 0x20000"], big, target, lambda t, d, want=want: _ops(t) == want))
    target = big[0:0x10000] + fill_after(3, 18, big, 0x10000)
    out.append(_one("offset 0, size 0x10000", ["one-byte copy op", "offsets 0 0x100 0x10000"], big, target,
                    lambda t, d: _ops(t) == [("copy", 0, 0x10000), ("insert", 3)] and d[6:] == b"\x80\x03" + t["ops"][1][1]))
    parts, want = [], []
    for a in (0x100, 0x10000):
        parts.append(fill_before(4, 19 + a, big, a) + big[a:a + 40] + fill_after(4, 20 + a, big, a + 40))
        want += [("insert", 4 if not want else 8), ("copy", a, 40)]
    out.append(_one("offsets 0x100 0x10000", ["offsets 0 0x100 0x10000"], big, b"".join(parts), lambda t, d, want=want: _ops(t) == want + [("insert", 4)]))
    far = rnd(0x1000000 + 4096, 21)
    parts, want = [], []
    for a in (0x1000000, 0x00FF00FF):
        parts.append(fill_before(4, 22 + a, far, a) + far[a:a + 40] + fill_after(4, 23 + a, far, a + 40))
        want += [("insert", 4 if not want else 8), ("copy", a, 40)]
    out.append(_one("far offsets", ["offsets 0x1000000 0x00ff00ff"], far, b"".join(parts),
                    lambda t, d, want=want: _ops(t) == want + [("insert", 4)] and t["k"] == 22 and b"\x98\x01\x28" in d and b"\x95\xff\xff\x28" in d))
    # -- insert runs
    for run in (126, 127, 128, 254, 255):
        target = fill_before(run, 24 + run, B, 480) + B[480:560] + fill_after(run, 25 + run, B, 560)
        ins = [("insert", 127)] * (run // 127) + ([("insert", run % 127)] if run % 127 else [])
        out.append(_one("inserts of %d" % run, ["inserts 126 127 128 254 255"], B, target, lambda t, d, ins=ins: _ops(t) == ins + [("copy", 480, 80)] + ins))
    # -- the two varints
    long = rnd(16400, 26)
    for nb, nt, edge in ((127, 128, "varints 127 128"), (128, 127, "varints 127 128"), (16383, 16384, "varints 16383 16384"),
                         (16384, 16383, "varints 16383 16384")):
        out.append(_one("varints %d %d" % (nb, nt), [edge], long[:nb], long[:nt],
                        lambda t, d, nb=nb, nt=nt: d.startswith(dm.varint(nb) + dm.varint(nt)) and len(dm.varint(nb) + dm.varint(nt)) == sum(
                            1 + (v > 127) + (v > 16383) for v in (nb, nt))))
    # -- the table
    lo = hi = None
    for seed in range(27, 200):
        base = rnd(1024, seed)
        slots = [dm.slot_of(base[16 * j:16 * j + 16], 10) for j in range(64)]
        dup = [(slots.index(s), j) for j, s in enumerate(slots) if slots.index(s) != j]
        if dup:
            lo, hi = dup[0]
            break
    target = rnd(20, 300) + base[16 * hi:16 * hi + 16] + rnd(20, 301) + base[16 * lo:16 * lo + 16] + rnd(20, 302)
    out.append(_one("two blocks in one slot", ["two blocks in one slot"], base, target,
                    lambda t, d, lo=lo, hi=hi: lo < hi and [m["j"] for m in t["matches"]] == [lo] and t["matches"][0]["p"] == 56))
    taken = {dm.slot_of(base[16 * j:16 * j + 16], 10) for j in range(64)}
    blk = next(b for b in (rnd(16, s) for s in range(400, 2000)) if dm.slot_of(b, 10) in taken)
    out.append(_one("an occupied slot, other bytes", ["occupied slot, other bytes"], base, rnd(20, 303) + blk + rnd(20, 304),
                    lambda t, d, blk=blk: not t["matches"] and dm.slot_of(blk, 10) in taken))
    blk = rnd(16, 305)
    out.append(_one("one repeated block", ["one repeated block"], blk * 100, rnd(9, 306)[:-1] + _not(blk[15]) + blk * 10 + _not(blk[0]) + rnd(9, 307),
                    lambda t, d: _ops(t) == [("insert", 9), ("copy", 0, 160), ("insert", 10)]))
    for blocks in (512, 513):
        base = rnd(16 * blocks + 7, 308)
        out.append(_one("%d blocks" % blocks, ["k 10 and 11"], base, fill_before(3, 309, base, 16 * 511) + base[16 * 511:],
                        lambda t, d, blocks=blocks: t["k"] == (10 if blocks == 512 else 11)))
    # -- several pairs over shared buffers: versions v0 <- v1 <- v2 and v0 <- v3
    v0 = rnd(3000, 310)
    v1 = v0[:1000] + rnd(30, 311) + v0[1000:]
    v2 = v1[:200] + v1[260:] + rnd(40, 312)
    v3 = rnd(10, 313) + v0
    out.append({"name": "versions", "edges": {"several targets on one base", "a base that is a target"}, "bufs": [v0, v1, v2, v3],
                "pairs": [(0, 1), (1, 2), (0, 3), (0, 0)], "claim": lambda tr, dl: all(len(t["matches"]) >= 1 for t in tr) and max(len(d) for d in dl) < 120})
    assert set().union(*[c["edges"] for c in out]) == DELTA_EDGES
    return out


def delta_model(case):
    """-> (traces, deltas) of a case's pairs"""
    made = [dm.make_delta(case["bufs"][b], case["bufs"][t]) for b, t in case["pairs"]]
    return [m[1] for m in made], [m[0] for m in made]


def laid_out(cases):
    """every buffer of every case once in one blob, buffer k at an address that is ALIGNMENTS[k mod 5] mod 16, the gaps (never
    empty) 0xff -> (blob, [(base_off, base_len, tgt_off, tgt_len)] over all pairs, [(case number, pair number)])"""
    blob, rows, who, k = bytearray(), [], [], 0
    for ci, c in enumerate(cases):
        at = []
        for b in c["bufs"]:
            blob += b"\xff"
            blob += b"\xff" * ((ALIGNMENTS[k % len(ALIGNMENTS)] - len(blob)) % 16)
            at.append(len(blob))
            blob += b
            k += 1
        for pi, (b, t) in enumerate(c["pairs"]):
            rows.append((at[b], len(c["bufs"][b]), at[t], len(c["bufs"][t])))
            who.append((ci, pi))
    return bytes(blob), rows, who


def _edit(data, seed, edits=3):
    """a version: `edits` small edits (a replacement, an insertion, a deletion) at random places"""
    rng = np.random.default_rng(seed)
    out = bytearray(data)
    for k in range(edits):
        at = int(rng.integers(0, len(out) - 40))
        new = rng.integers(32, 127, int(rng.integers(1, 24)), dtype=np.uint8).tobytes()
        if k % 3 == 0:
            out[at:at + len(new)] = new
        elif k % 3 == 1:
            out[at:at] = new
        else:
            del out[at:at + len(new)]
    return bytes(out)


def version_chains(chains=40, depth=8, size=5600):
    """objects and bases: `chains` chains of `depth` versions of slices of the corpus's book1, three small edits a version"""
    from decompress_amd import workloads
    book = workloads.corpus()["book1"]
    objects, bases = [], []
    for c in range(chains):
        cur = book[c * 17011 % (len(book) - size):][:size]
        for v in range(depth):
            bases.append(None if v == 0 else len(objects) - 1)
            objects.append((3, cur))
            cur = _edit(cur, 1000 * c + v)
    return objects, bases


def _ofs_pair(want, level):
    """two blobs, the second a kept delta against the first, at a distance of exactly `want` bytes"""
    seedling = rnd(want + 64, 500 + want)
    for n in range(want - 8, max(want - 300, 64), -1):
        base = seedling[:n]
        objects = [(3, base), (3, base + b"and a tail that is new")]
        m = dm.write_pack(objects, [None, 0], level=level)
        if m["keep"][1] and m["entries"][1]["offset"] - m["entries"][0]["offset"] == want:
            return objects
    raise AssertionError("no pair at distance %d" % want)


def _typed_objects():
    """a commit, a tree, a blob and a tag that `git index-pack --strict` takes - well-formed, and everything they name is in
    the pack -, then a second version of each"""
    from tests import pack_writer as pw
    text = np.random.default_rng(640).integers(97, 123, 300, dtype=np.uint8).tobytes()
    who = b"A U Thor <author@example.com> 1700000000 +0000"
    blob, blob2 = text, text[:150] + b" and more " + text[150:]
    entry = lambda name, data: b"100644 " + name + b"\0" + pw.object_name(3, data)
    tree = b"".join(entry(b"f%03d" % i, blob) for i in range(12))
    tree2 = tree + entry(b"g", blob2)
    commit = b"tree " + pw.object_name(2, tree).hex().encode() + b"\nauthor " + who + b"\ncommitter " + who + b"\n\n" + text + b"\n"
    commit2 = (b"tree " + pw.object_name(2, tree2).hex().encode() + b"\nparent " + pw.object_name(1, commit).hex().encode() + b"\nauthor " + who +
               b"\ncommitter " + who + b"\n\n" + text + b"\n")
    tag = b"object " + pw.object_name(1, commit).hex().encode() + b"\ntype commit\ntag v1\ntagger " + who + b"\n\n" + text + b"\n"
    tag2 = b"object " + pw.object_name(1, commit2).hex().encode() + b"\ntype commit\ntag v2\ntagger " + who + b"\n\n" + text + b"\n"
    return [(1, commit), (2, tree), (3, blob), (4, tag), (1, commit2), (2, tree2), (3, blob2), (4, tag2)]


@functools.lru_cache(maxsize=None)
def pack_cases():
    out = []
    B = rnd(4000, 600)
    # -- the keep bound: a copy and a run of new bytes, the run as long as it takes
    exact = over = None
    for nt in range(2000, 2040):
        for r in range(nt // 2 - 60, nt // 2):
            target = B[:nt - r] + rnd(r, 601)
            n = len(dm.make_delta(B, target)[0])
            if n == dm.delta_cap(nt) and exact is None:
                exact = target
            if n == dm.delta_cap(nt) + 1 and over is None:
                over = target
        if exact and over:
            break
    out.append({"name": "the keep bound", "edges": {"keep bound exact and one over"}, "objects": [(3, B), (3, exact), (3, over)], "bases": [None, 0, 0],
                "runs": [{}], "claim": lambda rs, exact=exact, over=over: rs[0]["keep"] == [False, True, False] and rs[0]["last"]["dropped_size"] == 1 and
                len(rs[0]["payloads"][1]) == dm.delta_cap(len(exact)) and len(dm.make_delta(B, over)[0]) == dm.delta_cap(len(over)) + 1})
    # -- a chain of 4 deltas under max_depth 1, 2 and 0
    vs = [rnd(1500, 602)]
    for k in range(4):
        vs.append(vs[-1][:300 * k + 100] + rnd(12, 603 + k) + vs[-1][300 * k + 100:])
    out.append({"name": "a chain of 4", "edges": {"max_depth 1 2 0 on a chain of 4"}, "objects": [(3, v) for v in vs], "bases": [None, 0, 1, 2, 3],
                "runs": [{"max_depth": 1}, {"max_depth": 2}, {"max_depth": 0}, {"max_depth": 50}],
                "claim": lambda rs: [r["depth"] for r in rs] == [[0, 1, 0, 1, 0], [0, 1, 2, 0, 1], [0, 1, 2, 3, 4], [0, 1, 2, 3, 4]] and
                [r["last"]["dropped_depth"] for r in rs] == [2, 1, 0, 0]})
    # -- the distance varint
    for a, b, edge in ((127, 128, "ofs varint 127 128"), (16511, 16512, "ofs varint 16511 16512")):
        for want in (a, b):
            objects = _ofs_pair(want, 6)
            out.append({"name": "a distance of %d" % want, "edges": {edge}, "objects": objects, "bases": [None, 0], "level": 6, "runs": [{}],
                        "claim": lambda rs, want=want: rs[0]["keep"] == [False, True] and rs[0]["entries"][1]["offset"] - 12 == want})
    # -- types, sizes below the limits, level 0, nothing
    out.append({"name": "every type", "edges": {"every type"}, "objects": _typed_objects(), "bases": [None] * 4 + [0, 1, 2, 3], "runs": [{}],
                "claim": lambda rs: rs[0]["keep"] == [False] * 4 + [True] * 4})
    small = rnd(200, 630)
    out.append({"name": "too small to try", "edges": {"no delta below 64 or base below 16"},
                "objects": [(3, small[:15]), (3, small[:15] + small[:60]), (3, small[:64]), (3, small[:63]), (3, small[:16]), (3, small[:16] * 4), (3, b"")],
                "bases": [None, 0, None, 2, None, 4, None], "runs": [{}],
                "claim": lambda rs: rs[0]["last"]["pairs"] == 1 and rs[0]["keep"] == [False] * 5 + [True, False] and len(rs[0]["payloads"][5]) == 10})
    out.append({"name": "level 0", "edges": {"level 0"}, "objects": [(3, B), (3, B[:2000] + rnd(20, 631) + B[2000:])], "bases": [None, 0], "level": 0,
                "runs": [{}], "claim": lambda rs: rs[0]["keep"] == [False, True] and len(rs[0]["pack"]) > 4000})
    out.append({"name": "nothing", "edges": {"n = 0"}, "objects": [], "bases": [], "runs": [{}], "claim": lambda rs: len(rs[0]["pack"]) == 32})
    out.append({"name": "one object twice", "edges": {"equal names"}, "objects": [(3, B), (3, B)], "bases": [None, 0], "runs": [{}],
                "claim": lambda rs: rs[0]["idx"] is None and rs[0]["keep"] == [False, True]})
    objects, bases = version_chains()
    out.append({"name": "version chains", "edges": {"version chains"}, "objects": objects, "bases": bases, "runs": [{}, {"deltas": False}],
                "claim": lambda rs: rs[0]["last"]["kept"] >= 0.9 * rs[0]["last"]["pairs"] and rs[0]["last"]["pairs"] == 280 and
                len(rs[0]["pack"]) < len(rs[1]["pack"]) / 2})
    assert set().union(*[c["edges"] for c in out]) == PACK_EDGES
    return out


@functools.lru_cache(maxsize=None)
def pack_model(name, level=6):
    """the model's results of a case's runs at a level (the case's own level wins), computed once"""
    c = next(c for c in pack_cases() if c["name"] == name)
    return tuple(dm.write_pack(c["objects"], c["bases"], level=c.get("level", level), **run) for run in c["runs"])
