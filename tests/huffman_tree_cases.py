"""Histograms for the deflate kernel's tree builder (tree_make_wave, tree_rle_wave, trees_wave in
csrc/deflate_kernel.hip), as command lists for De.Def.encode: families of `Case(name, cmds, plain, lit, dist)` - the
commands (literals, copy_cmd, EOB), the plaintext they inflate to, and the two histograms the encoder counts from them
(lit[256] is the 1 the encoder itself counts for the end of the block).  tests/test_huffman_trees.py proves on the CPU
that the oracle, the model (tests/huffman_tree_model.py) and libz agree on every case and that the families reach what
they are named for; tests/test_gpu_huffman_trees.py runs them through the kernel.

T1 heap sizes at the kernel's boundaries (64: the choices leave the register; 128: the DEEP merge step), T2 ties,
T3 codes deeper than 15 bits, T4 code-length codes deeper than 7 bits, T5 the run-length pass.

A histogram becomes commands this way: the literals first, then the copies with the near distances first and the long
lengths first, so every distance is in range when the family has put enough literals in front.  Where a family needs
given code LENGTHS (T4, T5) it takes counts of 2^(L - length): every Huffman tree of such counts has those lengths.

What the command lists cannot express: a literal/length tree without any symbol (the encoder counts the end of the
block itself: the smallest tree is {0, 256}); only symbol 285 used (a copy needs a byte in front: one literal
joins it); a run of zeros across 255 | 256 (256 always has a code)."""
import functools
import random
from collections import namedtuple

from tests import huffman_tree_model as model
from tests.deflate_tokens import DB, DX, LB, LX

EOB = 256
Case = namedtuple("Case", "name cmds plain lit dist")

SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 286)  # used literal/length symbols, end-of-block included
DIST_SIZES = (0, 1, 2, 29, 30)
BOUNDARIES = (64, 128, 192, 256)                                  # the run-length pass goes in steps of 64 positions
ZERO_RUNS = (1, 2, 3, 10, 11, 137, 138, 139, 255)
NONZERO_RUNS = (1, 2, 3, 4, 7, 8, 13, 14, 19, 20)
DIST_ZERO_RUNS = (1, 2, 3, 10, 11)                                # (what 30 positions hold)
FAR = {65: 6145, 66: 6145, 67: 6145, 68: 6145}                    # literals in front: 24 580 bytes, distance symbol 29 is in range


def copy_cmd(off, length):
    """De.Queue.cmd (`Copy (off, len)) - decompress_amd.de.copy_cmd (the GPU test compares the two)"""
    return 0x2000000 | ((length - 3) << 16) | (off - 1)


def build(name, lit, dist=()):
    """lit: {symbol: count} or a list, without the end-of-block symbol; dist: likewise over the 30 distance symbols"""
    if isinstance(lit, dict):
        lit = [lit.get(s, 0) for s in range(286)]
    if isinstance(dist, dict):
        dist = [dist.get(s, 0) for s in range(30)]
    lit = list(lit) + [0] * (286 - len(lit))
    dist = list(dist) + [0] * (30 - len(dist))
    assert lit[EOB] in (0, 1) and sum(lit[257:]) == sum(dist), name
    lit[EOB] = 1
    cmds = [s for s in range(256) for _ in range(lit[s])]
    plain = bytearray(cmds)
    lsyms = [s for s in range(285, 256, -1) for _ in range(lit[s])]
    dsyms = [d for d in range(30) for _ in range(dist[d])]
    for k, (ls, ds) in enumerate(zip(lsyms, dsyms)):
        i = ls - 257
        lext = (1 << LX[i]) - 1 if k & 1 else 0
        length = LB[i] + (min(lext, 30) if i == 27 else lext)  # (227 + 31 is length 258: symbol 285's)
        have = min(len(plain), 32768)
        assert DB[ds] <= have, (name, ds, have)
        d = DB[ds] + min((1 << DX[ds]) - 1 if k & 2 else 0, have - DB[ds])
        cmds.append(copy_cmd(d, length))
        if d >= length:
            plain += plain[len(plain) - d:len(plain) - d + length]
        else:
            plain += (bytes(plain[-d:]) * (length // d + 1))[:length]
    cmds.append(EOB)
    return Case(name, cmds, bytes(plain), lit, dist)


def literal_only(case):
    return not any(case.dist)


# ---- T1: heap sizes ---------------------------------------------------------------------------------------------------
SHAPES = ("equal", "two values", "distinct")


def _shape(shape, n):
    """n counts: all 1 (as the end of the block's), 2 and 3 in turn, 2, 3, 4, ..."""
    return [1] * n if shape == "equal" else [2 + (i & 1) for i in range(n)] if shape == "two values" else list(range(2, n + 2))


def _split(total, syms):
    """`total` copies over the symbols `syms`, as evenly as they go"""
    return {s: total // len(syms) + (k < total % len(syms)) for k, s in enumerate(syms)}


@functools.lru_cache(None)
def family_t1():
    rng = random.Random(2101)
    cases = []
    for n in SIZES:
        for shape in SHAPES:
            name = "T1 lit %d %s" % (n, shape)
            if n <= 257:
                syms = sorted(rng.sample(range(256), n - 1))
                cases.append(build(name, dict(zip(syms, _shape(shape, n - 1)))))
            else:
                lit = dict(zip([s for s in range(286) if s != EOB], _shape(shape, 285)))
                cases.append(build(name, lit, _split(sum(lit[s] for s in range(257, 286)), (0, 1))))
    for c in (1, 2, 5):  # the only length symbol is 285 (behind the one literal a copy needs)
        cases.append(build("T1 lit only 285 x %d" % c, {65: 1, 285: c}, {0: c}))
    sets = {"0": (0,), "1": (1,), "2": (2,), "29": (29,), "0 1": (0, 1), "5 29": (5, 29),
            "all but 7": tuple(d for d in range(30) if d != 7), "all but 29": tuple(range(29)), "all": tuple(range(30))}
    for what, dsyms in sets.items():  # (no distance symbol at all: every literal-only case)
        for shape in SHAPES:
            dist = dict(zip(dsyms, _shape(shape, len(dsyms))))
            lit = dict(FAR)
            lit.update(_split(sum(dist.values()), (257, 258)))
            cases.append(build("T1 dist %d (%s) %s" % (len(dsyms), what, shape), lit, dist))
    return cases


# ---- T2: ties -----------------------------------------------------------------------------------------------------------
FIB = (1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377)
TIES = {"equal": lambda i: 100, "powers of two": lambda i: 1 << (i % 8), "fibonacci": lambda i: FIB[i % len(FIB)],
        "staircase": lambda i: i + 1}


@functools.lru_cache(None)
def family_t2():
    rng = random.Random(2202)
    cases = []
    for n in (64, 128, 286):
        for what, f in TIES.items():
            for placed in ("in order", "shuffled"):
                counts = [f(i) for i in range(n - 1)]
                if n <= 257:
                    syms = list(range(n - 1)) if placed == "in order" else sorted(rng.sample(range(256), n - 1))
                else:
                    syms = [s for s in range(286) if s != EOB]
                if placed == "shuffled":
                    rng.shuffle(counts)
                lit = dict(zip(syms, counts))
                copies = sum(c for s, c in lit.items() if s > EOB)
                cases.append(build("T2 %s %d %s" % (what, n, placed), lit, _split(copies, tuple(range(10))) if copies else ()))
    return cases


# ---- T3: too deep for 15 bits ---------------------------------------------------------------------------------------
def tie_free(n):
    """1, 2, 4, 7, 12, ...: a(k) = a(k - 1) + a(k - 2) + 1.  No sum of the smallest ones equals a count, so the tree is
    a chain whatever the heap does with ties: n of them (and the end of the block's 1) are n bits deep."""
    a = [1, 2]
    while len(a) < n:
        a.append(a[-1] + a[-2] + 1)
    return a[:n]


@functools.lru_cache(None)
def family_t3():
    rng = random.Random(2303)
    cases = []
    for n in (17, 18, 19, 20):
        a = tie_free(n)
        cases.append(build("T3 lit %d in order" % n, dict(zip(range(65, 65 + n), a))))
        syms = rng.sample(range(256), n)
        cases.append(build("T3 lit %d shuffled" % n, dict(zip(syms, a))))
    for n in (17, 18, 19):
        for k in range(2):
            a = [x + rng.randrange(2) for x in tie_free(n)]
            cases.append(build("T3 lit %d jitter %d" % (n, k), dict(zip(rng.sample(range(256), n), a))))
    for n in (17, 18):  # deep symbols among shallow ones: the order in which the leaves left the heap decides who gets 15 bits
        for k in range(2):
            syms = rng.sample(range(256), n + 8)
            a = tie_free(n) + [2000 + 37 * i for i in range(4)] + [3 + 2 * i for i in range(4)]
            rng.shuffle(a)
            cases.append(build("T3 lit %d among shallow %d" % (n, k), dict(zip(sorted(syms), a))))
    # 20 tie-free counts and three more symbols (23 with the end of the block)
    a = tie_free(20)
    cases.append(build("T3 lit 23 symbols", dict(zip(rng.sample(range(256), 22), a + [3, 9]))))
    for n in (17, 18, 19):  # the same on the length symbols (the large counts on the short lengths), distance 1
        a = tie_free(n)
        lit = dict(zip(range(257 + n - 1, 256, -1), a))
        lit[65] = 1
        cases.append(build("T3 len %d in order" % n, lit, {0: sum(a)}))
        lit = dict(zip(rng.sample(range(257, 286), n), a))
        lit.update(FAR)
        cases.append(build("T3 len %d shuffled" % n, lit, _split(sum(a), (0, 3, 11, 29))))
    for n in (17, 18, 19):  # the same on the distance symbols
        a = tie_free(n)
        lit = {65: 2000, 257: sum(a)}
        cases.append(build("T3 dist %d in order" % n, lit, dict(zip(range(n - 1, -1, -1), a))))
    for n in (17, 18):
        a = tie_free(n)
        lit = dict(FAR)
        lit[257] = sum(a)
        cases.append(build("T3 dist %d shuffled" % n, lit, dict(zip(rng.sample(range(30), n), a))))
    a = tie_free(19) + [5000]
    lit = {65: 4200}
    lit.update(_split(sum(a), (257, 260, 285)))
    cases.append(build("T3 dist 20 symbols", lit, dict(zip(rng.sample(range(24), 20), a))))
    a = tie_free(17)  # both trees at once
    lit = dict(zip(rng.sample(range(257, 286), 17), a))
    lit.update(FAR)
    cases.append(build("T3 len 17 and dist 17", lit, dict(zip(rng.sample(range(30), 17), a))))
    return cases


# ---- T4: the code-length code deeper than 7 bits ----------------------------------------------------------------------
def _counts(lens):
    """{symbol: count} whose tree has these lengths (a complete code): 2^(L - length), L the longest"""
    L = max(lens)
    assert sum(1 << (L - l) for l in lens if l) == 1 << L
    return {s: 1 << (L - l) for s, l in enumerate(lens) if l}


def _of_lengths(name, lit_lens, dist_lens=()):
    """the case whose trees have these lengths; the end of the block (count 1) has the longest literal/length code.
    Without distance lengths the copies, if any, go to distance 1."""
    lit = _counts(lit_lens)
    assert lit.pop(EOB) == 1
    copies = sum(c for s, c in lit.items() if s > EOB)
    case = build(name, lit, _counts(dist_lens) if any(dist_lens) else {0: copies} if copies else {})
    assert model.make(case.lit, 286).lengths[:len(lit_lens)] == list(lit_lens), name
    return case


def _of_dist_lengths(name, dist_lens):
    """the case whose distance tree has these lengths: its copies on length symbol 257, behind literals that put
    every distance in range"""
    dist = _counts(dist_lens)
    return build(name, {**FAR, 257: sum(dist.values())}, dist)


CL_WANTED = (4, 4)  # literal-only cases; cases whose length and distance symbols carry lengths too


@functools.lru_cache(None)
def family_t4():
    """A seeded, directed search with the model.  A complete code grows from the chain 1, 2, .., L - 1, L, L by splitting
    leaves, preferably where that keeps the number of codes growing with their length - the code-length frequencies are
    those numbers; the lengths are then scattered over the literals, so that few of them form runs.  Every other seed
    moves one code of l bits to a length symbol: its 2^(L - l) copies take the chain 1, 2, .., D, D (D = L - l)
    scattered over the distance symbols 0 .. 15, which adds to the frequencies.  Kept: the first CL_WANTED of either
    kind whose code-length tree the model finds deeper than 7 bits (a second or two of CPU)."""
    cases, seed = [], 0
    while [sum(1 for c in cases if literal_only(c) == k) for k in (True, False)] != list(CL_WANTED) and seed < 600:
        seed += 1
        rng = random.Random(seed)
        copies = seed & 1
        if sum(1 for c in cases if literal_only(c) != copies) == CL_WANTED[copies]:
            continue
        L = rng.choice((9, 10, 11, 12))
        hist = [0] + [1] * (L - 1) + [2]
        target = rng.randrange(60, 250)
        while sum(hist) < target:
            cand = [l for l in range(1, L) if hist[l]]
            l = rng.choices(cand, [1 + 3 * (hist[l] > hist[l + 1] // 2) for l in cand])[0]
            hist[l] -= 1
            hist[l + 1] += 2
        for _ in range(30):
            lens = [l for l in range(1, L + 1) for _ in range(hist[l])]
            lens.remove(L)
            rng.shuffle(lens)
            lit_lens, dist_lens = [0] * 257, [1, 1]  # (no distance symbol: 0 and 1 get a bit each)
            if copies:
                moved = next(l for l in lens if 2 <= L - l <= 11)
                lens.remove(moved)
                lit_lens = [0] * rng.randrange(258, 287)
                lit_lens[-1] = moved
                chain = list(range(1, L - moved + 1)) + [L - moved]
                rng.shuffle(chain)
                dist_lens = [0] * 16
                for p, l in zip(rng.sample(range(16), len(chain)), chain):
                    dist_lens[p] = l
                while not dist_lens[-1]:
                    dist_lens.pop()
            for p, l in zip(sorted(rng.sample(range(256), len(lens))), lens):
                lit_lens[p] = l
            lit_lens[EOB] = L
            if model.make(model.scan(lit_lens, dist_lens), 19, 7).limited:
                name = "T4 cl seed %d longest %d, %d symbols%s" % (seed, L, sum(hist), " with copies" * copies)
                cases.append(_of_lengths(name, lit_lens, dist_lens if copies else ()))
                break
    return cases


# ---- T5: the run-length pass ------------------------------------------------------------------------------------------
def _isolated(lo, hi, taken):
    """odd positions in [lo, hi) with no taken position next to them"""
    return [p for p in range(lo | 1, hi, 2) if not any(q in taken for q in (p - 1, p, p + 1))]


def _fill(units, L):
    """lengths below L that fill `units` leaves of L bits: one code per set bit"""
    return [L - k for k in range(1, L) if units >> k & 1]


def lit_run(start, n, L=12):
    """literal/length code lengths with a run of n codes of L bits at [start, start + n); the end of the block has L bits
    too, one more code makes their number even, codes of distinct shorter lengths complete the code, every one of them
    between two zeros"""
    size = max(257, start + n)
    lens = [0] * size
    for p in range(start, start + n):
        lens[p] = L
    assert start + n - 1 != 255 and start != 257
    lens[EOB] = L
    taken = set(range(start, start + n)) | {EOB}
    free = _isolated(0, 255, taken)
    longest = sum(1 for l in lens if l == L)
    rest = ([L] if longest & 1 else []) + _fill((1 << L) - longest - (longest & 1), L)
    for p, l in zip(free[::3], rest):
        lens[p] = l
    return lens


def lit_zero_run(start, n):
    """literal/length code lengths with a run of n zeros at [start, start + n) between two codes: the chain 1, 2, .., L, L
    over at most 11 symbols"""
    assert start + n <= 256
    bounds = [p for p in (start - 1, start + n) if 0 <= p < 256]
    taken = set(range(start - 1, start + n + 1)) | {EOB}
    syms = bounds + _isolated(0, 255, taken)[::5][:11 - len(bounds)]
    L = len(syms)
    lens = [0] * 257
    lens[EOB] = L
    for p, l in zip(syms, [L] + list(range(L - 1, 0, -1))):
        lens[p] = l
    return lens


def dist_run(end, n):
    """30 distance code lengths with a run of n codes of 5 bits that ends at `end`, the last one used"""
    L, start = 5, end - n + 1
    lens = [0] * (end + 1)
    for p in range(start, end + 1):
        lens[p] = L
    rest = ([L] if n & 1 else []) + _fill((1 << L) - n - (n & 1), L)
    free = [p for p in range(0, start - 1, 2)]
    assert len(free) >= len(rest), (end, n)
    for p, l in zip(free, rest):
        lens[p] = l
    return lens


def dist_zero_run(end, n):
    """distance code lengths with n zeros in front of `end`, the last code, behind the chain 1, 2, .., L, L"""
    start = end - n
    syms = [end] + ([start - 1] if start > 0 else []) + [p for p in range(0, start - 2, 2)][:3]
    assert len(syms) >= 2
    L = len(syms) - 1
    lens = [0] * (max(syms) + 1)
    for p, l in zip(syms, [L, L] + list(range(L - 1, 0, -1))):
        lens[p] = l
    return lens


def runs_of(lens):
    """[(value, start, length)] of the maximal runs"""
    out = []
    for p, l in enumerate(lens):
        if out and out[-1][0] == l:
            out[-1][2] += 1
        else:
            out.append([l, p, 1])
    return [tuple(r) for r in out]


def straddles(start, n, b):
    """a run across b - 1 | b (a single position: on either side of it)"""
    return start in (b - 1, b) if n == 1 else start <= b - 1 and start + n > b


@functools.lru_cache(None)
def family_t5():
    cases = []
    for n in NONZERO_RUNS:
        for b in BOUNDARIES:
            if n == 1 and b == 256:
                continue  # (the end of the block's own code, wherever 255 has none)
            for start in ((b - 1, b) if n == 1 else (b - (n + 1) // 2,)):
                cases.append(_of_lengths("T5 lit run of %d at %d" % (n, start), lit_run(start, n)))
        cases.append(_of_lengths("T5 lit run of %d ends at 256" % n, lit_run(257 - n, n)))
        cases.append(_of_lengths("T5 lit run of %d ends at 285" % n, lit_run(286 - n, n)))
    for n in ZERO_RUNS:
        for b in BOUNDARIES[:3]:
            for start in ((b - 1, b) if n == 1 else (max(1, min(b - (n + 1) // 2, 256 - n)),)):
                cases.append(_of_lengths("T5 lit %d zeros at %d" % (n, start), lit_zero_run(start, n)))
        cases.append(_of_lengths("T5 lit %d zeros in front of 256" % n, lit_zero_run(256 - n, n)))
    for n in NONZERO_RUNS:
        for end in sorted({29, max(n - 1, min(n + 9, 29))}):
            if n + 2 * (len(_fill(32 - n - (n & 1), 5)) + (n & 1)) <= end + 1:
                cases.append(_of_dist_lengths("T5 dist run of %d ends at %d" % (n, end), dist_run(end, n)))
    for n in DIST_ZERO_RUNS:
        for end in sorted({29, n + 4}):
            cases.append(_of_dist_lengths("T5 dist %d zeros in front of %d" % (n, end), dist_zero_run(end, n)))
    return list({c.name: c for c in cases}.values())  # (the longest runs land on the same place for several boundaries)


def libz_block(plain):
    """libz's Z_HUFFMAN_ONLY block for these bytes (trees.c is what De.T was ported from), or None where libz did not
    answer with exactly one dynamic block: more than its 32 767 symbols a block, or a stored or fixed block was cheaper"""
    import zlib
    if len(plain) > 32767:
        return None
    c = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_HUFFMAN_ONLY)
    z = c.compress(plain) + c.flush()
    return z if z[0] & 7 == 5 else None  # (the last block, dynamic)


FAMILIES = {"T1": family_t1, "T2": family_t2, "T3": family_t3, "T4": family_t4, "T5": family_t5}


def all_cases():
    return [c for f in FAMILIES.values() for c in f()]
