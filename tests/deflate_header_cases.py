"""Hand-built dynamic block headers for the inflate kernels' header parser (dynamic_tables, build_walk, canon_counts in
csrc/inflate_wave_core.hpp): families of small raw streams, each `(name, raw, cap, expected reason tag)`.  The tag is
the rule of tests/deflate_header_model.py the case is named for ("ok": a valid header; None: whatever comes first, the
truncation family).  tests/test_deflate_headers.py proves on the CPU that every stream reaches its rule;
tests/test_gpu_inflate_headers.py runs them through the kernels.

Every header of H1-H3 comes in two placings: " /mid" has more than 1024 bytes of stored blocks behind it, so the
header's run-length loop takes its unchecked form (PLENTY bits of input left); " /end" is the stream's last block with
a few tokens behind the header, so the checked form runs.  100 stored bytes lie in front (33 000 where a body needs far
distances), so "the bytes in front of the failing block" shows in out_len.

H1 code shapes, H2 header layout, H3 invalid headers, H4 truncation at every byte, H5 one-code blocks.  What RFC 1951
cannot express as a VALID header is listed where it is asked for: HCLEN = 4 (only 16, 17, 18 and 0 have codes: no
end-of-block length) and an 18 of 138 that ends at hlit + hdist (at most 63 lengths follow symbol 256) are no_eob cases."""
import copy
import functools
import os
import random
import re

from tests import deflate_header_model as model
from tests.deflate_tokens import DB, DX, LB, LX
from tests.deflate_writer import CL_ORDER, FIXED_DIST, FIXED_LIT, Bits, Block, _rle, canonical, match, write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _geometry():
    csrc = os.path.join(ROOT, "decompress_amd", "csrc")
    with open(os.path.join(csrc, "inflate_wave_core.hpp")) as f:
        core = f.read()
    with open(os.path.join(csrc, "inflate_wave.hip")) as f:
        wave = f.read()
    a, b, c = re.search(r"plenty = .*>= (\d+) \* (\d+) \+ (\d+);", core).groups()
    return (int(re.search(r"constexpr uint32_t KMAX = (\d+);", core).group(1)),
            int(re.search(r"#define MD_STAGE (\d+)", wave).group(1)), int(a) * int(b) + int(c))


KMAX, STAGE, PLENTY = _geometry()  # steps of a budget walk; staging bytes; input bits that switch the checks off
UNBOUNDED = {}  # name -> bytes in front of the standing point, of the streams that never end (H5)


# ---- code lengths -------------------------------------------------------------------------------
def complete_code(n, maxbits, rng):
    """n code lengths of a complete code whose longest code has `maxbits` bits"""
    assert maxbits + 1 <= n <= 1 << maxbits or (maxbits, n) == (1, 2)
    ls = list(range(1, maxbits)) + [maxbits, maxbits]
    while len(ls) < n:
        i = rng.choice([i for i, l in enumerate(ls) if l < maxbits])
        ls[i] += 1
        ls.append(ls[i])
    return ls


def from_hist(hist):
    """the lengths of a histogram: hist[k] codes of k + 1 bits"""
    return [k + 1 for k, c in enumerate(hist) for _ in range(c)]


def spread(ls, size, must, rng):
    """the lengths `ls` on `size` symbols: `must` get one each, the rest go to random symbols"""
    syms = [s for s in range(size) if s not in must]
    rng.shuffle(syms)
    syms = sorted(list(must) + syms[:len(ls) - len(must)])
    ls = list(ls)
    rng.shuffle(ls)
    out = [0] * size
    for s, l in zip(syms, ls):
        out[s] = l
    return out


# ---- bodies ---------------------------------------------------------------------------------------
def length_of(ls, lext):
    i = ls - 257
    return LB[i] + lext if i < 28 else 258 if i == 28 else 3


def body(lit, dist, have):
    """tokens that use every symbol with a code: each literal; each length symbol with its extra bits all zero and all
    one; each distance symbol (below 30) likewise, where the output so far reaches that far"""
    toks, n = [], have
    for s in range(256):
        if lit[s]:
            toks.append(s)
            n += 1
    lsyms = [s for s in range(257, len(lit)) if lit[s]]
    dsyms = [s for s in range(min(30, len(dist))) if dist[s]]
    if not lsyms or not dsyms:
        return toks
    k = 0

    def add(ls, lext, ds, dext):
        nonlocal n
        ln = length_of(ls, lext)
        toks.append(match(ln, DB[ds] + dext, lsym=ls, lext=lext, dsym=ds, dext=dext))
        n += ln

    for ls in lsyms:
        lx = LX[ls - 257] if ls < 285 else 0
        for lext in sorted({0, (1 << lx) - 1}):
            near = [d for d in dsyms if DB[d] <= min(n, 32768)]
            if not near:
                break
            ds = near[k % len(near)]
            k += 1
            add(ls, lext, ds, min((1 << DX[ds]) - 1, min(n, 32768) - DB[ds]) if k & 1 else 0)
    for ds in dsyms:
        for dext in sorted({0, (1 << DX[ds]) - 1}):
            if DB[ds] + dext <= min(n, 32768):
                ls = lsyms[k % len(lsyms)]
                k += 1
                add(ls, 0, ds, dext)
    return toks


def raw_code(lens, sym):
    """the code of `sym` as raw bits (for a token the writer cannot finish: a length symbol whose distance is hand-made)"""
    code, n = canonical(lens)[sym]
    return Bits(int(format(code, "0%db" % n)[::-1], 2), n)


def _stored(rng, n):
    out = []
    while n > 0:
        k = min(n, 65535)
        out.append(Block("stored", [rng.randrange(256) for _ in range(k)]))
        n -= k
    return out


def _out_len(raw):
    return len(model.inflate(raw, 1 << 30).output)


def _two(rng, name, blk, tag, front=100, cap=None, few=24):
    """the two placings of one block; at the end of the stream only its first `few` tokens follow the header.
    cap None: what the stream produces (a failing one: the bytes in front + 16)"""
    cases = []
    for placing in ("mid", "end"):
        if placing == "end" and len(blk.tokens) > few:
            blk = copy.copy(blk)
            blk.tokens = blk.tokens[:few]
        blocks = _stored(rng, front) + [blk]
        if placing == "mid":
            blocks = blocks + _stored(rng, 600) + _stored(rng, 600)
        raw = write(blocks)
        c = cap if cap is not None else (_out_len(raw) if tag == "ok" else front + 16)
        cases.append(("%s /%s" % (name, placing), raw, c, tag))
    return cases


def dyn(lit, dist, toks=None, have=100, **kw):
    """a dynamic block with these code lengths and (unless given) the body that uses every code"""
    return Block("dynamic", body(lit, dist, have) if toks is None else toks, lit_lens=list(lit), dist_lens=list(dist), **kw)


# ---- H1: code shapes ------------------------------------------------------------------------------
# The largest literal/length tables a search over length histograms found (annealing with random restarts that moves one
# leaf pair at a time, need computed by model.table_need): see family_h3's docstring for where it ended.
LIT_840 = [1, 0, 2, 0, 1, 0, 3, 7, 0, 129, 65, 25, 17, 32, 4]
LIT_BEST = {286: [1, 1, 1, 0, 0, 0, 0, 0, 0, 77, 41, 97, 33, 33, 2], 287: [1, 1, 0, 1, 1, 0, 0, 0, 0, 113, 53, 49, 65, 1, 2],
            288: [1, 1, 1, 0, 0, 1, 1, 0, 0, 73, 13, 65, 33, 33, 66]}  # 852 entries each
LIT_854 = [1, 1, 1, 0, 0, 0, 0, 0, 0, 67, 93, 41, 17, 1, 66]  # 288 symbols, 854 entries: more than the table has
DIST_592 = [1, 1, 1, 0, 0, 1, 9, 9, 1, 1, 1, 1, 1, 1, 2]
DIST_594 = {31: [1, 1, 1, 0, 0, 0, 11, 9, 1, 1, 1, 1, 1, 1, 2], 32: [1, 1, 0, 2, 0, 0, 11, 9, 1, 1, 1, 1, 1, 1, 2]}
NEAR_DIST = [2, 2, 2, 3, 3]                                  # distances 1..6: reachable behind 100 bytes
FEW_LIT = dict(((97, 2), (98, 2), (256, 3), (257, 3), (258, 3), (265, 3)))


PAD = (Bits(0, 16),)  # behind a header without a body: the reference wants the longest code's bits before it looks at a code


def _lit(table, size=None):
    out = [0] * (size or max(table) + 1)
    for s, l in table.items():
        out[s] = l
    return out


@functools.lru_cache(None)
def family_h1():
    rng = random.Random(1101)
    cases = []
    for m in range(1, 16):  # literal/length codes by their longest code: no sub-tables up to 9 bits, then widths 1..6
        n = 2 if m == 1 else min(286, 1 << m)
        must = (256,) if m == 1 else (256, 257, 264 + m) if n >= 8 else (256, 257)
        lit = spread(complete_code(n, m, rng), 286, must, rng)
        cases += _two(rng, "H1 lit longest %d" % m, dyn(lit, NEAR_DIST), "ok")
    cases += _two(rng, "H1 lit 840 entries", dyn(spread(from_hist(LIT_840), 286, (256, 285), rng), NEAR_DIST), "ok")
    for nsym in (286, 287, 288):
        lit = spread(from_hist(LIT_BEST[nsym]), nsym, (256, nsym - 1), rng)
        cases += _two(rng, "H1 lit 852 entries %d symbols" % nsym, dyn(lit, NEAR_DIST, hlit=nsym), "ok")
    for seed in range(3):  # several sub-table widths in one table
        lit = spread(complete_code(286, 15, random.Random(seed)), 286, (256,), rng)
        cases += _two(rng, "H1 lit mixed widths %d" % seed, dyn(lit, NEAR_DIST), "ok")
    cases += _two(rng, "H1 fixed code as dynamic", dyn(FIXED_LIT, FIXED_DIST, have=33000, hlit=288, hdist=32), "ok", front=33000)
    few = _lit(FEW_LIT)
    for m in range(1, 16):  # distance codes by their longest code
        n = 2 if m == 1 else min(30, 1 << m)
        dist = spread(complete_code(n, m, rng), 30, (0,), rng)
        cases += _two(rng, "H1 dist longest %d" % m, dyn(few, dist, have=33000), "ok", front=33000)
    cases += _two(rng, "H1 dist 592 entries", dyn(few, spread(from_hist(DIST_592), 30, (), rng), have=33000), "ok", front=33000)
    for s in (0, 1, 15, 29):  # a lone 1-bit distance code, read at its code only (H5 reads the other slot)
        dist = [0] * s + [1]
        cases += _two(rng, "H1 dist lone code on %d" % s, dyn(few, dist, have=33000, hdist=s + 1), "ok", front=33000)
    return cases


# ---- H2: header layout ----------------------------------------------------------------------------
def _rle_syms(lens):
    return [(s, v) for s, v, _ in _rle(lens)]


def _expand_syms(syms):
    out = []
    for s, v in syms:
        out += [s] if s < 16 else [out[-1] if s == 16 else 0] * (v + (11 if s == 18 else 3))
    return out


def _cl_for(syms, maxbits=None, rng=None):
    """a complete code-length code for the symbols a header uses (at least two codes)"""
    used = sorted({s for s, _ in syms})
    while len(used) < 2:
        used.append(next(s for s in range(19) if s not in used))
    m = maxbits or max(1, (len(used) - 1).bit_length())
    ls = complete_code(len(used), m, rng or random.Random(len(used))) if len(used) > 2 else [1, 1]
    cl = [0] * 19
    for s, l in zip(used, ls):
        cl[s] = l
    return cl


def spelled(lit, dist, syms, toks=None, have=100, cl_lens=None, **kw):
    """a dynamic block whose header is the given run-length symbols; they must decode to lit + dist"""
    assert _expand_syms(syms) == list(lit) + list(dist), "the symbols do not spell these lengths"
    cl = cl_lens or _cl_for(syms)
    return Block("dynamic", body(lit, dist, have) if toks is None else toks, lit_lens=list(lit), dist_lens=list(dist),
                 hlit=len(lit), hdist=len(dist), cl_lens=cl, cl_syms=syms, **kw)


def _zeros(n):
    """run-length symbols for n zeros"""
    return _rle_syms([0] * n)


def _hclen_needed(k):
    """literal/length code lengths whose header needs exactly HCLEN = k (5..19): it uses the length CL_ORDER[k - 1] and
    none of the later ones.  (2^m - 1) codes of the shortest allowed length m, then a chain down to that length."""
    v, allowed = CL_ORDER[k - 1], [x for x in CL_ORDER[3:k] if x]
    m = min(allowed)
    assert all(x in allowed for x in range(m, v + 1))
    ls = [m] * ((1 << m) - 1) + (list(range(m + 1, v)) + [v, v] if v > m else [m])
    lit = [0] * 257
    for s, l in zip([256] + list(range(len(ls) - 1)), sorted(ls)):
        lit[s] = l
    return lit


@functools.lru_cache(None)
def family_h2():
    rng = random.Random(1202)
    cases = []
    few = _lit(FEW_LIT)
    for k in range(5, 20):  # HCLEN as small as the lengths allow, and the same header with more fields than needed
        lit = _hclen_needed(k)
        blk = dyn(lit, [0])
        cases += _two(rng, "H2 hclen %d needed" % k, blk, "ok")
        if k < 19:
            cases += _two(rng, "H2 hclen %d sent as %d" % (k, min(19, k + 3)), dyn(lit, [0], hclen=min(19, k + 3)), "ok")
    # HCLEN 4: only 16, 17, 18 and 0 can have codes, so every length is 0 and the end-of-block length is missing
    z = _zeros(258)
    cases += _two(rng, "H2 hclen 4", Block("dynamic", PAD, lit_lens=[0] * 257, dist_lens=[0], hlit=257, hdist=1, hclen=4, eob=False,
                                           cl_lens=_cl_for(z), cl_syms=z), "no_eob")
    # code-length codes: two 1-bit codes; all 19 symbols in use; a 7-bit longest code
    lit8 = [0] + [8] * 256
    cases += _two(rng, "H2 cl two 1-bit codes", spelled(lit8, [0], [(l, 0) for l in lit8 + [0]]), "ok")
    lit19 = [0] * 258
    for s, l in zip([0, 2, 6] + list(range(7, 17)), range(1, 14)):
        lit19[s] = l
    lit19[256], lit19[18], lit19[257] = 14, 15, 15
    s19 = _rle_syms(lit19 + [2, 2, 2, 2])
    assert {s for s, _ in s19} == set(range(19))
    cases += _two(rng, "H2 cl all 19 symbols", spelled(lit19, [2, 2, 2, 2], s19, cl_lens=[4] * 13 + [5] * 6), "ok")
    cl7 = complete_code(19, 7, rng)
    rng.shuffle(cl7)
    cases += _two(rng, "H2 cl 7-bit longest code", spelled(lit19, [2, 2, 2, 2], s19, cl_lens=cl7), "ok")
    # HLIT / HDIST corners and inner points
    for hlit, hdist in ((257, 1), (257, 32), (286, 30), (287, 31), (288, 32), (288, 1), (270, 10), (260, 29), (258, 2)):
        lit = _lit({97: 1, 256: 2, (hlit - 1 if hlit > 257 else 98): 2}, hlit)
        dist = [0] * hdist
        if hlit > 257:
            dist[0] = 1
            dist[hdist - 1] = 1  # (HDIST 1: a lone code)
        cases += _two(rng, "H2 hlit %d hdist %d" % (hlit, hdist), dyn(lit, dist, have=33000, hlit=hlit, hdist=hdist), "ok", front=33000)
    # runs
    lit = _lit({97: 2, 98: 2, 256: 2, 257: 2})
    syms = _zeros(97) + [(2, 0), (2, 0)] + _zeros(157) + [(2, 0), (16, 2)]
    cases += _two(rng, "H2 run 16 across hlit", spelled(lit, [2, 2, 2, 2], syms), "ok")
    lit = _lit({97: 1, 256: 2, 257: 2}, 260)
    syms = _zeros(97) + [(1, 0)] + _zeros(158) + [(2, 0), (2, 0), (17, 1), (1, 0), (1, 0)]
    cases += _two(rng, "H2 run 17 across hlit", spelled(lit, [0, 0, 1, 1], syms), "ok")
    lit = _lit({97: 1, 256: 2, 257: 2}, 270)
    syms = _zeros(97) + [(1, 0)] + _zeros(158) + [(2, 0), (2, 0), (18, 5), (1, 0), (1, 0)]
    cases += _two(rng, "H2 run 18 across hlit", spelled(lit, [0, 0, 0, 0, 1, 1], syms), "ok")
    lit = _lit({97: 1, 256: 2, 257: 2})
    syms = [(18, 80), (16, 3), (1, 0), (17, 7), (16, 3), (18, 127), (16, 1), (2, 0), (2, 0), (1, 0), (1, 0)]
    cases += _two(rng, "H2 run 16 after 17 and 18", spelled(lit, [1, 1], syms), "ok")
    lit = _lit({97: 1, 256: 2, 98: 2}, 288)
    syms = _zeros(97) + [(1, 0), (2, 0)] + _zeros(157) + [(2, 0), (18, 63 - 11)]
    cases += _two(rng, "H2 run 18 ends at hlit + hdist", spelled(lit, [0] * 32, syms), "ok")
    z = [(18, 120 - 11), (18, 138 - 11)]
    cases += _two(rng, "H2 run 18 of 138 ends at hlit + hdist", Block("dynamic", PAD, lit_lens=[0] * 257, dist_lens=[0], hlit=257, hdist=1,
                                                                      eob=False, cl_lens=_cl_for(z), cl_syms=z), "no_eob")
    lit = _lit({253: 2, 254: 2, 255: 2, 256: 2})
    cases += _two(rng, "H2 run ends at 256", spelled(lit, [0], _zeros(253) + [(2, 0), (16, 0), (0, 0)]), "ok")
    lit = _lit({255: 2, 256: 2, 257: 2, 258: 2})
    cases += _two(rng, "H2 run starts at 256", spelled(lit, [1, 1], _zeros(255) + [(2, 0), (16, 0), (1, 0), (1, 0)]), "ok")
    # the longest valid header: 320 lengths sent singly with 7-bit codes, HCLEN 19; and the shortest one found
    cl = [0] * 19
    cl[16], cl[17], cl[18] = 1, 2, 3
    for s in range(16):
        cl[s] = 7
    lens = FIXED_LIT + FIXED_DIST
    cases += _two(rng, "H2 longest header", spelled(FIXED_LIT, FIXED_DIST, [(l, 0) for l in lens], have=33000, cl_lens=cl), "ok", front=33000)
    cases += _two(rng, "H2 shortest header", dyn([0] * 256 + [1], [0]), "ok")
    return cases


# ---- H3: invalid headers ----------------------------------------------------------------------------
def _bad(lit, dist, **kw):
    """a block whose header is wrong: no body (its codes may not be codes at all)"""
    return Block("dynamic", PAD, lit_lens=list(lit), dist_lens=list(dist), eob=False, **kw)


@functools.lru_cache(None)
def family_h3():
    """One stream per reason tag, the Kraft cases, the table-size verdicts, overshooting runs, two faults in one header.

    Literal/length table over 852 entries: FOUND, with 288 symbols.  Annealing over complete length histograms (one leaf
    pair moved at a time, random restarts, need by deflate_header_model.table_need) reached 852 entries with 286 and
    with 287 symbols (zlib's own bound for 286) and nothing above it there; with 288 symbols it reached 854 entries
    (LIT_854), the largest need found.  So only HLIT = 288 can overflow the literal/length table, by two entries."""
    rng = random.Random(1303)
    cases = []
    few, near = _lit(FEW_LIT), NEAR_DIST
    ok_syms = _rle_syms(few + near)

    def hdr(name, tag, syms, cl, lit=few, dist=near, check=True, eob=False):
        return _two(rng, name, Block("dynamic", PAD, lit_lens=list(lit), dist_lens=list(dist), hlit=len(lit), hdist=len(dist),
                                     cl_lens=cl, cl_syms=syms, cl_check=check, eob=eob), tag)

    # the code-length code
    cases += hdr("H3 cl over-subscribed", "cl_over", ok_syms, [1, 1, 1] + [0] * 16, check=False)
    cases += hdr("H3 cl incomplete", "cl_incomplete", ok_syms, [2, 2] + [0] * 17, check=False)
    for s in (0, 1, 18):
        cl = [0] * 19
        cl[s] = 1
        cases += hdr("H3 cl lone code on %d" % s, "cl_incomplete", [(s, 0)] * 4, cl)
    zero = [0] * 19
    cases += hdr("H3 cl all zero read at 1", "cl_empty_slot", [Bits(1, 1)], zero)
    cases += hdr("H3 cl all zero read at 0 then 1", "cl_empty_slot", [Bits(0, 200), Bits(1, 1)], zero)
    cases += hdr("H3 cl all zero read at 0", "no_eob", [Bits(0, len(few) + len(near))], zero)
    # the run-length rules
    rest = _rle_syms((few + near)[3:])
    cases += hdr("H3 16 first", "rep16_first", [(16, 0)] + rest, _cl_for([(16, 0)] + rest), eob=True)
    for s, v, n in ((16, 3, 6), (17, 7, 10), (18, 127, 138), (18, 0, 11)):
        lens = few + near
        syms = _rle_syms(lens[:len(lens) - n + 1]) + [(s, v)]  # the run starts n - 1 lengths before the end: one too many
        cases += hdr("H3 run %d of %d overshoots by one" % (s, n), "run_overflow", syms, _cl_for(syms))
    # the end-of-block length, Kraft sums, lone 2-bit codes
    no_eob = list(few)
    no_eob[256], no_eob[0] = 0, 3
    cases += _two(rng, "H3 no end-of-block code", _bad(no_eob, near), "no_eob")
    over = list(few)
    over[0] = 3
    cases += _two(rng, "H3 lit one leaf too many", _bad(over, near), "lit_over")
    under = list(few)
    under[265] = 0
    cases += _two(rng, "H3 lit one leaf too few", dyn(under, near), "lit_incomplete")
    cases += _two(rng, "H3 dist one leaf too many", _bad(few, near + [3]), "dist_over")
    cases += _two(rng, "H3 dist one leaf too few", dyn(few, near[:-1], toks=[97, 98, (3, 1)]), "dist_incomplete")
    big = spread(complete_code(286, 15, rng), 286, (256,), rng)
    big_over = list(big)
    big_over[next(s for s in range(286) if big[s] == 15)] = 14  # a 15-bit leaf moved up: 2^-15 too much
    cases += _two(rng, "H3 lit 15-bit code one leaf too many", _bad(big_over, near), "lit_over")
    big_under = list(big)
    big_under[next(s for s in range(256) if big[s] == 15)] = 0
    cases += _two(rng, "H3 lit 15-bit code one leaf too few", dyn(big_under, near, toks=[]), "lit_incomplete")
    d15 = spread(complete_code(30, 15, rng), 30, (), rng)
    d15_over, d15_under = list(d15), list(d15)
    d15_over[d15.index(15)] = 14
    d15_under[d15.index(15)] = 0
    cases += _two(rng, "H3 dist 15-bit code one leaf too many", _bad(few, d15_over), "dist_over")
    cases += _two(rng, "H3 dist 15-bit code one leaf too few", dyn(few, d15_under, toks=[97]), "dist_incomplete")
    cases += _two(rng, "H3 lit lone 2-bit code", dyn([0] * 256 + [2], [0], toks=[]), "lit_incomplete")
    cases += _two(rng, "H3 dist lone 2-bit code", dyn(few, [2], toks=[97, 98, (3, 1), 97]), "dist_incomplete")
    cases += _two(rng, "H3 dist lone 2-bit code on 5", dyn(few, [0] * 5 + [2], toks=[97, 98]), "dist_incomplete")
    # table sizes (D3)
    for n, hist in sorted(DIST_594.items()):
        dist = spread(from_hist(hist), n, (), rng)
        cases += _two(rng, "H3 dist 594 entries %d symbols" % n, dyn(few, dist, toks=[97, 98, (3, 2)], hdist=n), "dist_enough")
    lit = spread(from_hist(LIT_854), 288, (256, 257), rng)
    cases += _two(rng, "H3 lit 854 entries 288 symbols", dyn(lit, near, toks=[s for s in range(40) if lit[s]], hlit=288), "lit_enough")
    # two faults in one header: the first one in the reference's order is the answer
    cases += _two(rng, "H3 no end-of-block code and dist over-subscribed", _bad(no_eob, near + [3]), "no_eob")
    cases += _two(rng, "H3 no end-of-block code and lit over-subscribed", _bad([3 if s == 1 else l for s, l in enumerate(no_eob)], near), "no_eob")
    cases += _two(rng, "H3 lit over-subscribed and dist 594 entries", _bad(over, spread(from_hist(DIST_594[31]), 31, (), rng)), "lit_over")
    syms = [(16, 0)] + rest
    raw = write(_stored(rng, 100) + [Block("dynamic", (), lit_lens=few, dist_lens=near, hlit=len(few), hdist=len(near),
                                           cl_lens=_cl_for(syms), cl_syms=[(16, 0)], eob=False)])
    cut = model.inflate(raw, 1 << 20)
    assert cut.tag == "rep16_first"
    # (the writer pads the last byte with zeros; the stream ends inside the 16's extra bits or right behind them)
    cases.append(("H3 16 first and truncated /end", raw, 116, "rep16_first"))
    # the end of the input in every field of a header (the block starts on a byte: the cuts are counted in its bits)
    front = write(_stored(rng, 100) + [Block("stored", [], last=False)])[:-5]  # (without the empty block: its 5 bytes)
    blk = write([dyn(big, near)])
    cases.append(("H3 truncated in hlit /end", front + blk[:1], 116, "eoi_at:hlit"))            # 8 bits: 3 + 5 of 14
    cases.append(("H3 truncated in the cl lengths /end", front + blk[:3], 116, "eoi_at:cl_lens"))  # 24 bits: 17 + 7
    cases.append(("H3 truncated in a cl symbol /end", front + blk[:60], 116, "eoi_at:cl_sym"))
    # 18 and 1 on 1-bit codes, HCLEN 18: the first 18 is bit 71, its 7 extra bits begin the tenth byte
    syms = [(18, 127), (18, 107), (1, 0), (1, 0)]
    cl = [0] * 19
    cl[18] = cl[1] = 1
    blk = write([Block("dynamic", (), lit_lens=[0] * 256 + [1], dist_lens=[1], hlit=257, hdist=1, cl_lens=cl, cl_syms=syms)])
    cases.append(("H3 truncated in a run's extra bits /end", front + blk[:9], 116, "eoi_at:rep_extra"))
    cases.append(("H3 not truncated in a run's extra bits /end", front + blk, 100, "ok"))
    return cases


# ---- H4: truncation ---------------------------------------------------------------------------------
H4_PICK = ("H1 lit longest 15 /end", "H1 dist longest 15 /end", "H1 fixed code as dynamic /end", "H1 dist lone code on 29 /end",
           "H2 hclen 19 needed /end", "H2 cl all 19 symbols /end", "H2 run 16 after 17 and 18 /end", "H2 shortest header /end",
           "H2 hlit 288 hdist 32 /end", "H3 16 first /end", "H3 run 18 of 138 overshoots by one /end", "H3 cl all zero read at 0 /end",
           "H3 dist 594 entries 32 symbols /end", "H3 no end-of-block code and dist over-subscribed /end")


@functools.lru_cache(None)
def family_h4():
    """headers of H1-H3 cut at every byte from the block's first byte to three bytes behind the header's end"""
    pool = {c[0]: c for c in family_h1() + family_h2() + family_h3()}
    cases = []
    for name in H4_PICK:
        _, raw, cap, _ = pool[name]
        info = model.inflate(raw, 1 << 20).info
        first = info["start"] >> 3
        if first > 1000:  # a long front: the cut streams begin at the block instead (it starts on a byte)
            raw, cap = raw[first:], 16
            info = model.inflate(raw, 1 << 20).info
            first = 0
        last = min(len(raw), ((info.get("end", 8 * len(raw)) + 7) >> 3) + 3)
        for k in range(first, last + 1):
            cases.append(("H4 %s cut at %d" % (name[:-5], k - first), raw[:k], cap, None))
    return cases


# ---- H5: one-code blocks ----------------------------------------------------------------------------
H5_LIT = _lit({97: 1, 257: 2, 256: 3, 98: 3})  # 'a' = 0, length 3 = 10, end of block = 110, 'b' = 111


@functools.lru_cache(None)
def family_h5():
    """The lone end-of-block code taken at once (Ok; a normal dynamic block follows) and read at its unused slot: the
    zero entry is literal 0 on no bits, so the stream stands still and writes zeros until the room ends - for `room`
    more bytes than lie in front.  The lone distance code read at its unused slot (distance 1 from no bits: the bit is
    the first one of the next code, which therefore begins with 1), and the empty distance table read at 0 and at 1,
    as the block's first match and behind KMAX - 1, KMAX, KMAX + 1 and 2 000 one-bit literals."""
    rng = random.Random(1505)
    cases = []
    eob_only = [0] * 256 + [1]
    few = _lit(FEW_LIT)
    for front in (0, 100, 40000):
        blocks = _stored(rng, front) + [Block("dynamic", (), lit_lens=eob_only, dist_lens=[0], last=False),
                                        Block("dynamic", body(few, NEAR_DIST, max(front, 0)) if front else [97, 98, (3, 1)],
                                              lit_lens=few, dist_lens=NEAR_DIST)]
        raw = write(blocks)
        cases.append(("H5 lone eob taken @%d" % front, raw, _out_len(raw), "ok"))
        raw = write(_stored(rng, front) + [Block("dynamic", [Bits(1, 1)], lit_lens=eob_only, dist_lens=[0], eob=False)]
                    + _stored(rng, 64))
        for room in (0, 1, 63, 64, 65, STAGE - 1, STAGE, STAGE + 1, 32768, 70000):
            name = "H5 lone eob slot @%d room %d" % (front, room)
            cases.append((name, raw, front + room, "ok"))
            UNBOUNDED[name] = front
    for k in (0, KMAX - 1, KMAX, KMAX + 1, 2000):
        head = [97] * k if k else []
        slot = [raw_code(H5_LIT, 257), 98]  # the distance slot is read at the 1 that begins 'b'
        for dist, what in (([1], "on 0"), ([0, 0, 0, 1], "on 3")):
            if k == 0:  # the block's first token: the distance reaches into the stored block in front
                blk = dyn(H5_LIT, dist, toks=slot + [97, (3, DB[len(dist) - 1])] + slot)
            else:
                blk = dyn(H5_LIT, dist, toks=head + slot + [97, (3, DB[len(dist) - 1])] + slot + [97])
            cases += _two(rng, "H5 lone dist code %s slot after %d" % (what, k), blk, "ok", few=1 << 20)
        for bit in (0, 1):
            toks = head + [raw_code(H5_LIT, 257), Bits(bit, 1), 98, 97]
            blk = dyn(H5_LIT, [0], toks=toks)
            cap = None if bit == 0 else 100 + k + 16
            for c in _two(rng, "H5 empty dist table bit %d after %d" % (bit, k), blk, "ok", cap=cap, few=1 << 20):
                cases.append(c)
    return cases


@functools.lru_cache(None)
def pieces_streams():
    """(name, raw, the byte behind the header) of four blocks without anything in front, for the streaming decoders:
    the longest header, all 19 code-length symbols, an 852-entry table of 288 symbols, a 594-entry distance table"""
    rng = random.Random(1606)
    cl = [0] * 19
    cl[16], cl[17], cl[18] = 1, 2, 3
    for s in range(16):
        cl[s] = 7
    few = _lit(FEW_LIT)
    lit19 = next(model.inflate(c[1], c[2]).info["lit_lens"] for c in family_h2() if c[0] == "H2 cl all 19 symbols /end")
    s19 = _rle_syms(lit19 + [2, 2, 2, 2])
    lit852 = spread(from_hist(LIT_BEST[288]), 288, (256, 287), rng)
    blocks = (("longest header", spelled(FIXED_LIT, FIXED_DIST, [(l, 0) for l in FIXED_LIT + FIXED_DIST], have=0, cl_lens=cl)),
              ("all 19 symbols", spelled(lit19, [2, 2, 2, 2], s19, have=0, cl_lens=[4] * 13 + [5] * 6)),
              ("852 entries", dyn(lit852, NEAR_DIST, have=0, hlit=288)),
              ("594 entries", dyn(few, spread(from_hist(DIST_594[32]), 32, (), rng), toks=[97, 98, (3, 2)], hdist=32)))
    out = []
    for name, blk in blocks:
        raw = write([blk])
        info = model.inflate(raw, 1 << 20).info
        out.append((name, raw, (info["end"] + 7) >> 3))
    return out


FAMILIES = {"H1": family_h1, "H2": family_h2, "H3": family_h3, "H4": family_h4, "H5": family_h5}
