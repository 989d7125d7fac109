"""The batch inflate kernel (csrc/inflate_wave.hip) at the limits of its rounds, on streams written token by token
(tests/deflate_writer.py) instead of by an encoder that chooses tokens for compression.

A round ends when its record pool (RMAX match records) or its staging buffer (STAGE bytes) is full, when a zone chain
breaks, or at an end-of-block - and a block end always ends a round, so the first round of a block starts at the
block's first output byte (R0).  The families below put tokens where those limits are: full record pools of near, far
and long records; a round whose near list and long list meet (copy_far's spill); 258-byte matches that fill the
staging buffer from one lane; heads of matches that straddle R0; failures and the output cap at chosen records of a
full round; the guarded last round; distances at their edges.  RMAX and STAGE are read from the kernel's source, so a
resize keeps the streams at the limits.

Every stream is compared with expand() (the tokens replayed), the CPU oracle (status, consumed, bytes) and, when valid,
zlib and Adler-32 - under both forms of the kernel.  Each family also asserts that a profile counter of the path it
is for is non-zero, so that a family that stops reaching its path fails."""
import functools
import os
import random
import re
import zlib

import numpy as np
import pytest

from tests.deflate_writer import OK, Block, expand, match, write

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _geometry():
    with open(os.path.join(ROOT, "decompress_amd", "csrc", "inflate_wave.hip")) as f:
        src = f.read()
    get = lambda k: int(re.search(r"#define %s (\d+)" % k, src).group(1))
    return get("MD_RMAX"), get("MD_STAGE")


RMAX, STAGE = _geometry()


class _Stream:
    """blocks of one stream and the output they have produced so far"""

    def __init__(self, rng):
        self.rng, self.blocks, self.n = rng, [], 0

    def stored(self, n):
        while n > 0:
            k = min(n, 65535)
            self.blocks.append(Block("stored", [self.rng.randrange(256) for _ in range(k)]))
            self.n += k
            n -= k
        return self

    def block(self, toks, kind="dynamic", **kw):
        self.blocks.append(Block(kind, toks, **kw))
        for t in toks:
            self.n += 1 if isinstance(t, int) else t[0]
        return self

    def near(self, count, dmax=4):
        """dense 3-byte matches with distances 1..dmax: 1-bit length code, 1-2-bit distance codes"""
        return [(3, self.rng.randrange(1, dmax + 1)) for _ in range(count)]

    def far(self, at, count, lens=None):
        """matches from 6 KiB .. 32 KiB back (sources older than any round) starting at output position `at`"""
        out, q = [], at
        for _ in range(count):
            ln = self.rng.choice(lens) if lens else 3
            ln = ln if isinstance(ln, int) else self.rng.randrange(*ln)
            out.append((ln, self.rng.randrange(6145, min(q, 32768) + 1)))
            q += ln
        return out


def _case(name, s, cap=None, zlib_ok=True):
    return (name, s.blocks, s.n if cap is None else cap, zlib_ok)


# ---- A. pool-bound rounds ---------------------------------------------------------------------
@functools.lru_cache(None)
def family_a():
    rng = random.Random(101)
    cases = []
    s = _Stream(rng).stored(100)
    s.block(s.near(4 * RMAX))
    cases.append(_case("A near", s))
    for pre in (12000, 40000):  # before output 32 KiB (checked emit) and after it (the unchecked `plain` emit)
        s = _Stream(rng).stored(pre)
        s.block(s.far(s.n, 4 * RMAX))
        cases.append(_case("A far 3 @%d" % pre, s))
        s = _Stream(rng).stored(pre)
        s.block(s.far(s.n, 4 * RMAX, lens=[3] * 6 + [(17, 33)]))
        cases.append(_case("A far 17-32 @%d" % pre, s))
        s = _Stream(rng).stored(pre)
        s.block(s.far(s.n, 4 * RMAX, lens=[3] * 40 + [(17, 33), (33, 259), 258]))
        cases.append(_case("A far 33-258 @%d" % pre, s))
        s = _Stream(rng).stored(pre)
        toks, q = [], s.n
        for _ in range(4 * RMAX):  # near and far in one pool
            t = (3, rng.randrange(1, 5)) if rng.random() < 0.5 else s.far(q, 1, lens=[3, 3, (17, 33), (33, 120)])[0]
            toks.append(t)
            q += t[0]
        s.block(toks)
        cases.append(_case("A mixed @%d" % pre, s))
    return cases


# ---- B. the near list and the long list meet: copy_far's spill ---------------------------------
def _spill_block(s, rng, hs, extra_len=(1, 1)):
    """the first ~RMAX + 64 tokens of a block: short near matches with straddlers between them (source 17.. bytes
    before the block start, end after it: counted in both of copy_far's lists), as many as the staging buffer holds"""
    total = RMAX + 64
    budget = STAGE - 256
    toks, k = [], 0
    nt = int(0.3 * total)
    for i in range(total):
        if i % (total // nt) == 0 and nt:
            h = rng.choice(hs)
            ln = min(258, h + rng.randrange(*extra_len) if extra_len[1] > extra_len[0] else h + extra_len[0])
            if k + ln + 3 * (total - i) <= budget:
                toks.append((ln, k + h))
                k += ln
                continue
        toks.append((3, rng.randrange(1, 5)))
        k += 3
    return toks


@functools.lru_cache(None)
def family_b():
    rng = random.Random(202)
    cases = []
    for name, pre, hs, ext in (("B h17", 1000, [17], (1, 1)), ("B h17-24", 1000, list(range(17, 25)), (1, 3)),
                               ("B h17-250", 1000, [17] * 20 + [18, 40, 100, 250], (1, 1)),
                               ("B plain", 40000, [17, 18, 19], (1, 1))):
        s = _Stream(rng).stored(pre - 300)
        s.block([rng.randrange(256) for _ in range(300)], kind="fixed")  # a literal block
        s.block(_spill_block(s, rng, hs, ext) + s.near(2 * RMAX))
        cases.append(_case(name, s))
    return cases


# ---- C. staging-bound rounds --------------------------------------------------------------------
@functools.lru_cache(None)
def family_c():
    rng = random.Random(303)
    cases = []
    s = _Stream(rng).stored(300)
    s.block([(258, rng.randrange(1, 3)) for _ in range(600)])  # 2-bit tokens: one lane's zone overflows the buffer
    cases.append(_case("C 258 runs", s))
    for pre in (12000, 40000):
        s = _Stream(rng).stored(pre)
        toks, q = [], s.n
        for i in range(900):
            t = (258, rng.randrange(1, 3)) if (i // 7) % 3 else (258, rng.randrange(6145, min(q, 32768) + 1))
            toks.append(t)
            q += 258
        s.block(toks)
        cases.append(_case("C 258 near+far @%d" % pre, s))
        s = _Stream(rng).stored(pre)
        toks, q = [], s.n
        for i in range(2500):  # zones that shrink to SMIN, then a stretch of literals that widens them again
            t = (258, 1) if i % 500 < 300 else rng.randrange(256) if i % 500 < 420 else (rng.randrange(100, 259), rng.randrange(1, 300))
            toks.append(t)
            q += 1 if isinstance(t, int) else t[0]
        s.block(toks)
        cases.append(_case("C 258 and literals @%d" % pre, s))
    return cases


# ---- D. straddling heads at a block start ------------------------------------------------------
def _straddlers(pairs, budget=STAGE - 512):
    """(head, length) pairs -> blocks whose matches all begin before the block start and end after it"""
    blocks, cur, k = [], [], 0
    for h, ln in pairs:
        if cur and k + ln > budget:
            blocks.append(cur)
            cur, k = [], 0
        cur.append((ln, k + h))
        k += ln
    if cur:
        blocks.append(cur)
    return blocks


@functools.lru_cache(None)
def family_d():
    rng = random.Random(404)
    cases = []
    heads = list(range(1, 41)) + [41, 47, 63, 64, 65, 100, 127, 128, 129, 200, 255, 256, 257]
    pairs = []
    for h in heads:
        for ln in sorted({min(max(x, 3), 258) for x in (h + 1, h + 2, h + 7, 2 * h, 258, rng.randrange(h + 1, 259))}):
            pairs.append((h, ln))
    for h in (1, 2, 16, 17, 200):  # every length for a few heads
        pairs += [(h, ln) for ln in range(max(h + 1, 3), 259)]
    for pre, kind in ((400, "fixed"), (40000, "dynamic")):
        s = _Stream(rng).stored(pre)
        for toks in _straddlers(pairs):
            s.block(toks, kind=kind, last=False)
        s.block([], kind="fixed")
        cases.append(_case("D heads @%d %s" % (pre, kind), s))
    return cases


# ---- E. failures and the output cap inside a full round ----------------------------------------
def _full_round(rng, pre, k, bad):
    s = _Stream(rng).stored(pre)
    toks = s.near(2 * RMAX + 64)
    written = s.n + 3 * k
    if bad == "dist+1":
        toks[k] = (3, written + 1)
    elif bad in (30, 31):
        toks[k] = match(3, 1, dsym=bad)
    else:
        toks[k] = match(3, rng.randrange(1, 5), lsym=bad)
    extra = (1000 + bad,) if bad in (30, 31) else (bad,) if bad in (286, 287) else ()
    s.block(toks, extra=extra, hlit=288 if bad in (286, 287) else None, hdist=32 if bad in (30, 31) else None)
    return s


@functools.lru_cache(None)
def family_e():
    rng = random.Random(505)
    cases = []
    ks = sorted({0, 1, 63, 64, 65, RMAX // 2, RMAX - 1, RMAX, RMAX + 1})
    for k in ks:
        for bad, pres in (("dist+1", (200,)), (30, (200, 40000)), (31, (200,)), (286, (200, 40000)), (287, (200,))):
            for pre in pres:
                cases.append(_case("E %s at %d @%d" % (bad, k, pre), _full_round(rng, pre, k, bad), zlib_ok=False))
    # the output cap at every byte of a 258-byte record in the middle of a full round, and at its first and last records
    for pre in (200, 40000):
        s = _Stream(rng).stored(pre)
        toks = s.near(2 * RMAX)
        j = RMAX // 2
        toks[j] = (258, rng.randrange(1, 5))
        s.block(toks)
        at = pre + 3 * j
        for c in range(at, at + 259):
            cases.append(_case("E cap %d @%d" % (c - at, pre), s, cap=c))
        last = pre + 3 * (RMAX - 1) + 255  # where record RMAX - 1 begins
        for c in (pre, pre + 1, pre + 2, pre + 3, last, last + 1, last + 2, last + 3):
            cases.append(_case("E cap at %d @%d" % (c - pre, pre), s, cap=c))
    return cases


# ---- F. the guarded last round ------------------------------------------------------------------
@functools.lru_cache(None)
def family_f():
    rng = random.Random(606)
    cases = []
    for blen in range(1, 40):
        for pre in (3000, 36000):
            s = _Stream(rng).stored(pre)
            s.block(s.near(50), kind="fixed", last=False)
            toks, k = [], 0
            while k < blen:
                left = blen - k
                r = rng.random()
                if left < 3 or r < 0.2:
                    toks.append(rng.randrange(256))
                    k += 1
                    continue
                ln = rng.randrange(3, min(left, 258) + 1)
                if r < 0.6:
                    d = rng.randrange(ln, min(s.n, 32768) + 1)  # far
                else:
                    d = k + rng.randrange(1, min(ln, 300))  # straddles the round start (head < length)
                toks.append((ln, d))
                k += ln
            s.block(toks, kind=rng.choice(["fixed", "dynamic"]))
            for extra in (0, 1, 15):
                cases.append(_case("F %d +%d @%d" % (blen, extra, pre), s, cap=s.n + extra))
            cases.append(_case("F %d -1 @%d" % (blen, pre), s, cap=s.n - 1))
    return cases


# ---- G. distance edges --------------------------------------------------------------------------
@functools.lru_cache(None)
def family_g():
    rng = random.Random(707)
    cases = []
    for pre in (100, 5000, 32767, 32768, 40000):
        for where in ("first", "last"):
            for dd in (0, 1):
                s = _Stream(rng).stored(pre)
                head = [] if where == "first" else s.near(RMAX - 1)
                w = s.n + sum(t[0] for t in head)
                d = min(w, 32768) + dd
                if d > 32768:
                    continue
                s.block(head + [(3, d)] + s.near(8))
                cases.append(_case("G d=written%s %s @%d" % ("+1" if dd else "", where, pre), s, zlib_ok=dd == 0))
    return cases


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "E": family_e, "F": family_f, "G": family_g}
PROBE = {"A": ("A near", ["end_records"]), "B": ("B h17-24", ["far_spill"]), "C": ("C 258 near+far @40000", ["end_stage", "end_fit"])}


_RAW, _REF = {}, {}  # (the families' block lists live as long as the module: their ids are stable keys)


def _raw(blocks):
    if id(blocks) not in _RAW:
        _RAW[id(blocks)] = write(blocks)
    return _RAW[id(blocks)]


def _ref(oracle, blocks, cap):
    """(expand's status and bytes, the oracle's status, consumed and bytes)"""
    key = (id(blocks), cap)
    if key not in _REF:
        _REF[key] = (expand(blocks, cap), oracle.de_inflate(_raw(blocks), cap))
    return _REF[key]


def _check(oracle, cases, results):
    """kernel results against expand(), the oracle and zlib"""
    for (name, blocks, cap, zlib_ok), (st, used, out, adler) in zip(cases, results):
        raw = _raw(blocks)
        (est, eout), (ost, oused, oout) = _ref(oracle, blocks, cap)
        assert (ost, oout) == (est, eout), name  # the writer and its reference agree with the oracle
        assert (st, used) == (ost, oused), (name, st, used, ost, oused)
        assert out == oout, (name, len(out), len(oout), next((i for i, (a, b) in enumerate(zip(out, oout)) if a != b), None))
        if st == OK:
            assert used == len(raw) and adler == zlib.adler32(out), name
            if zlib_ok:
                assert zlib.decompress(raw, -15) == out, name


def test_round_streams_are_what_they_claim(oracle):
    """(CPU) every family's streams: the writer's reference and the oracle agree, and the streams reach their limits
    by construction - enough records for a full pool, enough bytes for a full staging buffer"""
    for fam in FAMILIES.values():
        for name, blocks, cap, _ in fam():
            (est, eout), (ost, _, oout) = _ref(oracle, blocks, cap)
            assert (ost, oout) == (est, eout), name
    assert sum(1 for t in family_a()[0][1][-1].tokens if not isinstance(t, int)) >= 2 * RMAX
    assert 3 * RMAX < STAGE  # 3-byte records fill the pool before the staging buffer


@pytest.fixture(scope="module")
def eng():
    import decompress_amd
    return decompress_amd.Engine(0)


@pytest.fixture(params=[2, 1], ids=["two-wavefronts", "one-wavefront"])
def eng_ring(eng, request):
    eng.set_option("inflate_waves", request.param)
    yield eng
    eng.set_option("inflate_waves", 2)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_family(eng_ring, oracle, fam):
    cases = FAMILIES[fam]()
    res = eng_ring.inflate_many([_raw(c[1]) for c in cases], [c[2] for c in cases])
    _check(oracle, cases, res)


@pytest.mark.gpu
@pytest.mark.parametrize("fam", sorted(PROBE))
def test_family_reaches_its_path(eng_ring, oracle, fam):
    """the family's probe stream alone (stream 0, the one the profile reports) with the in-kernel profile on"""
    name, counters = PROBE[fam]
    case = next(c for c in FAMILIES[fam]() if c[0] == name)
    eng_ring.set_option("profile", 1)
    try:
        res = eng_ring.inflate_many([_raw(case[1])], [case[2]])
        prof = eng_ring.get_profile()
    finally:
        eng_ring.set_option("profile", 0)
    _check(oracle, [case], res)
    for k in counters:
        assert prof[k] > 0, (name, k, {c: prof[c] for c in prof if not c.startswith("cyc_")})


def _bounds_run(eng, oracle, cases, pattern=0xA5, raw=None, check=None):
    """one batch with the streams' outputs back to back (no padding, unaligned offsets) in a buffer filled with a
    pattern: nothing outside [out_off, out_off + out_len) may change.  raw / check: for cases of another make than this
    module's (tests/test_gpu_inflate_headers.py): how a case gives its stream and how the results are compared."""
    import torch
    raws = [(raw or _raw)(c[1]) for c in cases]
    n = len(cases)
    in_len = np.array([len(r) for r in raws], dtype=np.int64)
    in_off = np.zeros(n, dtype=np.int64)
    np.cumsum(in_len[:-1], out=in_off[1:])
    cap = np.array([c[2] for c in cases], dtype=np.int64)
    out_off = np.zeros(n, dtype=np.int64)
    np.cumsum(cap[:-1], out=out_off[1:])
    out_off += 3  # (the first stream unaligned too)
    size = int(out_off[-1] + cap[-1]) + 64
    dev = eng.device
    t = lambda a: torch.from_numpy(a).to(dev)
    d_in = t(np.frombuffer(b"".join(raws) + bytes(16), dtype=np.uint8).copy())
    d_out = torch.full((size,), pattern, dtype=torch.uint8, device=dev)
    out_len, consumed, status, _ = eng.inflate_batch(0, d_in, t(in_off), t(in_len), d_out, t(out_off), t(cap))
    torch.cuda.synchronize(dev)
    out = d_out.cpu().numpy()
    out_len, consumed, status = out_len.cpu().numpy(), consumed.cpu().numpy(), status.cpu().numpy()
    written = np.zeros(size, dtype=bool)
    for i in range(n):
        assert 0 <= out_len[i] <= cap[i], cases[i][0]
        written[out_off[i]:out_off[i] + out_len[i]] = True
    outside = np.nonzero(~written & (out != pattern))[0]
    assert outside.size == 0, ("written outside [out_off, out_off + out_len)", outside[:16])
    res = [(int(status[i]), int(consumed[i]), out[out_off[i]:out_off[i] + out_len[i]].tobytes(), zlib.adler32(
        out[out_off[i]:out_off[i] + out_len[i]].tobytes())) for i in range(n)]
    (check or _check)(oracle, cases, res)


@pytest.mark.gpu
def test_bounds_small_batch(eng_ring, oracle):
    """a few streams of every family, exact and tight caps, errors included"""
    cases = []
    for fam in "ABCDEF":
        cs = FAMILIES[fam]()
        cases += cs[:2] + cs[-2:]
    _bounds_run(eng_ring, oracle, cases)


@pytest.mark.gpu
def test_bounds_all_families(eng_ring, oracle):
    cases = [c for fam in "ABCDEFG" for c in FAMILIES[fam]()]
    _bounds_run(eng_ring, oracle, cases)
