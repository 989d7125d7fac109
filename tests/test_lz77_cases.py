"""tests/lz77_cases.py against its two CPU witnesses: every case's claims hold in the model (tests/lz77_model.py), the
model's parse equals the oracle's (commands and both histograms) and, for Lz's matcher, libz's own decisions; and the
families together reach the branches they are named for.  The GPU half is tests/test_gpu_lz77_cases.py."""
import zlib
from collections import defaultdict
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import lz77_cases as K
from tests import lz77_model as M
from tests.deflate_tokens import tokens

COMBOS = [(0, lv) for lv in K.ALL0] + [(1, lv) for lv in K.ALL1]


@pytest.fixture(scope="module")
def parses():
    """model parse of every case at every (matcher, level), queues 4 096 and 16 filled in one pass:
    {(name, matcher, level): Parse}, its cmds a dict by queue size"""
    out = {}
    for name, data, _ in K.cases():
        for m, lv in COMBOS:
            out[name, m, lv] = M.parse(data, m, lv, (4096, 16))
    return out


def check_claims(name, data, claims, parse_of):
    """every claim of a case against the model; parse_of(matcher, level) -> Parse"""
    looks, lk = {}, {}
    want_look = defaultdict(set)
    for c in claims:
        if c[0] in ("look", "look_differs"):
            for lv in c[2]:
                want_look[c[1], lv].add(c[3])
    for (m, lv), ps in want_look.items():
        looks[m, lv] = M.look_ahead(data, m, lv, sorted(ps))
    for c in claims:
        kind = c[0]
        if kind == "link":
            _, m, pos, dist = c
            if m not in lk:
                lk[m] = M.links(data, m)
            assert lk[m][0][pos] == dist, (name, c, lk[m][0][pos])
        elif kind == "tail":
            if 0 not in lk:
                lk[0] = M.links(data, 0)
            assert lk[0][1][c[1]] == c[2], (name, c, lk[0][1])
        elif kind == "look":
            _, m, levels, pos, field, value = c
            for lv in levels:
                got = getattr(looks[m, lv][pos], field)
                assert got == value, (name, c, lv, got)
        elif kind == "look_differs":
            _, m, levels, pos = c
            for lv in levels:
                assert looks[m, lv][pos].full != looks[m, lv][pos].quarter, (name, c, lv)
        elif kind == "call":
            _, m, levels, pos, bar, walked = c
            for lv in levels:
                got = [x for x in parse_of(m, lv).calls if x.pos == pos]
                assert len(got) == 1 and got[0].bar == bar and walked in (None, got[0].walked), (name, c, lv, got)
        elif kind == "match":
            _, m, levels, pos, length, dist, k = c
            for lv in levels:
                got = [x for x in parse_of(m, lv).matches if x.pos == pos]
                assert len(got) == 1 and got[0].length == length and dist in (None, got[0].dist) \
                    and got[0].deferrals == k, (name, c, lv, got)
        elif kind == "literals":
            _, m, levels, lo, hi = c
            for lv in levels:
                got = [x for x in parse_of(m, lv).matches if lo <= x.pos < hi]
                assert not got, (name, c, lv, got)
        elif kind == "slides":
            _, m, levels, count = c
            for lv in levels:
                assert len(parse_of(m, lv).slides) == count, (name, c, lv, parse_of(m, lv).slides)
        elif kind == "ring":
            _, pos, d = c
            assert (pos - d) % 1024 == 0 and -8 < d < 8, (name, c)
            assert any(pos in x[1:] for x in claims if x[0] in ("match", "call", "look")), (name, c)
        else:
            raise AssertionError("unknown claim %r" % (c,))


def test_names_sizes_and_prefixes():
    cases = K.cases()
    assert {K.family(n) for n, _, _ in cases} == set(K.FAMILIES)
    big = [n for n, d, _ in cases if len(d) > 60000]
    assert len(big) <= 12, big
    for fam in "ABCDGH":  # the families that sweep a prefix: all of them many alignments to the 64-lane step
        pres = {int(n.rsplit("_pre", 1)[1]) % 64 for n, _, _ in cases if n[0] == fam and "_pre" in n}
        assert len(pres) >= 8, (fam, sorted(pres))
    # a few G and H structures stand a few positions before, at and behind a multiple of 1 024, the look-ahead ring
    ring = defaultdict(set)
    for n, _, claims in cases:
        for c in claims:
            if c[0] == "ring":
                ring[n[0]].add(c[2])
    assert ring["G"] >= {-2, 0, 1} and ring["H"] >= {-2, 0, 1}, dict(ring)
    pres = {int(n.rsplit("_pre", 1)[1]) for n, _, _ in cases if "_pre" in n}
    assert {p % 64 for p in pres} == set(range(64)) and len(pres) >= 100, sorted(set(range(128)) - pres)


def test_claims_hold_in_the_model(parses):
    for name, data, claims in K.cases():
        check_claims(name, data, claims, lambda m, lv, name=name: parses[name, m, lv])


def test_model_equals_oracle(oracle, parses):
    """commands and both histograms, matcher 0 at levels 1-9 and matcher 1 at levels 4-9, queues 4 096 and 16"""
    cases = K.cases()
    jobs = [(name, data, m, lv, q) for name, data, _ in cases for m, lv in COMBOS for q in (4096, 16)]
    with ThreadPoolExecutor(16) as ex:  # (ctypes releases the GIL)
        wants = list(ex.map(lambda j: oracle.lz77_all(j[1], level=j[3], queue=j[4], matcher=j[2]), jobs))
    for (name, data, m, lv, q), want in zip(jobs, wants):
        got = parses[name, m, lv]
        assert got.cmds[q] == want[0], (name, m, lv, q, len(got.cmds[q]), len(want[0]))
        assert (got.lits, got.dists) == (want[1], want[2]), (name, m, lv, q)


def _table(lens):
    """code lengths -> a decoding table indexed by the next max-length bits (LSB first): (symbol, length)"""
    top = max(lens)
    count = [0] * (top + 2)
    for ln in lens:
        count[ln] += 1
    count[0] = 0
    code, nxt = 0, [0] * (top + 2)
    for b in range(1, top + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = [None] * (1 << top)
    for sym, ln in enumerate(lens):
        if ln:
            rev = int(format(nxt[ln], "0%db" % ln)[::-1], 2)
            nxt[ln] += 1
            for k in range(rev, 1 << top, 1 << ln):
                table[k] = (sym, ln)
    return table, top


def fast_tokens(z):
    """tests/deflate_tokens.tokens without the block markers, with a bit buffer and one table per code instead of a
    dictionary probe per bit: this file reads several megabytes of libz's output.  Stored blocks are refused."""
    from tests.deflate_tokens import DB, DX, LB, LX
    bits = int.from_bytes(z, "little")  # (consumed 2 048 bits at a time: shifting the whole stream per symbol is quadratic)
    buf, cnt, at = 0, 0, 0
    out, op = [], 0

    def fill(n):
        nonlocal buf, cnt, at
        if cnt < n:
            buf |= ((bits >> at) & ((1 << 2048) - 1)) << cnt
            at += 2048
            cnt += 2048

    def take(n):
        nonlocal buf, cnt
        fill(n)
        v = buf & ((1 << n) - 1)
        buf >>= n
        cnt -= n
        return v

    def sym(tb):
        nonlocal buf, cnt
        table, top = tb
        fill(top)
        s, ln = table[buf & ((1 << top) - 1)]
        buf >>= ln
        cnt -= ln
        return s
    while True:
        last, kind = take(1), take(2)
        assert kind in (1, 2), "libz wrote a stored block: its decisions are not in the stream"
        if kind == 1:
            lt, dt = _table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _table([5] * 30)
        else:
            hl, hd, hc = take(5) + 257, take(5) + 1, take(4) + 4
            cl = [0] * 19
            for k in range(hc):
                cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[k]] = take(3)
            ct, ls = _table(cl), []
            while len(ls) < hl + hd:
                s = sym(ct)
                if s < 16:
                    ls.append(s)
                elif s == 16:
                    ls += [ls[-1]] * (3 + take(2))
                elif s == 17:
                    ls += [0] * (3 + take(3))
                else:
                    ls += [0] * (11 + take(7))
            lt, dt = _table(ls[:hl]), _table(ls[hl:] if any(ls[hl:]) else [1])
        while True:
            s = sym(lt)
            if s < 256:
                out.append((op, "L", s))
                op += 1
            elif s == 256:
                break
            else:
                ln = LB[s - 257] + take(LX[s - 257])
                ds = sym(dt)
                d = DB[ds] + take(DX[ds])
                out.append((op, "M", ln, d))
                op += ln
        if last:
            return out


def _libz_tokens(data, level):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 8)
    return fast_tokens(co.compress(data) + co.flush())


def _cmd_tokens(cmds):
    out, pos = [], 0
    for c in cmds:
        if c == M.EOB:
            continue
        if c & M.COPY:
            ln, d = ((c >> 16) & 0x1FF) + 3, (c & 0xFFFF) + 1
            out.append((pos, "M", ln, d))
            pos += ln
        else:
            out.append((pos, "L", c))
            pos += 1
    return out


def test_fast_tokens_equal_the_plain_tokenizer():
    for name, data, _ in K.cases()[::40]:
        for lv in (4, 9):
            co = zlib.compressobj(lv, zlib.DEFLATED, -15, 8)
            z = co.compress(data) + co.flush()
            assert fast_tokens(z) == [t for t in tokens(z) if t[0] != "B"], (name, lv)


def test_lz_matcher_equals_libz(parses):
    """lib/lz.ml is zlib's deflate_slow: the model's decisions for matcher 1 are libz's own, token for token.  No case
    is skipped: the background keeps libz away from stored blocks, and inputs of a few bytes get a fixed block."""
    for name, data, _ in K.cases():
        for lv in K.ALL1:
            want = _libz_tokens(data, lv)
            got = _cmd_tokens(parses[name, 1, lv].cmds[4096])
            assert len(got) == len(want), (name, lv, len(got), len(want))
            for k, (x, y) in enumerate(zip(got, want)):
                assert x == y, (name, lv, k, x, y)


def test_families_reach_their_branches(parses):
    """counts from the trace, not from the names"""
    cases = K.cases()
    by_family = defaultdict(list)
    for name, data, _ in cases:
        by_family[K.family(name)].append((name, data))
    # A: at every level a bar-2 walk of exactly max_chain candidates that the budget ended with more in the chain, one
    # of max_chain whose chain ended there too, one of max_chain - 1 that stopped on the chain's end, and a full result
    # that differs from the quartered one
    for lv in K.ALL0:
        mc = M.config(0, lv).max_chain
        walks = defaultdict(set)
        differ = False
        for name, data in by_family["A"]:
            for c in parses[name, 0, lv].calls:
                if c.bar == 2:
                    walks[c.walked].add(c.more)
            t = [cl[3] for cl in dict((n, c) for n, _, c in cases)[name] if cl[0] == "look"][0]
            look = M.look_ahead(data, 0, lv, [t])[t]
            differ = differ or look.full != look.quarter
        assert walks[mc] == {True, False} and walks[mc - 1] == {False} and max(walks) == mc, (lv, dict(walks))
        assert differ, lv
    # B: at every nice_length a walk that stops at its first candidate and one that goes on to a longer one
    for lv in range(1, 8):
        nice = M.config(0, lv).nice_length
        stopped = went_on = False
        for name, data in by_family["B"]:
            for c in parses[name, 0, lv].calls:
                if c.bar == 2 and c.length >= nice:
                    stopped = stopped or c.walked == 1
                    went_on = went_on or c.walked >= 2
        assert stopped and went_on, lv
    # C: every length class comes out as a match
    lens = {m.length for name, _ in by_family["C"] for m in parses[name, 0, 9].matches}
    assert set(range(4, 19)) | {23, 24, 25, 31, 32, 33, 255, 256, 257, 258} <= lens, sorted(lens)
    assert 3 in {m.length for name, _ in by_family["C"] for m in parses[name, 1, 9].matches}
    # D: walks over candidates none of which shares 3 bytes (result 2), both matchers
    for m in (0, 1):
        assert any(c.length == 2 and c.walked >= 2 for name, _ in by_family["D"] for c in parses[name, m, 9].calls), m
    # E: matches at distance MAX_DIST exactly, none beyond; slides
    dists = {x.dist for name, _ in by_family["E"] for x in parses[name, 0, 6].matches}
    assert M.MAX_DIST in dists and M.MAX_DIST - 1 in dists and max(dists) == M.MAX_DIST, sorted(dists)[-4:]
    two = [parses[name, 0, 6] for name, _ in by_family["E"] if len(parses[name, 0, 6].slides) == 2]
    assert two and all(any(a < x.pos <= a + 50 and x.dist == M.MAX_DIST for x in p.matches) for p in two for a in p.slides)
    # F: matches clipped to the lookahead, the clipped 3 at 4 096 included; the H7 tail after a slide
    clipped = [(c.length, c.dist) for name, data in by_family["F"] for c in parses[name, 0, 6].calls
               if c.pos + c.length == len(data)]
    assert (3, 4096) in clipped and len({ln for ln, _ in clipped}) >= 8, clipped
    # G: lazy chains of every depth up to 100 and the depths around the wave's 64 chains and 80-position view; a walk
    # that the budget of the quarter cuts short
    for m, lv in ((0, 9), (1, 9)):
        depths = {x.deferrals for name, _ in by_family["G"] for x in parses[name, m, lv].matches}
        assert depths >= set(range(0, 6)) | {62, 63, 64, 65, 66, 78, 79, 80, 81, 82, 100}, (m, sorted(depths))
    for lv in range(1, 9):  # (level 9: max_lazy is the longest match itself)
        cfg = M.config(0, lv)
        stops = {x.deferrals for name, _ in by_family["G"] for x in parses[name, 0, lv].matches}
        assert cfg.max_lazy - 4 in stops, (lv, sorted(stops))
    assert any(c.bar >= 8 and c.budget == 8 and c.walked == 8 for name, _ in by_family["G"] for c in parses[name, 0, 5].calls)
    # ... and at the quarter mark itself, De's matcher: a quartered walk that finds its match at its last link, and one
    # that ends one link short of the only longer candidate
    for lv in (2, 3, 5, 6, 7, 8):
        cfg = M.config(0, lv)
        cut = [c for name, _ in by_family["G"] for c in parses[name, 0, lv].calls
               if c.bar >= cfg.good_length and c.walked == c.budget == cfg.max_chain >> 2 and c.more]
        assert any(c.length > c.bar for c in cut) and any(c.length == c.bar for c in cut), (lv, cut)
    # H: literal runs of the lengths around the 64-lane step and the 8 x 64 group
    runs = set()
    for name, _ in by_family["H"]:
        ms = sorted(parses[name, 0, 6].matches)
        runs |= {b.pos - (a.pos + a.length) for a, b in zip(ms, ms[1:])}
    assert runs >= {62, 63, 64, 65, 66, 510, 511, 512, 513, 514, 1022, 1023, 1024, 1025, 1026}, sorted(runs)
    # I: links of every distance the family names
    have = set()
    for name, data in by_family["I"]:
        have |= set(M.links(data, 0)[0])
    assert have >= {1, 2, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193}
