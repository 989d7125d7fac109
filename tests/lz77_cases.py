"""Hand-built inputs for the deflate match finder (csrc/deflate_front.hip, deflate_link.hpp, deflate_kernel.hip's
parse_step / literal_run / lz_deflate) at the limits the kernels have and the reference has not.

Every case is (name, data, claims).  A claim states, in terms of tests/lz77_model.py, the property the case exists for;
tests/test_lz77_cases.py checks every claim, so a case cannot quietly stop hitting its edge:

  ("link", matcher, pos, dist)                        links()[0][pos] == dist
  ("tail", k, pos)                                    links(data, 0)[1][k] == pos
  ("look", matcher, levels, pos, field, value)        look_ahead()[pos].field == value at each of the levels
  ("look_differs", matcher, levels, pos)              the full-chain and quartered results at pos differ
  ("call", matcher, levels, pos, bar, walked)         parse() calls longest_match at pos with that bar and walks
                                                      exactly `walked` candidates (None: any)
  ("match", matcher, levels, pos, length, dist, k)    parse() emits that match behind k deferrals
  ("literals", matcher, levels, lo, hi)               parse() emits no match that starts in [lo, hi)
  ("slides", matcher, levels, count)                  the window slides that often
  ("ring", pos, d)                                    pos, which other claims of the case name, lies d positions from
                                                      a multiple of 1 024 (the sequential kernel's look-ahead ring)

The background is a de Bruijn sequence B(37, 3) per 50 653 bytes (alphabets 40.., 120.., 200..): no 3-gram repeats, so
what a case plants is the only structure in it.  Sources are planted by copying the target's bytes BACK into earlier
background (the target's own bytes stay background), fenced by bytes from outside the alphabets so that a planted
match has exactly its length.  Successive cases stand behind background prefixes of successive lengths 0 .. 127: every
family meets every alignment to the 64-lane step, the 80-position view and the 256-position chunk.

Deterministic: no randomness but one seeded search for fingerprint collisions.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

from tests import lz77_model as M

MAX_DIST = M.MAX_DIST
ALL0 = tuple(range(1, 10))   # De.Lz77's levels
ALL1 = tuple(range(4, 10))   # Lz's
FAMILIES = "ABCDEFGHI"


@functools.lru_cache(None)
def _de_bruijn():
    k, n = 37, 3
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return bytes(seq)


@functools.lru_cache(None)
def _background():
    s = _de_bruijn()
    s = s[4001:] + s[:4001]  # (the sequence begins 0 0 0 1 0 0 2 0 0 3 ...: begin where pairs do not repeat either)
    return b"".join(bytes(c + off for c in s) for off in (40, 120, 200))


def background(n, start=0):
    bg = _background()
    assert start + n <= len(bg)
    return bytearray(bg[start:start + n])


class _Fence:
    """bytes from outside the alphabets, a different one each time"""
    def __init__(self):
        self.k = 0

    def __call__(self, *avoid):
        while True:
            self.k += 1
            g = 1 + (self.k * 7) % 39
            if g not in avoid:
                return g


def plant(buf, dst, src, ln, fence):
    """make buf[src:src+ln] a copy of buf[dst:dst+ln] (src < dst) that matches dst for exactly ln bytes and does not
    match one byte earlier"""
    assert 0 <= src and src + ln < dst
    buf[src:src + ln] = buf[dst:dst + ln]
    if dst + ln < len(buf):
        buf[src + ln] = fence(buf[dst + ln])
    if src > 0:
        buf[src - 1] = fence(buf[dst - 1])


def _hashes4(buf):
    a = np.frombuffer(bytes(buf), dtype=np.uint8).astype(np.uint32)
    v = a[:-3] | (a[1:-2] << 8) | (a[2:-1] << 16) | (a[3:] << 24)
    return (v * np.uint32(0x9E3779B1)) >> np.uint32(17)


def _hashes3(buf):
    a = np.frombuffer(bytes(buf), dtype=np.uint8).astype(np.uint32)
    return ((a[:-2] << 10) ^ (a[1:-1] << 5) ^ a[2:]) & np.uint32(0x7FFF)


def plant_clean(buf, dd, src, ln, fence, more=None):
    """plant ln bytes at distance dd, the source at `src` or the first place behind it for which no position between
    source and target shares the target's hash4: the source is the head of the target's chain for De's matcher;
    more(buf, t) plants what else belongs to the target.  -> (target position, whether the same holds for Lz's hash)"""
    for _ in range(400):
        trial = bytearray(buf)
        t = src + dd
        plant(trial, t, src, ln, fence)
        if more:
            more(trial, t)
        h4, h3 = _hashes4(trial), _hashes3(trial)
        if (h4[src + 1:t] == h4[t]).sum() == (1 if more else 0):
            buf[:] = trial
            return t, (h3[src + 1:t] == h3[t]).sum() == (1 if more else 0)
        src += 1
    raise AssertionError("no clean place")


def place_heads(buf, positions, seed=0):
    """write one 4-byte head at every position: one whose hash (either matcher's) no other position of buf has"""
    for seed in range(seed, seed + 400):
        hd = bytes([1 + (seed * 5 + k * 11) % 39 for k in range(4)])
        trial = bytearray(buf)
        for p in positions:
            trial[p:p + 4] = hd
        h4, h3 = _hashes4(trial), _hashes3(trial)
        if (h4 == M.hash4(*hd)).sum() == len(positions) and (h3 == M.hash3(*hd[:3])).sum() == len(positions):
            buf[:] = trial
            return hd
    raise AssertionError("no head without a stray hash collision")


def _levels_where(pred, matcher=0):
    return tuple(lv for lv in (ALL1 if matcher else ALL0) if pred(M.config(matcher, lv)))


class _Sweep:
    """the prefix lengths 0 .. 127 in turn"""
    def __init__(self, step=1):
        self.k, self.step = -step, step

    def __call__(self):
        self.k = (self.k + self.step) % 128
        return self.k


# ---------------------------------------------------------------------------------------------------------------
# A. chain depth: c positions share one hash and one 4-byte head in front of a target with that head; every candidate
# shares exactly the 4 bytes except the one at link index i (1 = the head of the chain), which shares 7.  The members
# are a period-7 stretch ("head xyz" over and over), which the matcher covers with long matches: only the target and
# the few positions around the odd member walk the chain, so the model stays cheap at 4 097 links (spacing 7).
def chain_stream(pre, c, i, head_seed=0, tail=320, unit_len=7):
    """-> (buf, target position, distance of the long candidate, distance of the nearest one); the members stand
    unit_len bytes apart and the long candidate shares unit_len bytes with the target"""
    gap = 9
    for seed in range(head_seed, head_seed + 64):
        hd = bytes([1 + (seed * 5 + k * 11) % 39 for k in range(4)])
        if unit_len == 7:
            unit = hd + bytes([80 + (seed * 3) % 20, 100 + (seed * 7) % 19, 101 + (seed * 7) % 19 + 1])
        else:
            unit = hd + bytes(80 + (seed * 3 + 7 * j) % 40 for j in range(unit_len - 4))
        region = pre or 128  # (position 0 is NIL: it cannot be a member)
        t = region + unit_len * c + gap
        buf = background(t + tail)
        buf[region:region + unit_len * c] = unit * c
        buf[t:t + 4] = hd
        buf[region - 1], buf[t - 1] = 0xFD, 0xFE  # nothing in front of the head joins a match
        buf[region + unit_len * c] = 0xFC         # ... and nothing behind the last member
        if i:
            u = region + unit_len * (c - i)
            buf[u + 4:u + unit_len] = buf[t + 4:t + unit_len]
        hs = _hashes4(buf)
        mine = M.hash4(*hd)
        if int((hs == mine).sum()) == c + 1:  # no other position of the stream is in this chain
            return buf, t, (t - (region + unit_len * (c - i))) if i else 0, gap + unit_len
    raise AssertionError("no head without a stray hash collision")


def chain_claims(c, i, t, dlong, dnear):
    claims = []
    for lv in ALL0:
        cfg = M.config(0, lv)
        q = cfg.max_chain >> 2
        walked = min(c, cfg.max_chain)
        full = (7, dlong) if i and i <= cfg.max_chain else (4, dnear)
        quarter = (7, dlong) if i and i <= q else (4, dnear)
        claims += [("look", 0, (lv,), t, "walked", walked), ("look", 0, (lv,), t, "full", full),
                   ("look", 0, (lv,), t, "quarter", quarter), ("call", 0, (lv,), t, 2, walked)]
        if full != quarter:
            claims.append(("look_differs", 0, (lv,), t))
    return claims


def family_a():
    sweep = _Sweep(3)
    seen, cases = set(), []
    for lv in ALL0:
        mc = M.config(0, lv).max_chain
        q = mc >> 2
        cs = [q - 1, q, q + 1, mc - 1, mc, mc + 1] + ([127, 128, 129, 130] if mc >= 128 else [])
        wanted = [1, q - 1, q, q + 1, mc - 1, mc, mc + 1, 127, 128, 129]
        for c in cs:
            if c < 1:
                continue
            idx = sorted({i for i in wanted if 1 <= i <= c})
            # every c carries its deepest index and (the streams of 7 and 29 KiB aside) the one at the quarter mark or the
            # head; every index is carried by the smallest c that holds it
            pick = {idx[-1]} | ({max(k for k in idx if k <= max(q, 1))} if c < 1000 else set())
            pick |= {i for i in idx if c == min(x for x in cs if x >= i)}
            for i in sorted(pick):
                if (c, i) not in seen:
                    seen.add((c, i))
                    pre = sweep()
                    buf, t, dl, dn = chain_stream(pre, c, i, head_seed=len(seen))
                    cases.append(("A.chain_c%d_i%d_pre%d" % (c, i, pre), bytes(buf), chain_claims(c, i, t, dl, dn)))
    return cases


# ---------------------------------------------------------------------------------------------------------------
# B. nice_length: a shallow candidate of nice - 1 / nice / nice + 1 bytes, a longer one behind it
def family_b():
    sweep, cases = _Sweep(3), []
    for nice in (8, 16, 32, 128):
        for s in (nice - 1, nice, nice + 1):
            pre, fence = sweep(), _Fence()
            deep = nice + 6
            buf = background(pre + 2 * deep + 700)
            d_src, s_src = pre + 8, pre + deep + 40
            t = s_src + deep + 40
            plant(buf, t, d_src, deep, fence)
            plant(buf, t, s_src, s, fence)
            claims = []
            for m in (0, 1):
                for lv in (ALL1 if m else ALL0):
                    n_lv = M.config(m, lv).nice_length
                    want = (s, t - s_src) if s >= n_lv else (min(deep, 258), t - d_src)
                    claims.append(("look", m, (lv,), t, "full", want))
            cases.append(("B.nice%d_shallow%d_pre%d" % (nice, s, pre), bytes(buf), claims))
    return cases


# ---------------------------------------------------------------------------------------------------------------
# C. the compare code: every length class of prefix16 / lcp258_from16, and the scan_end pre-filter
C_LENGTHS = list(range(3, 19)) + [23, 24, 25, 31, 32, 33, 255, 256, 257, 258, 300]


def family_c():
    sweep, cases = _Sweep(5), []
    for k in range(0, len(C_LENGTHS), 6):
        pre, fence = sweep(), _Fence()
        lens = C_LENGTHS[k:k + 6]
        buf = background(pre + sum(2 * ln + 40 for ln in lens) + 400)
        p, claims = pre + 5, []
        for ln in lens:
            src, t = p, p + ln + 20
            plant(buf, t, src, ln, fence)
            for m in (0, 1):
                if ln >= 4 or m == 1:  # hash4 never brings a 3-byte match together: its 4th byte differs
                    claims.append(("look", m, ALL1 if m else ALL0, t, "full", (min(ln, 258), t - src)))
            if ln >= 4:
                claims.append(("match", 0, ALL0, t, min(ln, 258), t - src, 0))
            p = t + ln + 20
        cases.append(("C.lengths_%s_pre%d" % ("_".join(map(str, lens)), pre), bytes(buf), claims))
    # a best match of `best` >= 16 bytes at the head of the chain, then a candidate that agrees on 16 bytes and
    # differs at best - 1 (shorter), at best (as long: the nearer one stays), at best + 1 (longer by one: it wins)
    for best in (16, 17, 24, 40):
        for delta in (-1, 0, 1):
            pre, fence = sweep(), _Fence()
            second = best + delta
            buf = background(pre + 4 * best + 600)
            far, near = pre + 6, pre + best + 50
            t = near + best + 50
            plant(buf, t, far, second, fence)
            plant(buf, t, near, best, fence)
            want = (second, t - far) if delta > 0 else (best, t - near)
            lv0 = _levels_where(lambda c: c.nice_length > best + 1)
            lv1 = _levels_where(lambda c: c.nice_length > best + 1, 1)
            claims = [("look", 0, lv0, t, "full", want), ("look", 1, lv1, t, "full", want),
                      ("look", 0, lv0, t, "walked", 2)]
            cases.append(("C.best%d_second%+d_pre%d" % (best, delta, pre), bytes(buf), claims))
    return cases


# ---------------------------------------------------------------------------------------------------------------
# D. fingerprints: strings that share the position's hash and the 16-bit fingerprint of its first 3 bytes, not the bytes
@functools.lru_cache(None)
def liars(matcher, count=6):
    """-> [(a, b)]: byte strings (4 bytes for hash4, 3 for Lz's hash) with one hash and one fp16 whose first 3 bytes
    differ.  A seeded birthday search over 2^21 strings (hash4) / all 2^24 3-grams (Lz)."""
    if matcher == 0:
        v = np.random.default_rng(1951).integers(0, 1 << 32, 1 << 21, dtype=np.uint64).astype(np.uint32)
        v = np.unique(v)
        h = (v * np.uint32(0x9E3779B1)) >> np.uint32(17)
    else:
        g = np.arange(256, dtype=np.uint32)
        b0, b1, b2 = [x.ravel() for x in np.meshgrid(g, g, g, indexing="ij")]
        v = b0 | (b1 << 8) | (b2 << 16)
        h = ((b0 << 10) ^ (b1 << 5) ^ b2) & np.uint32(0x7FFF)
    f = ((v & np.uint32(0xFFFFFF)) * np.uint32(0x9E3779B1)) >> np.uint32(16)
    key = (h.astype(np.uint64) << np.uint64(16)) | f.astype(np.uint64)
    order = np.argsort(key, kind="stable")
    ks, vs = key[order], v[order]
    out = []
    for j in np.nonzero(ks[1:] == ks[:-1])[0]:
        a, b = int(vs[j]), int(vs[j + 1])
        if (a ^ b) & 0xFFFFFF:
            n = 3 if matcher else 4
            out.append((a.to_bytes(4, "little")[:n], b.to_bytes(4, "little")[:n]))
            if len(out) == count:
                break
    assert len(out) == count
    return out


def family_d():
    """the position holds `a`; the chain in front of it is a sequence of L (the liar `b`) and T (a true candidate: `a`
    and 3 more bytes of the target); "LL" is a chain that ends without a candidate: the look-ahead's FL_ENDED"""
    sweep, cases = _Sweep(7), []
    for matcher in (0, 1):
        for k, pattern in enumerate(("LT", "TL", "LTLT", "TLLT", "LL", "L", "LLLLT")):
            a, b = liars(matcher)[k % 6]
            pre, fence = sweep(), _Fence()
            step = 24
            t = pre + 10 + step * len(pattern)
            buf = background(t + 340)
            buf[t:t + len(a)] = a
            true_len = len(a) + 3  # (below every nice_length: the walk goes on)
            spots = []
            for j, ch in enumerate(pattern):  # pattern[0] is the nearest candidate
                at = t - step * (j + 1)
                if ch == "T":
                    buf[at:at + true_len] = buf[t:t + true_len]
                    buf[at + true_len] = fence(buf[t + true_len])
                    buf[at - 1] = fence(buf[t - 1])
                else:
                    buf[at:at + len(b)] = b
                spots.append(at)
            trues = [at for at, ch in zip(spots, pattern) if ch == "T"]
            levels = _levels_where(lambda c: c.max_chain >= len(pattern), matcher)
            want = (true_len, t - trues[0]) if trues else (2, 0)
            claims = [("look", matcher, levels, t, "full", want), ("look", matcher, levels, t, "share3", bool(trues)),
                      ("link", matcher, t, t - spots[0])]
            claims.append(("look", matcher, levels, t, "walked", len(pattern)))
            if not trues:
                claims.append(("literals", matcher, levels, t - 2, t + 2))
            cases.append(("D.m%d_%s_pre%d" % (matcher, pattern, pre), bytes(buf), claims))
    return cases


# ---------------------------------------------------------------------------------------------------------------
# E. reach: the head is a candidate at MAX_DIST, a link only below it; links reach 32 767; slides drop what is below
def family_e():
    cases = []
    # one 36 KiB stream: 12-byte matches at distance MAX_DIST - 1 / MAX_DIST / MAX_DIST + 1 as the head of the chain,
    # the same as its second link behind a nearer 5-byte candidate, and 9-byte sources 32 767 / 32 768 back
    fence = _Fence()
    pre = 70
    buf = background(pre + 32768 + 8 * 400 + 700)
    claims = []
    plan = [(False, MAX_DIST - 1), (False, MAX_DIST), (False, MAX_DIST + 1), (True, MAX_DIST - 1), (True, MAX_DIST),
            (True, MAX_DIST + 1), (False, 32767), (False, 32768)]
    for k, (second, dd) in enumerate(plan):
        # (second: a nearer candidate in front, the far one is now a link)
        t, lz_too = plant_clean(buf, dd, pre + 10 + 400 * k, 12, fence,
                                (lambda b, t: plant(b, t, t - 60, 5, fence)) if second else None)
        reach = dd < MAX_DIST or (dd == MAX_DIST and not second)
        for m in (0, 1) if lz_too else (0,):
            want = (12, dd) if reach else ((5, 60) if second else (2, 0))
            claims.append(("look", m, ALL1 if m else ALL0, t, "full", want))
            claims.append(("link", m, t, 60 if second else (dd if dd <= 32767 else 0)))
        if not reach and not second:
            claims.append(("literals", 0, ALL0, t - 1, t + 2))
    cases.append(("E.reach", bytes(buf), claims))
    # two slides (on literals the window slides at strstart 65 275 and 98 043): 12-byte matches at distance MAX_DIST whose
    # targets lie just before, at and just behind the slide, one at MAX_DIST + 1, and the H7 tail after a slide (the last
    # 3 bytes equal an earlier "abcX", X the byte 32 KiB back)
    fence = _Fence()
    n = 3 * 32768 + 900
    buf = background(n)
    claims = [("slides", m, ALL1 if m else ALL0, 2) for m in (0, 1)]
    for k in (1, 2):
        slide = 32768 * k + MAX_DIST + 1
        for off, dd in ((-40, MAX_DIST), (0, MAX_DIST), (40, MAX_DIST), (80, MAX_DIST + 1), (120, MAX_DIST - 1)):
            t, lz_too = plant_clean(buf, dd, slide + off - dd, 12, fence)  # (slide + off, or a few positions behind it)
            assert t < slide + off + 20
            for m in (0, 1) if lz_too else (0,):
                if dd <= MAX_DIST:
                    claims.append(("match", m, ALL1 if m else ALL0, t, 12, dd, 0))
                else:
                    claims.append(("literals", m, ALL1 if m else ALL0, t - 1, t + 2))
    x = buf[n - 32768]
    src = n - 3 - 500
    buf[src:src + 4] = bytes(buf[n - 3:n]) + bytes([x])
    buf[src - 1] = 0xFB  # (not the byte in front of the tail)
    src0 = n - 3 - 900  # ... and an "abc\\0" for the other tail head: not in the chain the matcher takes after a slide
    buf[src0:src0 + 4] = bytes(buf[n - 3:n]) + b"\0"
    buf[src0 - 1] = 0xFB
    claims += [("tail", 0, src0), ("tail", 1, src), ("match", 0, ALL0, n - 3, 3, 500, 0)]
    cases.append(("E.slides", bytes(buf), claims))
    return cases


# ---------------------------------------------------------------------------------------------------------------
# F. the end of the input
def family_f():
    sweep, cases = _Sweep(11), []
    # the last 340 bytes are a copy of earlier ones: every position 3 .. 340 bytes in front of the end has a true
    # candidate and its match runs into the end; stream lengths 256 k + {-3 .. 3}
    for d in range(-3, 4):
        n = 256 * 6 + d
        buf = background(n)
        buf[n - 340:n] = buf[100:440]
        buf[99] = 3
        claims = [("look", m, ALL1 if m else ALL0, n - 300, "share3", True) for m in (0, 1)]
        claims += [("look", m, ALL1 if m else ALL0, n - 4, "share3", True) for m in (0, 1)]
        cases.append(("F.tail_copy_len%d" % n, bytes(buf), claims))
    # (those tail copies cover every offset.)  One position alone: a 12-byte true candidate for the position e bytes in
    # front of the end, e = 3 .. 24 and a sample of the rest with every e around MIN_LOOKAHEAD
    for e in range(3, 341, 1):
        if e > 24 and e % 16 not in (5, 6) and e not in (255, 256, 257, 258, 259, 260, 261, 262, 263, 340):
            continue
        pre = sweep()
        n = pre + 420
        buf = background(n)
        fence = _Fence()
        t = n - e
        ln = min(12, e)
        buf[40:40 + ln] = buf[t:t + ln]
        if ln < e:
            buf[40 + ln] = fence(buf[t + ln])
        buf[39] = fence(buf[t - 1])
        claims = []
        if e >= 4:
            claims.append(("look", 0, ALL0, t, "share3", True))
            claims.append(("match", 0, ALL0, t, ln, t - 40, 0))
        claims.append(("look", 1, ALL1, t, "share3", True))
        if ln >= 3:
            claims.append(("match", 1, ALL1, t, ln, t - 40, 0))
        cases.append(("F.end_minus%d_pre%d" % (e, pre), bytes(buf), claims))
    # lengths 0 .. 6
    for n in range(7):
        cases.append(("F.len%d_run" % n, b"w" * n, []))
        cases.append(("F.len%d_bg" % n, bytes(background(n)), []))
    # H7: the last 3 bytes hash with a 4th byte from beyond the data - zero before the first slide: they equal an
    # earlier "abc\0", at distance 4 096 (kept) and 4 097 (too far for a 3-byte match)
    for dd in (4096, 4097, 100):
        n = 4200 + dd % 7
        buf = background(n)
        src = n - 3 - dd
        buf[src:src + 4] = bytes(buf[n - 3:n]) + b"\0"
        buf[src - 1] = 0xFB  # (not the byte in front of the tail)
        claims = [("tail", 0, src)]
        if dd <= 4096:
            claims.append(("match", 0, ALL0, n - 3, 3, dd, 0))
        else:
            claims.append(("literals", 0, ALL0, n - 4, n))
        cases.append(("F.h7_zero_dist%d" % dd, bytes(buf), claims))
    # the data ends exactly at the end of the 64 KiB buffer: the window slides with nothing left to read, and the last
    # 3 bytes equal an earlier "abcX", X the byte 32 KiB back (H7 after a slide); a copied tail in front of them
    n = 65536
    buf = background(n)
    buf[n - 300:n - 10] = buf[n - 9000:n - 8710]
    x = buf[n - 32768]
    src = n - 3 - 500
    buf[src:src + 4] = bytes(buf[n - 3:n]) + bytes([x])
    buf[src - 1] = 0xFB  # (not the byte in front of the tail)
    cases.append(("F.len65536_h7_after_slide", bytes(buf),
                  [("tail", 1, src), ("slides", 0, ALL0, 1), ("match", 0, ALL0, n - 3, 3, 500, 0),
                   ("look", 0, ALL0, n - 200, "share3", True)]))
    return cases


# ---------------------------------------------------------------------------------------------------------------
# G. lazy chains
def staircase(buf, p, k, fence, first=4, src0=None):
    """positions p + j, j = 0 .. k, match first + j bytes, each from a source of its own in front of p; -> end of the
    sources"""
    src = src0
    for j in range(k + 1):
        ln = first + j
        plant(buf, p + j, src, ln, fence)
        src += ln + 3
    return src


def _stair_size(k, first=4):
    return sum(first + j + 3 for j in range(k + 1))


def stair_claims(p, k, first, matcher):
    """the chain of deferrals goes on while the match before is shorter than max_lazy"""
    claims = []
    # (Lz's hash puts background positions into these chains: where the quartered budget is small they hide the source)
    for lv in (_levels_where(lambda c: c.max_chain >= 128, 1) if matcher else ALL0):
        ml = M.config(matcher, lv).max_lazy
        d = min(k, max(0, ml - first))
        claims.append(("match", matcher, (lv,), p + d, first + d, None, d))
    return claims


def _stairs_case(pre, k, first):
    fence = _Fence()
    p = pre + 4 + _stair_size(k, first) + 10
    buf = background(p + k + first + k + 330)
    staircase(buf, p, k, fence, first, pre + 4)
    claims = stair_claims(p, k, first, 1)
    if first == 4:
        claims += stair_claims(p, k, first, 0)
    return buf, claims, p


def _back_to_back_case(pre, total):
    """three matches back to back: total - 30, 30 and 6 bytes; -> the start of the third"""
    fence = _Fence()
    p = pre + 300
    buf = background(p + 500)
    a = total - 30
    plant(buf, p, pre + 4, a, fence)
    plant(buf, p + a, pre + 100, 30, fence)
    plant(buf, p + total, pre + 150, 6, fence)
    claims = [("match", 0, ALL0, p, a, None, 0), ("match", 0, ALL0, p + a, 30, None, 0),
              ("match", 0, ALL0, p + total, 6, None, 0), ("match", 1, ALL1, p + total, 6, None, 0)]
    return buf, claims, p + total


def _deep_case(pre, where, seed):
    """a position whose chain is longer than the look-ahead walks (130 links > KSPEC) -> that position"""
    fence = _Fence()
    buf, t, dl, dn = chain_stream(pre + 120, 130, 129, head_seed=seed, tail=400)
    members = 131 if where == "in_stairs" else 130  # (the source of t - 1's match holds the head too)
    claims = [("look", 0, (7, 8, 9), t, "walked", members), ("look", 0, (7, 8, 9), t, "full", (7, dl))]
    if where == "behind_match":
        plant(buf, t - 8, pre + 4, 8, fence)
        claims += [("match", 0, ALL0, t - 8, 8, None, 0), ("call", 0, (7, 8, 9), t, 2, 130)]
    elif where == "in_stairs":
        # t - 2 matches 5, t - 1 matches 6 (their sources end before the head), t matches 7 through link 129
        plant(buf, t - 2, pre + 4, 5, fence)
        plant(buf, t - 1, pre + 20, 6, fence)
        claims += [("match", 0, (7, 8, 9), t, 7, dl, 2)]
    else:
        claims += [("call", 0, (7, 8, 9), t, 2, 130), ("match", 0, (7, 8, 9), t, 7, dl, 0)]
    return buf, claims, t


def _run_case(pre, run, variant, k=0):
    """a 10-byte match, `run` match-free positions, an 11-byte match; in the run no head at all (variant 0) or a chain of
    fingerprint-only candidates (1) -> the run's end"""
    fence = _Fence()
    p = pre + 60
    q = p + 10 + run          # the first match covers [p, p + 10); the second starts `run` positions behind it
    buf = background(q + 360)
    plant(buf, p, p - 56, 10, fence)
    plant(buf, q, p - 36, 11, fence)
    claims = [("match", m, ALL1 if m else ALL0, p, 10, None, 0) for m in (0, 1)]
    claims += [("match", m, ALL1 if m else ALL0, q, 11, None, 0) for m in (0, 1)]
    claims += [("literals", m, ALL1 if m else ALL0, p + 10, q) for m in (0, 1)]
    if variant == 1:
        for m in (0, 1):
            a, b = liars(m)[k % 6]
            at = p + 20 + 8 * m
            buf[at:at + len(b)] = b
            buf[at + 12:at + 12 + len(a)] = a
            for x in (at - 1, at + len(b), at + 11, at + 12 + len(a)):  # (the bytes around them join no match either)
                buf[x] = fence()
            claims += [("look", m, ALL1 if m else ALL0, at + 12, "share3", False), ("link", m, at + 12, 12)]
    return buf, claims, q


def family_g():
    sweep, cases = _Sweep(9), []
    ks = [1, 2, 3, 4, 5, 11, 12, 13, 14, 27, 28, 29, 30, 62, 63, 64, 65, 66, 78, 79, 80, 81, 82, 100, 124, 125, 126]
    for k in ks:
        for first in (4, 3):
            if first == 3 and k not in (1, 2, 3, 13, 14, 29, 30, 64, 80):
                continue
            pre = sweep()
            buf, claims, _ = _stairs_case(pre, k, first)
            cases.append(("G.stairs%d_from%d_pre%d" % (k, first, pre), bytes(buf), claims))
    # p + 1 matches as long as p (the match at p goes out) / longer by one (it gives way)
    for delta in (0, 1):
        pre, fence = sweep(), _Fence()
        p = pre + 80
        buf = background(p + 400)
        plant(buf, p, pre + 4, 9, fence)
        plant(buf, p + 1, pre + 30, 9 + delta, fence)
        lv0 = _levels_where(lambda c: c.max_lazy > 9)
        lv1 = _levels_where(lambda c: c.max_lazy > 9, 1)
        want = (p + 1, 10, 1) if delta else (p, 9, 0)
        cases.append(("G.next_%s_pre%d" % ("longer" if delta else "equal", pre), bytes(buf),
                      [("match", 0, lv0, want[0], want[1], None, want[2]),
                       ("match", 1, lv1, want[0], want[1], None, want[2])]))
    # the quarter mark of a quartered walk: p holds a match of good_length bytes, so p + 1 is searched over
    # q = max_chain >> 2 candidates; its only longer candidate is link q of its chain (found: the match at p gives way)
    # or link q + 1 (not found: the match at p goes out).  The members stand as far apart as the long candidate must be
    # long to beat good_length.  (Level 9: 1 025 members 40 bytes apart do not fit the window.)
    for lv, unit_len in ((2, 7), (3, 7), (5, 12), (6, 12), (7, 12), (8, 40)):
        cfg = M.config(0, lv)
        q, good = cfg.max_chain >> 2, cfg.good_length
        assert good < unit_len and good < cfg.max_lazy
        for i in (q, q + 1):
            pre, fence = sweep(), _Fence()
            buf, t, dl, dn = chain_stream(pre + 60, q + 4, i, head_seed=200 + 2 * lv + i - q, unit_len=unit_len)
            plant(buf, t - 1, pre + 4, good, fence)
            claims = [("call", 0, (lv,), t, good, q)]
            if i <= q:
                claims.append(("match", 0, (lv,), t, unit_len, dl, 1))
            else:
                claims.append(("match", 0, (lv,), t - 1, good, None, 0))
            cases.append(("G.quarter_level%d_link%d_pre%d" % (lv, i, pre), bytes(buf), claims))
    # a match at p of good_length - 1 / good_length bytes; p + 1 is the target of a chain of 20 whose long candidate is
    # link 12: behind the quarter mark of levels 3 and 5 (max_chain 32), within the full chain
    for ln in (7, 8):
        pre, fence = sweep(), _Fence()
        buf, t, dl, dn = chain_stream(pre + 40, 20, 12, head_seed=40 + ln)
        p = t - 1
        # p's own match: ln bytes from a source in the lead (the target's head is part of them)
        plant(buf, p, pre + 4, ln, fence)
        cfg5 = M.config(0, 5)
        assert cfg5.good_length == 8 and cfg5.max_chain == 32
        claims = [("look", 0, (5,), t, "full", (7, dl)), ("look", 0, (5,), t, "quarter", (4, dn)), ("look_differs", 0, (5,), t)]
        if ln >= 8:   # prev_length >= good_length: the quartered walk
            claims.append(("call", 0, (5,), t, ln, 8))
        else:
            claims.append(("call", 0, (5,), t, ln, 21))  # (p's source holds the head too: 21 members)
        cases.append(("G.good_length_prev%d_pre%d" % (ln, pre), bytes(buf), claims))
    # the same where it decides: p matches 5 bytes (levels 1 .. 4: good_length 4 -> quartered; levels 5 .. 7: full), the
    # long candidate of p + 1 (7 bytes) is link 12 of 20
    pre, fence = sweep(), _Fence()
    buf, t, dl, dn = chain_stream(pre + 40, 20, 12, head_seed=77)
    p = t - 1
    plant(buf, p, pre + 4, 5, fence)
    cases.append(("G.good_length_decides_pre%d" % pre, bytes(buf),
                  [("match", 0, (5, 6, 7), t, 7, dl, 1), ("match", 0, (3,), p, 5, None, 0),
                   ("call", 0, (3,), t, 5, 8), ("call", 0, (5, 6, 7), t, 5, 21)]))
    # matches back to back, of lengths that end 63 / 64 / 65 / 79 / 80 / 81 positions behind the first one's start
    for total in (63, 64, 65, 79, 80, 81):
        pre = sweep()
        buf, claims, _ = _back_to_back_case(pre, total)
        cases.append(("G.back_to_back_%d_pre%d" % (total, pre), bytes(buf), claims))
    # a position whose chain is longer than the look-ahead walks: as the first position after literals, directly behind
    # a match's end, and in the middle of a staircase
    for where in ("first", "behind_match", "in_stairs"):
        pre = sweep()
        buf, claims, _ = _deep_case(pre, where, 90 + len(where))
        cases.append(("G.deep_%s_pre%d" % (where, pre), bytes(buf), claims))
    # Lz only (hash4 never brings a 3-byte match together inside the data): a 3-byte match at distance 4 095 / 4 096 /
    # 4 097 as a chain's first match; behind a position whose own 3-byte match the TOO_FAR rule dropped (4 200 back:
    # this one is the first match again); and behind a kept 3-byte match, which it cannot beat at any distance
    for dd in (4095, 4096, 4097):
        for before in (None, 4200, 100):
            pre, fence = sweep(), _Fence()
            t = pre + 4300
            buf = background(t + 330)
            plant(buf, t, t - dd, 3, fence)
            if before:
                plant(buf, t - 1, t - 1 - before, 3, fence)
            if before == 100:
                claims = [("match", 1, ALL1, t - 1, 3, 100, 0), ("literals", 1, ALL1, t, t + 3)]
            elif dd <= 4096:
                claims = [("match", 1, ALL1, t, 3, dd, 0), ("literals", 1, ALL1, t - 2, t)]
            else:
                claims = [("literals", 1, ALL1, t - 2, t + 3)]
            claims.append(("look", 1, ALL1, t, "full", (3, dd)))
            cases.append(("G.too_far_%d_before%s_pre%d" % (dd, before, pre), bytes(buf), claims))
    cases += _ring_cases("G")
    return cases


# the look-ahead ring of the sequential kernel holds 1 024 positions (position & 1023): a staircase's start, the third of
# three matches back to back, an unsettled position and a literal run's end a few positions before, at and behind a
# multiple of 1 024
def _ring_cases(fam):
    builders = {"G": [("stairs5", lambda pre: _stairs_case(pre, 5, 4)), ("back_to_back_64", lambda pre: _back_to_back_case(pre, 64)),
                      ("deep_first", lambda pre: _deep_case(pre, "first", 120))],
                "H": [("run64", lambda pre: _run_case(pre, 64, 0)), ("run513_liars", lambda pre: _run_case(pre, 513, 1, 3))]}[fam]
    cases = []
    for what, build in builders:
        _, _, anchor0 = build(1)
        for d in (-2, 0, 1):
            pre = 1 + (d - anchor0) % 1024
            buf, claims, anchor = build(pre)
            assert anchor == anchor0 + pre - 1
            cases.append(("%s.ring_%s_at%+d" % (fam, what, d), bytes(buf), claims + [("ring", anchor, d)]))
    return cases


# ---------------------------------------------------------------------------------------------------------------
# H. literal runs between matches and the hand-over between the wave and lane 0
def family_h():
    sweep, cases = _Sweep(13), []
    # every run-length class (one step, one group of 8 steps, two groups) without a head in the run and with chains of
    # fingerprint-only candidates ...
    for k, run in enumerate([62, 63, 64, 65, 66, 510, 511, 512, 513, 514, 1022, 1023, 1024, 1025, 1026]):
        pre = sweep()
        buf, claims, _ = _run_case(pre, run, k % 2, k)
        cases.append(("H.run%d_v%d_pre%d" % (run, k % 2, pre), bytes(buf), claims))
    # ... and with a head out of reach (its source MAX_DIST + 1 back): one run of each class behind one lead of 32 KiB
    pre, fence = sweep(), _Fence()
    p = pre + MAX_DIST + 300
    buf = background(p + 64 + 513 + 1026 + 500)
    claims = []
    for j, run in enumerate((64, 513, 1026)):
        q = p + 10 + run
        plant(buf, p, pre + MAX_DIST + 30 * j, 10, fence)
        r, _ = plant_clean(buf, MAX_DIST + 1, p + 12 - MAX_DIST - 1, 10, fence)
        assert r + 10 < q
        claims += [("match", m, ALL1 if m else ALL0, p, 10, None, 0) for m in (0, 1)]
        claims += [("literals", m, ALL1 if m else ALL0, p + 10, q) for m in (0, 1)]
        claims += [("look", 0, ALL0, r, "full", (2, 0)), ("link", 0, r, MAX_DIST + 1)]
        p = q
    plant(buf, p, pre + MAX_DIST + 90, 11, fence)
    claims += [("match", m, ALL1 if m else ALL0, p, 11, None, 0) for m in (0, 1)]
    cases.append(("H.runs_head_out_of_reach_pre%d" % pre, bytes(buf), claims))
    cases += _ring_cases("H")
    return cases


# ---------------------------------------------------------------------------------------------------------------
# I. link order: equal hashes inside a 64-position step, across the 8 steps of a group, across the wavefronts' groups
def family_i():
    sweep, cases = _Sweep(17), []
    for delta in (1, 2, 63, 64, 65, 511, 512, 513, 8191, 8192, 8193):
        pre = sweep()
        p = pre + 70
        buf = background(p + delta + 340)
        if delta == 1:
            buf[p:p + 5] = b"\x02" * 5
        elif delta == 2:
            buf[p:p + 6] = b"\x02\x09" * 3
        else:
            place_heads(buf, [p, p + delta], seed=delta)
        cases.append(("I.pair_delta%d_pre%d" % (delta, pre), bytes(buf),
                      [("link", 0, p + delta, delta), ("link", 1, p + delta, delta)]))
    # 3, 5 and 40 members spread over a step, a group and a round of the 16 wavefronts' groups (40 members in a step: a
    # run, the heads overlap)
    for members in (3, 5, 40):
        for span in (64, 512, 8192):
            pre = sweep()
            p = pre + 70
            buf = background(p + span + 340)
            if 5 * members > span:
                buf[p:p + members + 3] = b"\x02" * (members + 3)
                at = [p + j for j in range(members)]
            else:
                at = [p + (span - 5) * j // (members - 1) for j in range(members)]
                place_heads(buf, at, seed=members + span)
            claims = []
            for x, y in zip(at, at[1:]):
                claims += [("link", 0, y, y - x), ("link", 1, y, y - x)]
            cases.append(("I.members%d_span%d_pre%d" % (members, span, pre), bytes(buf), claims))
    return cases


@functools.lru_cache(None)
def cases():
    out = []
    for fam in (family_a, family_b, family_c, family_d, family_e, family_f, family_g, family_h, family_i):
        out += fam()
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out


def family(name):
    return name[0]
