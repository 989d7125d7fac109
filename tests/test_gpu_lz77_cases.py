"""tests/lz77_cases.py through the deflate kernels: what the link and match kernels leave in the front workspace against
tests/lz77_model.py (links, fingerprints, tail heads, look-ahead verdicts and results), the compressed bytes against the
oracle at every level and queue size, De.Lz77.compress against the oracle's commands, and the profiled kernel's counters
against what the model says lane 0 has to walk itself.  The CPU half (the claims, the model against the oracle and
libz) is tests/test_lz77_cases.py.  Needs an MI355X: `pytest -m gpu`."""
import os
import re
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import lz77_cases as K
from tests import lz77_model as M

pytestmark = pytest.mark.gpu

FL_ENDED, FL_MATCH = 2, 4
QUEUES = (16, 32, 64, 4096)
COMBOS = [(0, lv) for lv in K.ALL0] + [(1, lv) for lv in K.ALL1]


def _constant(name):
    """a constant of csrc/deflate_common.hpp, as the resource tests read theirs"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "decompress_amd", "csrc",
                        "deflate_common.hpp")
    with open(path) as f:
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, f.read())
    assert m, name
    return int(m.group(1))


KSPEC = _constant("KSPEC")


@pytest.fixture(scope="module")
def eng():
    import decompress_amd
    return decompress_amd.Engine(0)


@pytest.fixture(scope="module")
def cases():
    return K.cases()


def _representatives(cases):
    """one case per family: the largest of those below 10 KiB (the long chain, the long staircase, the long run ...),
    or the family's smallest"""
    best = {}
    for name, data, _ in sorted(cases, key=lambda c: len(c[1])):
        fam = K.family(name)
        if fam not in best or len(data) < 10240:
            best[fam] = (name, data)
    assert set(best) == set(K.FAMILIES)
    return [best[f] for f in K.FAMILIES]


# ---- the arrays ------------------------------------------------------------------------------------------------
def _fp16(data, count):
    a = np.frombuffer(data, dtype=np.uint8).astype(np.uint32)
    v = a[:count] | (a[1:count + 1] << 8) | (a[2:count + 2] << 16)
    return (v * np.uint32(0x9E3779B1)) >> np.uint32(16)


@pytest.mark.parametrize("matcher", [0, 1])
def test_links_fingerprints_and_tails(cases, matcher):
    from tests import deflate_front_probe as probe
    res = probe.run([d for _, d, _ in cases], matcher, 6)
    for i, (name, data, _) in enumerate(cases):
        dist, tails = M.links(data, matcher)
        assert int(res.p_end[i]) == len(dist) == M.p_end(data, matcher), name
        link = res.link(i)
        bad = np.nonzero((link & 0xFFFF) != np.array(dist, dtype=np.uint32))[0]
        assert not len(bad), (name, int(bad[0]), int(link[bad[0]] & 0xFFFF), dist[bad[0]])
        if len(data) >= 4:  # (a stream of 3 bytes has one string and nothing to compare its fingerprint with: none is written)
            bad = np.nonzero((link >> 16) != _fp16(data, len(dist)))[0]
            assert not len(bad), (name, int(bad[0]))
        if matcher == 0:
            assert tuple(int(x) for x in res.tail[i]) == tails, (name, res.tail[i], tails)


@pytest.mark.parametrize("matcher,level", COMBOS)
def test_look_ahead_sound_and_complete(cases, matcher, level):
    """flg / m / mq of every position of every case: a verdict is never wrong (soundness), and the positions the
    look-ahead can settle within min(max_chain, KSPEC) links are settled (completeness)"""
    from tests import deflate_front_probe as probe
    res = probe.run([d for _, d, _ in cases], matcher, level)
    kspec = min(M.config(matcher, level).max_chain, KSPEC)
    settled = 0
    for i, (name, data, _) in enumerate(cases):
        looks = M.look_ahead(data, matcher, level)
        if not looks:
            continue
        a = np.array([(x.full[0], x.full[1], x.quarter[0], x.quarter[1], x.walked, x.share3, x.near_end) for x in looks],
                     dtype=np.int64)
        flen, fdist, qlen, qdist, walked, share3, near = (a[:, k] for k in range(7))
        share3, near = share3.astype(bool), near.astype(bool)
        flg, m, mq = res.flg(i), res.m(i).astype(np.int64), res.mq(i).astype(np.int64)
        assert np.isin(flg, (0, FL_ENDED, FL_MATCH)).all(), name

        def first(mask):
            return (name, int(np.nonzero(mask)[0][0])) if mask.any() else None
        ended, matched = flg == FL_ENDED, flg == FL_MATCH
        # soundness
        assert first(ended & share3) is None, ("ended, but a candidate shares 3 bytes", first(ended & share3))
        assert first(matched & near) is None, ("a match read beyond the data", first(matched & near))
        for got, wlen, wdist, what in ((m, flen, fdist, "full"), (mq, qlen, qdist, "quartered")):
            bad = matched & ((got >> 16) != wlen)
            assert first(bad) is None, (what, "length", first(bad))
            bad = matched & (wlen > 2) & ((got & 0xFFFF) != wdist)
            assert first(bad) is None, (what, "distance", first(bad))
        # completeness
        bad = ~near & (walked <= kspec) & (flg == 0)
        assert first(bad) is None, ("not settled", first(bad))
        bad = near & share3 & (flg != 0)
        assert first(bad) is None, ("settled too close to the end", first(bad))
        bad = near & ~share3 & (walked <= kspec) & ~ended
        assert first(bad) is None, ("not ended", first(bad))
        settled += int((flg != 0).sum())
    assert settled


def _long_streams(cases):
    by = {n: d for n, d, _ in cases}
    one = by["E.slides"]
    two = by["E.reach"] + by["F.len65536_h7_after_slide"]
    # ... and 100 000 bytes of the families G, H, I on end, with both tail heads planted within a segment's reach
    three = bytearray(b"".join(d for n, d, _ in cases if n[0] in "GHI")[:100_000])
    n = len(three)
    three[n - 603:n - 599] = bytes(three[n - 3:n]) + b"\0"
    three[n - 303:n - 299] = bytes(three[n - 3:n]) + bytes([three[n - 32768]])
    return [one, two, bytes(three)]


def test_link_segments_equal_one_workgroup(cases):
    """three streams of about 100 KiB: md_launch_link_chunked at 16 KiB segments gives the one-workgroup kernel's link
    and tail, word for word, and the model's"""
    from tests import deflate_front_probe as probe
    for k, data in enumerate(_long_streams(cases)):
        assert 90_000 <= len(data) <= 110_000
        dist, tails = M.links(data, 0)
        # (a tail head further back than a segment's 32 KiB warm-up is never a candidate: the segments hand over 0)
        assert all(t == 0 or len(data) - 3 - t <= 32767 for t in tails), (k, tails)
        whole = probe.run([data], 0, 6)
        segs = probe.run([data], 0, 6, chunked_segment=16384)
        assert (whole.link(0) & 0xFFFF).tolist() == dist, k
        assert np.array_equal(whole.link(0), segs.link(0)), (k, np.nonzero(whole.link(0) != segs.link(0))[0][:4])
        assert tuple(int(x) for x in whole.tail[0]) == tuple(int(x) for x in segs.tail[0]) == tails, (k, whole.tail, segs.tail)


# ---- the bytes -------------------------------------------------------------------------------------------------
def _first_difference(got, want):
    from tests.deflate_tokens import tokens
    try:
        a, b = tokens(got), tokens(want)
    except Exception as e:  # a stream that does not parse: say so, the assertion on the bytes follows
        return "unparsable (%r)" % (e,)
    for k, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return "token %d: got %r, want %r" % (k, x, y)
    return "lengths %d / %d tokens" % (len(a), len(b))


def _bytes_equal_oracle(eng, oracle, cases, level, driver, matcher, queues=QUEUES):
    bufs = [d for _, d, _ in cases]
    with ThreadPoolExecutor(16) as ex:  # (ctypes releases the GIL)
        wants = {q: list(ex.map(lambda d, q=q: oracle.deflate_raw(d, level, q, driver, True, matcher), bufs)) for q in queues}
    for q in queues:
        res = eng.deflate_many(bufs, level=level, queue=q, driver=driver, matcher=matcher,
                               caps=[len(w[0]) + 3 if w[0] is not None else 64 for w in wants[q]])
        for (name, data, _), (st, out, adler), (want, wadler) in zip(cases, res, wants[q]):
            if want is None:  # De.Queue.Full in the reference (the CLI driver's end-of-block push)
                assert (st, out) == (13, b""), (name, level, q)
                continue
            assert st == 0, (name, level, q, st)
            if out != want:
                print(name, level, q, driver, matcher, _first_difference(out, want))
            assert out == want, (name, level, q, len(out), len(want))
            assert adler == wadler == zlib.adler32(data)


@pytest.mark.parametrize("level", K.ALL0)
def test_bytes_equal_oracle(eng, oracle, cases, level):
    _bytes_equal_oracle(eng, oracle, cases, level, 0, 0)


@pytest.mark.parametrize("driver,level", [(1, 4), (2, 7)], ids=["De.Higher", "CLI"])
def test_bytes_equal_oracle_other_drivers(eng, oracle, cases, driver, level):
    _bytes_equal_oracle(eng, oracle, cases, level, driver, 0)


@pytest.mark.parametrize("level", K.ALL1)
def test_bytes_equal_oracle_lz_matcher(eng, oracle, cases, level):
    _bytes_equal_oracle(eng, oracle, cases, level, 0, 1)


def test_lz77_alone_equals_oracle(eng, oracle, cases):
    """De.Lz77.compress / Lz.compress on their own are one launch per call: one representative per family"""
    from decompress_amd import de
    for name, data in _representatives(cases):
        for matcher, level, q in ((0, 1, 16), (0, 6, 4096), (0, 9, 64), (1, 4, 4096), (1, 9, 16)):
            got = de.Lz77.compress(data, level=level, queue=q, matcher=matcher)
            want = oracle.lz77_all(data, level=level, queue=q, matcher=matcher)
            assert got[0] == want[0], (name, matcher, level, q, len(got[0]), len(want[0]))
            assert (got[1], got[2]) == (want[1], want[2]), (name, matcher, level, q)


# ---- the paths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [6, 9])
def test_profiled_paths(eng, cases, level):
    """one representative per family alone under the profiled kernel: the unprofiled bytes; lane 0 walked (word 14) at
    least the links of the longest_match calls nobody else can serve - those at positions the look-ahead leaves
    unsettled (more than min(max_chain, KSPEC) links, or too close to the end with a candidate that shares 3 bytes); the wave wrote commands (word 10) for
    the lazy-chain and literal-run families"""
    kspec = min(M.config(0, level).max_chain, KSPEC)
    for name, data in _representatives(cases):
        want = eng.deflate_many([data], level=level, queue=4096)
        eng.set_option("profile", 1)
        try:
            got = eng.deflate_many([data], level=level, queue=4096)
            p = eng.get_profile_raw()
        finally:
            eng.set_option("profile", 0)
        assert got == want and got[0][0] == 0 and zlib.decompress(got[0][1], -15) == data, name
        parse = M.parse(data, 0, level, 4096)
        ahead = M.p_end(data, 0)  # (the call at position len - 3, the tail, is lane 0's own as well)
        looks = M.look_ahead(data, 0, level, sorted({c.pos for c in parse.calls if c.pos < ahead}))
        # (too close to the end the look-ahead still settles a position none of whose candidates shares 3 bytes)
        own = sum(c.walked for c in parse.calls
                  if c.pos >= ahead or looks[c.pos].walked > kspec or (looks[c.pos].near_end and looks[c.pos].share3))
        print(name, "level", level, "lane 0 must walk", own, "profile words", list(p))
        assert p[14] >= own, (name, p[14], own)
        if K.family(name) in "GH":
            assert p[10] > 0, (name, list(p))
