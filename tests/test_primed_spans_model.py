"""CPU-side checks of the model of PRIMED joined spans (tests/primed_spans_model.py): with no prefix the witness
built on the oracle (tests/primed_oracle.c) is the oracle itself; for Lz's matcher its decisions are libz's with the prefix
as preset dictionary; every expected stream is one that libz and the oracle's inflaters read to the end; the case list
holds the families it is meant to hold - asserted from the model's tokens; and priming makes the 40 KiB text cases shorter."""
import zlib

import pytest

from tests import deflate_spans_model as U
from tests import primed_spans_model as P
from tests.deflate_tokens import tokens

CASES = P.cases()
BY_NAME = {c[0]: c for c in CASES}
IDS = [c[0] for c in CASES]


def _toks(raw):
    return [t for t in tokens(raw) if t[0] != "B"]


def test_without_a_prefix_the_witness_is_the_oracle(oracle):
    """first = 0 on every span of every case of deflate_spans_model: the restated driver loop is the oracle's"""
    seen = set()
    for name, data, span, params in U.cases():
        p = (params.get("level", 6), params.get("queue", 4096), params.get("driver", U.ZL), params.get("dynamic", True), params.get("matcher", 0))
        for t in U.spans_of(data, span):
            if (t, p) in seen:
                continue
            seen.add((t, p))
            want, _ = oracle.deflate_raw(t, *p)
            assert P.primed_raw(t, 0, *p) == want, (name, len(t))
    # ... and with one span (nothing in front of it) the primed model is the unprimed one
    for data in (b"", U._text(3, 5000)):
        for fmt in (P.DEFLATE, P.ZLIB, P.GZIP):
            assert P.expected(data, 1 << 20, fmt) == U.expected(data, 1 << 20, fmt)


@pytest.mark.parametrize("name,data,span,params", CASES, ids=IDS)
def test_lz_matcher_decides_as_libz_with_the_prefix_as_dictionary(name, data, span, params):
    """Lz is zlib's deflate_slow: the tokens of every primed body equal those of libz given the prefix as zdict (levels 4 - 9;
    below 4 libz runs deflate_fast and Lz runs level 4)"""
    level = params.get("level", 6)
    if level < 4:
        level = 4
    q = dict(level=level, queue=params.get("queue", 4096), matcher=1)
    rs = P.raws(bytes(data), span, **q)
    for (s, e, w), raw in zip(P.prefixes(len(data), span), rs):
        args = (level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY)
        c = zlib.compressobj(*args, zdict=bytes(data[s - w:s])) if w else zlib.compressobj(*args)
        z = c.compress(bytes(data[s:e])) + c.flush()
        # libz lowers nice_match to the look-ahead once that is shorter (deflate.c longest_match: "if ((uInt)nice_match >
        # s->lookahead) nice_match = (int)s->lookahead"), Lz does not (lib/lz.ml), so within MAX_MATCH of the end the two may
        # take equally long matches at different distances - primed or not.  Everything that begins in front of that is held equal.
        # (Where libz stores a block - random bytes - its decisions are not in the stream: what lies in front of that is compared.)
        edge = min([e - s - 258] + [t[2] for t in tokens(z) if t[0] == "B" and t[1] == 0])
        mine, libz = _toks(raw), _toks(z)
        assert [t for t in mine if t[0] < edge] == [t for t in libz if t[0] < edge], (name, s, w)
        assert zlib.decompress(raw, -15, 0) == data[s:e] if not w else zlib.decompressobj(-15, zdict=bytes(data[s - w:s])).decompress(raw) == data[s:e]


@pytest.mark.parametrize("name,data,span,params", CASES, ids=IDS)
def test_expected_is_a_stream_every_inflater_reads(oracle, name, data, span, params):
    plain = dict(P.GZ_HEADER, hcrc=False)
    for fmt, wbits, hdr in ((P.DEFLATE, -15, None), (P.ZLIB, 15, None), (P.GZIP, 31, plain), (P.GZIP, None, P.GZ_HEADER)):
        want = P.expected(data, span, fmt, header=hdr, **params)
        if want is None:
            assert name == "queue-full"
            continue
        if wbits is not None:
            d = zlib.decompressobj(wbits)
            assert d.decompress(want) == data and d.eof and d.unused_data == b""
        cap = len(data) + 64
        if fmt == P.DEFLATE:
            assert oracle.de_inflate(want, cap) == (0, len(want), data)
        elif fmt == P.ZLIB:
            assert oracle.zl_inflate(want, cap) == (0, len(want), data)
        else:
            st, used, out, _ = oracle.gz_inflate(want, cap)
            assert (st, used, out) == (0, len(want), data)


def _case(name):
    _, data, span, params = BY_NAME[name]
    return bytes(data), span, params


def test_family_prefix_growth_and_odd_spans():
    data, span, _ = _case("growth")
    assert [w for _, _, w in P.prefixes(len(data), span)] == [4096 * i for i in range(9)] + [32768] * 4
    assert P.prefixes(len(data), span)[-1][:2] == (48 << 10, (48 << 10) + 1)
    data, span, _ = _case("odd-5000")
    assert [s % 2 for s, _, _ in P.prefixes(len(data), span)] == [0, 0, 0, 0, 0] and span % 64 and 5000 % 16  # unaligned starts
    assert [s for s, _, _ in P.prefixes(len(data), span)][1] == 5000


def test_family_first_match_from_the_prefix():
    data, span, params = _case("prefix-only")
    first = P.span_tokens(data, span, 1, **params)[0]
    assert first == (0, "M", 40, 1900) and first[3] >= first[2]  # source wholly in the prefix
    data, span, params = _case("prefix-only-byte-in-front")  # De's first longest_match also compares the byte in front
    assert P.span_tokens(data, span, 1, **params)[:2] == [(0, "L", data[2000]), (1, "M", 39, 1900)]
    data, span, params = _case("prefix-only-byte-in-front-lz")  # Lz's does not
    assert P.span_tokens(data, span, 1, **params)[0] == (0, "M", 40, 1900)
    data, span, params = _case("straddle")
    first = [t for t in P.span_tokens(data, span, 1, **params) if t[1] == "M"][0]
    assert first[0] <= 1 and first[3] == 2 and first[2] > first[3]  # source starts in the prefix and runs into the span
    # ... and unprimed neither span can do that
    assert U.expected(data, span, U.DEFLATE) != P.expected(data, span, P.DEFLATE)


def test_family_max_dist_and_nil():
    data, span, params = _case("max-dist")
    _, t1, t2 = P._max_dist()
    toks = P.span_tokens(data, span, 1, **params)
    assert (t1 - span, "M", 12, P.MAX_DIST) in toks  # the only earlier occurrence, at MAX_DIST exactly: taken
    assert all(t[3] <= P.MAX_DIST for t in toks if t[1] == "M")
    lit = {t[0] for t in toks if t[1] == "L"}
    assert all(t2 - span + k in lit for k in range(12))  # one further: not taken
    data, span, params = _case("nil")
    _, t = P._nil()
    assert data.find(data[t:t + 3]) == 0 and data.find(data[t:t + 3], 1) == t  # the only earlier occurrence is offset 0
    for i, (s, e, w) in enumerate(P.prefixes(len(data), span)):
        for tok in P.span_tokens(data, span, i, **params):
            assert tok[1] == "L" or s + tok[0] - tok[3] > s - w  # no source at position 0 of X_i
    lit = {tok[0] for tok in P.span_tokens(data, span, 1, **params) if tok[1] == "L"}
    assert all(t - span + k in lit for k in range(3))


def test_family_short_last_spans_and_slides():
    for k in (1, 2, 3):
        data, span, params = _case("short-last-%d" % k)
        pf = P.prefixes(len(data), span)
        assert pf[-1] == (33000, 33000 + k, 32768)
        assert [t[1] for t in P.span_tokens(data, span, 1, **params)] == ["L"] * k  # (fewer than MIN_MATCH + 1 bytes: literals)
    # De.Lz77 slides when strstart - base >= WSIZE + MAX_DIST = 65 274, seen by the fill at the first position behind it the
    # matcher stops at: X_i of these spans is 65 274, 65 275, 65 276 bytes long, and 98 304
    for ln in (32506, 32507, 32508):
        data, span, _ = _case("slide-%d" % ln)
        s, e, w = P.prefixes(len(data), span)[2]
        assert w == 32768 and e - s + w == 32768 + ln and ln + 32768 - 65275 in (-1, 0, 1)
    data, span, _ = _case("slide-65536")
    s, e, w = P.prefixes(len(data), span)[1]
    assert w == 32768 and e - s + w >= 65275 + 32768  # two slides inside the span
    names = [c[0] for c in CASES]
    for part in ("F.tail_copy_len", "F.end_minus3_", "F.end_minus262_", "F.h7_zero_dist4096", "F.len65536_h7_after_slide", "F.len0_run"):
        assert any(n.startswith(part) for n in names), part
    for name, data, span, params in CASES:
        if name.startswith("F.") and len(data) > 32768:  # (the empty text: one span, nothing behind the prefix)
            assert span == 32768 and P.prefixes(len(data), span)[1][2] == 32768


def test_family_grid_queue_full_repeat_alternating_checksums():
    grid = [c for c in CASES if c[0].startswith("text40k-")]
    assert {(p.get("level", 6), p.get("dynamic", True)) for _, _, _, p in grid if "driver" not in p and not p.get("matcher")} == \
        {(lv, dy) for lv in (0, 1, 4, 6, 9) for dy in (False, True)}
    assert {(p["driver"], p["matcher"]) for _, _, _, p in grid if "driver" in p} == {(d, m) for d in (P.HIGHER, P.CLI) for m in (0, 1)}
    assert all(span == 4096 and p["queue"] == 256 and len(d) == 40 << 10 for _, d, span, p in grid)
    full = [name for name, data, span, params in CASES if P.forms(data, span, **params) is None]
    assert full == ["queue-full"]
    data, span, params = _case("repeat")
    assert [f[0] for f in U.forms(data, span, **params)] == ["S"] * 8 and len(U.expected(data, span, U.DEFLATE)) > 8 * 4096
    f = P.forms(data, span, **params)
    assert [x[0] for x in f] == ["S"] + ["J"] * 7
    assert len(P.expected(data, span, P.DEFLATE)) < 4096 + 8 * 64
    data, span, params = _case("alternating")
    assert {x[0] for x in P.forms(data, span, **params)} == {"J", "S"}
    assert {"ff-5551", "ff-5552", "ff-5553", "ff-65521"} <= set(BY_NAME)


def test_priming_makes_the_text_cases_strictly_shorter():
    for name, data, span, params in CASES:
        if name.startswith("text40k-") and params.get("level", 6) != 0:
            for fmt in (P.DEFLATE, P.ZLIB, P.GZIP):
                assert len(P.expected(data, span, fmt, **params)) < len(U.expected(data, span, fmt, **params)), (name, fmt)
