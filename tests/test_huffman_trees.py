"""The CPU side of tests/huffman_tree_cases.py: three witnesses for the Huffman trees the GPU tests compare against.
The oracle's T.make (oracle/de_deflate.c) equals the model's (tests/huffman_tree_model.py, written from the algorithm's
description); the oracle's whole block equals libz's Z_HUFFMAN_ONLY block wherever libz wrote one dynamic block; the
header the oracle wrote, read back by tests/deflate_header_model.py, carries the model's lengths and the payload
inflates to the plaintext.  test_coverage asserts that the families reach the paths they are named for."""
import zlib

import pytest

from tests import deflate_header_model as header_model
from tests import huffman_tree_cases as cases
from tests import huffman_tree_model as model
from tests.conftest import load_golden

FAMILIES = sorted(cases.FAMILIES)
_TREES = {}


def trees_of(case):
    """the model's three trees of a case, and the code-length frequencies between them"""
    if case.name not in _TREES:
        lt, dt = model.make(case.lit, 286, 15), model.make(case.dist, 30, 15)
        bl = model.scan(lt.lengths[:lt.max_code + 1], dt.lengths[:dt.max_code + 1])
        _TREES[case.name] = (lt, dt, model.make(bl, 19, 7), bl)
    return _TREES[case.name]


def _same_tree(oracle, freqs, length, max_length, want, what):
    mc, lens, codes, _ = oracle.tree_make(length, list(freqs), max_length)
    assert mc == want.max_code, what
    assert lens == want.lengths, what
    assert codes == want.codes, what


@pytest.mark.parametrize("name", ["tree_0", "tree_rfc5322_corpus"])
def test_model_reproduces_kats(name):
    c = next(c for c in load_golden("deflate_kat.json") if c["name"] == name)
    t = model.make(c["freqs"][:c["length"]], c["length"], 15)
    for sym, l in c["lengths"].items():
        assert t.lengths[int(sym)] == l, sym
    for sym, code in c["codes"].items():
        assert t.codes[int(sym)] == code, sym


def test_model_equals_oracle_without_symbols(oracle):
    """the tree of an empty histogram (what a command list cannot reach for the literal/length alphabet): 0 and 1 join"""
    for length, max_length in ((286, 15), (30, 15), (19, 7)):
        want = model.make([0] * length, length, max_length)
        assert (want.max_code, want.lengths[:3]) == (1, [1, 1, 0])
        _same_tree(oracle, [0] * length, length, max_length, want, length)


@pytest.mark.parametrize("family", FAMILIES)
def test_model_equals_oracle(oracle, family):
    for c in cases.FAMILIES[family]():
        lt, dt, ct, bl = trees_of(c)
        _same_tree(oracle, c.lit, 286, 15, lt, (c.name, "literal/length"))
        _same_tree(oracle, c.dist, 30, 15, dt, (c.name, "distance"))
        _same_tree(oracle, bl, 19, 7, ct, (c.name, "code length"))


def test_oracle_equals_libz(oracle):
    """every literal-only case that libz answers with one dynamic block: the oracle's block is libz's, byte for byte.
    libz pins 123 of the 152 literal-only cases of at most 32 767 bytes, all 12 too deep ones among them; the rest are
    short inputs for which it chose a stored or fixed block."""
    lit_only = [c for c in cases.all_cases() if cases.literal_only(c) and len(c.plain) <= 32767]
    pinned = []
    for c in lit_only:
        z = cases.libz_block(c.plain)
        if z is not None:
            assert oracle.encode_cmds(c.cmds, "dynamic") == z, c.name
            pinned.append(c.name)
    deep = [c.name for c in lit_only if trees_of(c)[0].limited]
    print("libz pinned %d of %d literal-only cases, %d of %d too deep ones" % (len(pinned), len(lit_only),
                                                                            len(set(deep) & set(pinned)), len(deep)))
    assert len(deep) >= 8 and set(deep) <= set(pinned)
    assert 2 * len(pinned) >= len(lit_only), (len(pinned), len(lit_only))


@pytest.mark.parametrize("family", FAMILIES)
def test_header_and_payload(oracle, family):
    for c in cases.FAMILIES[family]():
        z = oracle.encode_cmds(c.cmds, "dynamic")
        r = header_model.inflate(z, len(c.plain))
        lt, dt, ct, _ = trees_of(c)
        assert (r.status, r.consumed, r.tag, len(r.headers)) == (0, len(z), "ok", 1), c.name
        assert r.info["lit_lens"] == lt.lengths[:lt.max_code + 1], c.name
        assert r.info["dist_lens"] == dt.lengths[:dt.max_code + 1], c.name
        assert r.info["cl_lens"] == ct.lengths, c.name
        assert r.output == c.plain, c.name
        assert zlib.decompress(z, -15) == c.plain, c.name


def test_coverage():
    """what the families are there for, by the model's classification.  Reached: the 15-bit fix-up in 22
    literal/length trees (plain depths 16 .. 20) and 7 distance trees (16 .. 18), the 7-bit one in 9 code-length trees
    (plain depth 8)."""
    every = cases.all_cases()
    assert len({c.name for c in every}) == len(every)
    trees = {c.name: trees_of(c) for c in every}
    # heap sizes
    lit_sizes = {sum(1 for f in c.lit if f) for c in every}
    assert set(cases.SIZES) <= lit_sizes
    dist_sizes = {sum(1 for f in c.dist if f) for c in every}
    assert set(cases.DIST_SIZES) <= dist_sizes
    assert any(c.dist[29] and sum(1 for f in c.dist if f) == 1 for c in every)
    assert any(c.lit[285] and not any(c.lit[257:285]) for c in every)
    # the fix-ups
    lit_deep = [t[0].depth for t in trees.values() if t[0].limited]
    dist_deep = [t[1].depth for t in trees.values() if t[1].limited]
    cl_deep = [t[2].depth for t in trees.values() if t[2].limited]
    print("fix-up ran: literal/length %d cases (plain depths %s), distance %d (%s), code length %d (%s)"
          % (len(lit_deep), sorted(set(lit_deep)), len(dist_deep), sorted(set(dist_deep)), len(cl_deep), sorted(set(cl_deep))))
    assert len(lit_deep) >= 8
    assert any(d in (16, 17) for d in lit_deep) and any(d in (18, 19) for d in lit_deep) and any(d >= 20 for d in lit_deep)
    assert len(dist_deep) >= 4
    assert len(cl_deep) >= 4
    for n in (17, 18, 19):  # the tie-free counts are as deep as they are many
        assert model.plain_depth(cases.tie_free(n) + [1]) == n
    # the run-length pass: every run length across every step boundary, and at the end of the lengths
    lit_runs = [(v, s, n, t[0].max_code) for t in trees.values() for v, s, n in cases.runs_of(t[0].lengths[:t[0].max_code + 1])]
    dist_runs = [(v, s, n, t[1].max_code) for t in trees.values() for v, s, n in cases.runs_of(t[1].lengths[:t[1].max_code + 1])]
    for n in cases.NONZERO_RUNS:
        for b in cases.BOUNDARIES:
            assert any(v and k == n and cases.straddles(s, k, b) for v, s, k, _ in lit_runs), (n, b)
        assert any(v and k == n and s + k - 1 == mc for v, s, k, mc in lit_runs), n
        assert any(v and k == n and s + k - 1 == mc and mc > 256 for v, s, k, mc in lit_runs), n
        assert any(v and k == n and s + k - 1 == mc for v, s, k, mc in dist_runs), n
    for n in cases.ZERO_RUNS:
        for b in cases.BOUNDARIES[:3]:  # (256 always has a code)
            assert any(not v and k == n and cases.straddles(s, k, b) for v, s, k, _ in lit_runs), (n, b)
        assert any(not v and k == n and s + k == mc for v, s, k, mc in lit_runs), n
    for n in cases.DIST_ZERO_RUNS:
        assert any(not v and k == n and s + k == mc for v, s, k, mc in dist_runs), n
