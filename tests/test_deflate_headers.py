"""(CPU) The header corpus (tests/deflate_header_cases.py) is what it claims: on every stream the plain model
(tests/deflate_header_model.py) equals the CPU oracle in status, consumed and bytes; the model's reason tag is the rule
the case is named for, so a case reaches its rule and not an earlier one; zlib agrees wherever zlib accepts the header;
each placing is on its side of the run-length loop's two forms.  And the corpus is sensitive: for each of the model's
named defects some stream tells the defective model from the oracle."""
import hashlib
import zlib

import pytest

from tests import deflate_header_model as model
from tests.deflate_header_cases import (DIST_592, DIST_594, FAMILIES, KMAX, LIT_840, LIT_854, LIT_BEST, PLENTY, STAGE, UNBOUNDED,
                                        from_hist)
from tests.deflate_writer import Bits, Block, expand, write

TAGS = ["cl_over", "cl_incomplete", "cl_empty_slot", "rep16_first", "run_overflow", "no_eob", "lit_over", "lit_incomplete",
        "dist_over", "dist_incomplete", "lit_enough", "dist_enough", "eoi_at:hlit", "eoi_at:cl_lens", "eoi_at:cl_sym",
        "eoi_at:rep_extra", "ok"]
_MODEL, _ORACLE = {}, {}


def _model(raw, cap):
    if (raw, cap) not in _MODEL:
        _MODEL[(raw, cap)] = model.inflate(raw, cap)
    return _MODEL[(raw, cap)]


def _oracle(oracle, raw, cap):
    if (raw, cap) not in _ORACLE:
        _ORACLE[(raw, cap)] = oracle.de_inflate(raw, cap)
    return _ORACLE[(raw, cap)]


def test_geometry_is_read_from_the_kernel():
    assert (KMAX, PLENTY) == (64, 316 * 14 + 64) and STAGE % 16 == 0 and STAGE > 1024


@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_model_equals_oracle_and_reaches_the_rule(oracle, fam):
    cases = FAMILIES[fam]()
    assert len({c[0] for c in cases}) == len(cases)
    for name, raw, cap, tag in cases:
        r = _model(raw, cap)
        assert (r.status, r.consumed, r.output) == _oracle(oracle, raw, cap), (name, r.status, r.tag)
        if tag is not None:
            assert r.tag == tag, (name, r.tag)
        if r.tag not in ("ok", None):  # a header failed
            assert r.status == (1 if r.tag.startswith("eoi_at:") else 4) and r.consumed == 0, name
        if r.status == 0:
            assert r.consumed <= len(raw), name


def test_every_tag_has_a_stream():
    have = {c[3] for fam in FAMILIES.values() for c in fam()}
    assert have - {None} == set(TAGS)


@pytest.mark.parametrize("fam", ["H1", "H2", "H3"])
def test_placings(fam):
    """' /mid' streams have at least PLENTY bits behind the code-length code's lengths (the unchecked run-length loop),
    ' /end' streams fewer (the checked one) - counted the way the kernel counts: from the bit behind the HCLEN fields to
    the end of the stream"""
    seen = set()
    for name, raw, cap, _ in FAMILIES[fam]():
        info = _model(raw, cap).info
        if "hclen" not in info:
            continue
        left = 8 * len(raw) - (info["start"] + 17 + 3 * info["hclen"])
        assert name.endswith((" /mid", " /end")), name
        assert (left >= PLENTY) == name.endswith(" /mid"), (name, left)
        seen.add(name[-4:])
    assert seen == {"/mid", "/end"}


def _zlib_takes(r):
    """zlib reads these headers the same way: at most 286 / 30 lengths, complete codes (or one 1-bit code), and no
    unused slot and no empty distance table read (zlib has no code there)"""
    for h in r.headers:
        if "end" not in h or h["hlit"] > 286 or h["hdist"] > 30 or h["slots"] or h["empty_reads"]:
            return False
        for ls in (h["lit_lens"], h["dist_lens"]):
            over, left = model.kraft(ls)
            if any(ls) and left and sorted(ls)[-2:] != [0, 1]:
                return False
    return True


def test_zlib_agrees_where_it_accepts_the_header(oracle):
    count = 0
    for fam in FAMILIES.values():
        for name, raw, cap, _ in fam():
            r = _model(raw, cap)
            if r.status != 0 or not _zlib_takes(r):
                continue
            d = zlib.decompressobj(-15)
            assert d.decompress(raw) == r.output and d.eof and d.unused_data == raw[r.consumed:], name
            count += 1
    assert count > 150, count


def test_corpus_covers_what_it_lists():
    """H1's table shapes by the model's count: no sub-tables and every sub-table width 1..6 for both alphabets, several
    widths in one table, the 592-entry, the 840-entry and the 852-entry tables; H2's HCLEN values; H5's places"""
    lit_w, dist_w, lit_need, dist_need, mixed, hclen = set(), set(), set(), set(), 0, set()
    for name, raw, cap, tag in FAMILIES["H1"]() + FAMILIES["H2"]():
        r = _model(raw, cap)
        if tag != "ok":
            continue
        h = r.info
        assert r.status == 0, name
        if name.startswith("H2 hclen"):
            hclen.add(h["hclen"])
            if "needed" in name:
                assert h["hclen"] == int(name.split()[2]), name
        lw, dw = model.table_shape(h["lit_lens"], 9)[1], model.table_shape(h["dist_lens"], 6)[1]
        lit_w |= set(lw) or {0}
        dist_w |= set(dw) or {0}
        mixed += len(set(lw)) >= 3
        lit_need.add(h["lit_need"])
        dist_need.add(h["dist_need"])
    assert lit_w >= set(range(7)) and dist_w >= set(range(7)) and mixed >= 3
    assert 592 in dist_need and max(dist_need) == 592 and 840 in lit_need and max(lit_need) == 852
    assert hclen == set(range(5, 20))
    assert model.table_need(from_hist(DIST_592), 6) == 592 and model.table_need(from_hist(LIT_840), 9) == 840
    assert [model.table_need(from_hist(DIST_594[n]), 6) for n in (31, 32)] == [594, 594]
    assert [(sum(LIT_BEST[n]), model.table_need(from_hist(LIT_BEST[n]), 9)) for n in (286, 287, 288)] == [(286, 852), (287, 852), (288, 852)]
    assert (sum(LIT_854), model.table_need(from_hist(LIT_854), 9)) == (288, 854)
    h5 = [c[0] for c in FAMILIES["H5"]()]
    for k in (0, KMAX - 1, KMAX, KMAX + 1, 2000):
        assert sum(1 for n in h5 if n.endswith("after %d /mid" % k)) == 4, k
    assert len(UNBOUNDED) == 30 and all(_model(c[1], c[2]).status == 2 for c in FAMILIES["H5"]() if c[0] in UNBOUNDED)
    slots = [_model(c[1], c[2]).info["slots"] for c in FAMILIES["H5"]() if "lone dist code" in c[0]]
    assert slots and all(s == 2 for s in slots)  # both hand-made distances were read from the unused slot


# ---- the corpus notices a wrong reader ------------------------------------------------------------
# One defect cannot change what a reader returns, only why: every check between the last length and the first token
# answers Invalid_dictionary without reading input, so their order is invisible in (status, consumed, bytes).  For that
# one the stream that tells is the one whose reason tag changes (two faults in one header).
TAG_ONLY = {"no_eob_late"}


@pytest.mark.parametrize("defect", sorted(model.DEFECTS))
def test_defect_is_caught(oracle, defect):
    by_result, by_tag = [], []
    for fam in ("H1", "H2", "H3", "H5"):
        for name, raw, cap, tag in FAMILIES[fam]():
            r = model.inflate(raw, cap, defects=(defect,))
            if (r.status, r.consumed, r.output) != _oracle(oracle, raw, cap):
                by_result.append(name)
            elif tag is not None and r.tag != tag:
                by_tag.append(name)
    if defect in TAG_ONLY:
        assert by_tag and not by_result, (defect, by_result[:3])
    else:
        assert by_result, defect


# ---- the writer ---------------------------------------------------------------------------------------
def test_writer_additions_leave_old_streams_alone():
    """the round families' streams (tests/test_gpu_inflate_rounds.py) hash to what the writer gave before it learned to
    spell headers out"""
    from tests.test_gpu_inflate_rounds import FAMILIES as ROUNDS, _raw
    h = hashlib.sha256()
    for fam in sorted(ROUNDS):
        seen = set()
        for _, blocks, _, _ in ROUNDS[fam]():
            if id(blocks) not in seen:
                seen.add(id(blocks))
                h.update(_raw(blocks))
    assert h.hexdigest() == ROUNDS_SHA256


ROUNDS_SHA256 = "724e7ef8c5191b156d766ec3177b3638da675802f6458acf424ae2239446c5a8"  # taken with the writer of the commit before


def test_expand_refuses_what_it_cannot_express():
    for b in (Block("dynamic", [1], cl_lens=[4] * 13 + [5] * 6), Block("dynamic", [1], hclen=19), Block("dynamic", [1], eob=False),
              Block("dynamic", [1, Bits(1, 1)])):
        write([b])
        with pytest.raises(AssertionError):
            expand([b])
    ones = dict(lit_lens=[0, 1] + [0] * 254 + [1], dist_lens=[0])  # end-of-block is the bit 1
    assert write([Block("dynamic", [1, 1], **ones)], eob=False) == write([Block("dynamic", [1, 1], eob=False, **ones)])
    assert write([Block("dynamic", [1, 1], **ones)], eob=False) != write([Block("dynamic", [1, 1], **ones)])
    with pytest.raises(AssertionError):  # a symbol of the header without a code
        write([Block("dynamic", [], lit_lens=[0] * 256 + [1], dist_lens=[0], hlit=257, hdist=1, cl_lens=[1, 1] + [0] * 17,
                     cl_syms=[(18, 127)])])
