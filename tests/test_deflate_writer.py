"""The test-side deflate writer (tests/deflate_writer.py) against three decoders: zlib, the token reader
(tests/deflate_tokens.py) and the CPU oracle.  The GPU round tests build their streams with it, so it must be right."""
import random
import zlib

import pytest

from tests import deflate_tokens
from tests.deflate_writer import (END_OF_OUTPUT, INVALID_DISTANCE, INVALID_DISTANCE_CODE, OK, Block, expand,
                                  limited_lengths, match, write)


def _random_tokens(rng, n, have=0, maxlen=258, maxdist=32768, lit_alphabet=256):
    toks = []
    for _ in range(n):
        if have >= 3 and rng.random() < 0.5:
            ln = rng.choice([3, 4, 5, 10, 17, 31, 32, 33, 100, 257, 258, rng.randrange(3, 259)])
            ln = min(ln, maxlen)
            d = rng.randrange(1, min(have, maxdist) + 1)
            toks.append((ln, d))
            have += ln
        else:
            toks.append(rng.randrange(lit_alphabet))
            have += 1
    return toks, have


def _random_blocks(rng, nblocks):
    blocks, have = [], 0
    for _ in range(nblocks):
        kind = rng.choice(["stored", "fixed", "dynamic", "dynamic"])
        n = rng.choice([0, 1, 2, 50, 400, 3000])
        if kind == "stored":
            toks = [rng.randrange(256) for _ in range(n)]
            have += n
        else:
            toks, have = _random_tokens(rng, n, have)
        blocks.append(Block(kind, toks))
    return blocks


def _tok_view(blocks):
    """what deflate_tokens.tokens reports for `blocks`: literals and (length, distance) matches, block kinds"""
    out, op = [], 0
    for b in blocks:
        out.append(("B", {"stored": 0, "fixed": 1, "dynamic": 2}[b.kind], op))
        for t in b.tokens:
            if isinstance(t, int):
                out.append((op, "L", t))
                op += 1
            else:
                out.append((op, "M", t[0], t[1]))
                op += t[0]
    return out


def _check_valid(oracle, blocks):
    raw = write(blocks)
    st, want = expand(blocks)
    assert st == OK
    d = zlib.decompressobj(-15)
    assert d.decompress(raw) + d.flush() == want and d.eof and d.unused_data == b""
    assert deflate_tokens.tokens(raw) == _tok_view(blocks)
    ost, oused, oout = oracle.de_inflate(raw, len(want))
    assert (ost, oused, oout) == (0, len(raw), want)
    return raw, want


@pytest.mark.parametrize("seed", range(12))
def test_random_blocks(oracle, seed):
    rng = random.Random(seed)
    _check_valid(oracle, _random_blocks(rng, rng.randrange(1, 7)))


def test_empty_and_stored_blocks(oracle):
    _check_valid(oracle, [Block("stored", [])])
    _check_valid(oracle, [Block("fixed", [])])
    _check_valid(oracle, [Block("dynamic", [])])
    _check_valid(oracle, [Block("stored", []), Block("dynamic", [1, 2, 3, (3, 3)]), Block("stored", [])])
    _check_valid(oracle, [Block("stored", list(range(256)) * 255 + list(range(255)))])  # 65535 bytes
    _check_valid(oracle, [Block("fixed", [7]), Block("dynamic", [(258, 1)] * 300), Block("fixed", [(3, 32768 - 1000)])])


def test_fifteen_bit_codes(oracle):
    """Tie-free symbol counts (1, 2, 4, 7, 12, ..: each the two before it and one more) make the unlimited Huffman code
    deeper than 15 bits: the lengths are limited.  (Plain Fibonacci counts do not: their ties are broken towards the
    shallow subtree and 20 of them come out 11-12 bits deep.)"""
    from tests import huffman_tree_model
    rng = random.Random(5)
    counts = [1, 2]
    while len(counts) < 17:
        counts.append(counts[-1] + counts[-2] + 1)
    toks = []
    for i, f in enumerate(counts):  # (with end-of-block's 1: an unlimited code 17 bits deep)
        toks += [i + 65] * f
    rng.shuffle(toks)
    assert huffman_tree_model.plain_depth([toks.count(i) for i in range(256)] + [1]) > 15
    b = Block("dynamic", toks)
    lens = limited_lengths([toks.count(i) for i in range(256)] + [1], 15)
    assert max(lens) == 15
    _check_valid(oracle, [b])
    # explicit lengths: symbol i has i + 1 bits (1..14), symbol 14 and end-of-block 15 bits: a complete code
    lit = [0] * 288
    for i in range(14):
        lit[i] = i + 1
    lit[14] = lit[256] = 15
    toks = [rng.randrange(15) for _ in range(2000)]
    _check_valid(oracle, [Block("dynamic", toks, lit_lens=lit)])


def test_single_distance_code(oracle):
    """one distance code of one bit (an incomplete distance code: RFC 1951 allows it), used and unused"""
    toks = [1, 2, 3, 4] + [(4, 4)] * 50
    dist = [0] * 30
    dist[3] = 1
    _check_valid(oracle, [Block("dynamic", toks, dist_lens=dist)])
    _check_valid(oracle, [Block("dynamic", [5] * 40, dist_lens=[1])])


def test_length_258_both_ways_and_wide_headers(oracle):
    toks = [9] + [match(258, 1, lsym=284)] * 5 + [(258, 1)] * 5 + [match(258, 1, lsym=284, lext=31)]
    blocks = [Block("dynamic", toks), Block("fixed", toks[1:]), Block("dynamic", toks[1:], hlit=286, hdist=30)]
    raw, want = _check_valid(oracle, blocks)
    assert want == bytes([9]) * (1 + 258 * 33)
    assert raw != write([Block("dynamic", [9] + [(258, 1)] * 11), Block("fixed", [(258, 1)] * 11),
                         Block("dynamic", [(258, 1)] * 11, hlit=286, hdist=30)])
    # HLIT = 288 and HDIST = 32 (zlib refuses more than 286 / 30 lengths; the oracle and the kernel take them)
    wide = [Block("dynamic", toks, hlit=288, hdist=32)]
    assert _check_invalid(oracle, wide) == OK
    assert deflate_tokens.tokens(write(wide)) == _tok_view(wide)


def _check_invalid(oracle, blocks, cap=1 << 20):
    raw = write(blocks)
    st, want = expand(blocks, cap)
    ost, oused, oout = oracle.de_inflate(raw, cap)
    assert (ost, oout) == (st, want), (ost, st)
    assert oused == (len(raw) if st == OK else 0)
    return st


def test_invalid_symbols_and_their_status(oracle):
    """The symbols RFC 1951 reserves, given codes: distance codes 30 / 31 stop the stream with Invalid_distance_code
    in front of the token (fixed blocks code them; dynamic blocks with HDIST = 32); the lengths 286 / 287 are NOT
    errors for this decoder family - they decode as length 3 without extra bits (lib/de.ml's table), what the oracle
    and the kernel both do, so the stream is valid for them (zlib rejects it)."""
    pre = list(range(40))
    for kind in ("fixed", "dynamic"):
        for ds in (30, 31):
            b = Block(kind, pre + [match(5, 1, dsym=ds)] + [1, 2], extra=(1000 + ds,), hdist=32 if kind == "dynamic" else None)
            assert _check_invalid(oracle, [b]) == INVALID_DISTANCE_CODE
        for ls in (286, 287):
            b = Block(kind, pre + [match(3, 7, lsym=ls), (10, 20)], extra=(ls,), hlit=288 if kind == "dynamic" else None)
            assert _check_invalid(oracle, [b]) == OK
            with pytest.raises(zlib.error):
                zlib.decompress(write([b]), -15)
    # distances beyond what is written, and the output cap in front of a literal / inside a match
    assert _check_invalid(oracle, [Block("dynamic", pre + [(3, 41)])]) == INVALID_DISTANCE
    assert _check_invalid(oracle, [Block("dynamic", pre + [(3, 40)])]) == OK
    assert _check_invalid(oracle, [Block("dynamic", pre + [(20, 40)])], cap=59) == END_OF_OUTPUT
    assert _check_invalid(oracle, [Block("dynamic", pre + [(20, 40)])], cap=60) == OK
    assert _check_invalid(oracle, [Block("stored", pre), Block("fixed", [1])], cap=40) == END_OF_OUTPUT
    assert _check_invalid(oracle, [Block("stored", pre)], cap=39) == END_OF_OUTPUT
