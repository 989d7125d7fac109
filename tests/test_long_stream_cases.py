"""The hand-built streams of tests/long_stream_cases.py, on the CPU: libz agrees with dw.expand about every one of them,
every stream has the shape its family is named for, and `predict` - the finder's and par_decode's rules restated - says
which of them the long-stream path cuts at block starts only.  This settles the piece counts tests/test_gpu_long_stream.py
asserts; nothing here has seen a GPU."""
import zlib

import pytest

from tests import deflate_writer as dw
from tests import long_stream_cases as lc
from tests.deflate_writer import Block
from tests.long_stream_cases import GROUP, JUMP_FROM, WIN, K

ALL = [(f, i) for f in lc.FAMILIES for i in range(lc.COUNTS[f])]


@pytest.fixture(params=ALL, ids=lambda p: "%s%d" % p)
def case(request):
    f, i = request.param
    return lc.family(f)[i]


def test_the_family_sizes_are_the_ones_listed():
    for f in lc.FAMILIES:
        assert len(lc.family(f)) == sum(1 for g, _ in ALL if g == f), f
    names = [c.name for c in lc.all_cases()]
    assert len(set(names)) == len(names)


def _libz(case):
    d = zlib.decompressobj(-15, zdict=case.meta["hist"]) if case.meta["hist"] else zlib.decompressobj(-15)
    out = d.decompress(case.raw)
    assert d.eof and d.unused_data == b""
    return out


def test_libz_agrees_with_expand(case):
    if case.status == dw.OK:
        assert _libz(case) == case.plain and len(case.plain) == case.meta["total"]
    else:
        assert case.status == dw.INVALID_DISTANCE and len(case.plain) < case.meta["total"]
        with pytest.raises(zlib.error):
            _libz(case)


def test_every_piece_start_is_a_block_start(case):
    """but for F's false candidates, which predict names"""
    if "false" in case.meta:
        assert case.false == [case.meta["false"]] and all(v is None for v in case.pieces.values())
        return
    assert case.false == []
    for fmt, starts in case.meta["predicted"].items():
        assert set(case.design) <= set(starts), (fmt, sorted(set(case.design) - set(starts)))


def test_the_piece_count_is_the_variant_s(case):
    """5 .. 23 pieces: the one-workgroup chain; 24 or more: pointer jumping"""
    lo, hi = (5, JUMP_FROM - 1) if case.variant == "chain" else (JUMP_FROM, 1 << 30)
    for fmt, n in case.pieces.items():
        if n is None:  # (a false candidate goes, the start behind its stored block comes)
            n = len(lc.piece_fronts(case, fmt)) - 1
        assert lo <= n <= hi, (fmt, n)
    size = len(case.raw) if case.meta["cut"] is None else case.meta["cut"]
    assert size >= (lc.CONT_MIN if case.family == "H" else lc.HIGHER_MIN)


def _sizes(case):
    f = lc.piece_fronts(case)
    return [b - a for a, b in zip(f, f[1:])]


def test_family_shapes(case):
    m, sizes = case.meta, _sizes(case)
    fronts = lc.piece_fronts(case)
    if case.family == "W":
        assert sizes.count(WIN) == 2  # the pieces that are one copy of the whole window
    if "sizes" in m:
        i = 0
        for n in m["sizes"]:  # in this order, each followed by a reader
            i = sizes.index(n, i) + 2
    if "short" in m:
        run = best = 0
        for n in sizes:
            run = run + 1 if n < 4096 else 0
            best = max(best, run)
        assert best >= m["short"] >= 14
    if "mod16" in m:
        assert {n % 16 for n in sizes if n in (32 + r if r % 2 else 4112 + r for r in m["mod16"])} == set(m["mod16"])
    if case.family == "R":
        assert [f for f in fronts[1:-1] if f < WIN] == m["front"] and m["front"][0] < 5000 and (m["bad"] == "resolve" or len(m["front"]) == 8)
        want = {None: lambda: m["total"], "resolve": lambda: m["front"][0], "tail1": lambda: m["front"][0] + 20,
                "tail2": lambda: m["front"][1] + 20, "taillast": lambda: m["front"][-1] + 20}
        assert len(case.plain) == want[m["bad"]]()
        if m["bad"] == "resolve":  # the piece goes on for more than a window behind the match: only resolve_kernel meets it
            assert sizes[1] > WIN + 3 and fronts[1] == m["front"][0]
    if case.family == "G":
        assert case.pieces["de"] == m["want"] and len(case.raw) <= 4.5 * 2**20
        assert (m["want"] > GROUP + 1) == (m["want"] >= 1025)
    if "want" in m and case.family == "F":
        for fmt, starts in m["predicted"].items():
            assert [q % 8 for q in m["want"]] == list(range(8)) and set(m["want"]) <= set(starts)
            assert m["late"] not in starts and m["late"] in dict(case.starts) and 0 < K * 8 - m["late"] % (K * 8) < 29
    if "headers" in m:
        assert len(m["headers"]) >= 4
        for name, q in m["headers"]:
            assert q % 8 and q in m["predicted"]["de"] and lc.header_parses(case.raw, q), name
    if "trailer" in m:
        assert m["trailer"] == 8 * len(case.raw) and case.raw.endswith(b"\x01" + lc.MARKER)
        assert m["trailer"] in m["predicted"]["zl"] and m["trailer"] in m["predicted"]["gz"] and m["trailer"] not in m["predicted"]["de"]
    if case.family == "X":
        bits = [q for q in m["predicted"]["de"] if q <= m["final"]] + [8 * len(case.raw)]
        grow = [n for n, a, b in zip(sizes, bits, bits[1:]) if n > 6 * ((b + 7) // 8 - a // 8) + 65536]
        assert len(grow) == 1 and (grow[0] > 4000000) == ("1032" in case.name)
    if "residue" in m:
        assert len(case.plain) % 65536 == m["residue"] and len(case.plain) > 2 * 65536
    if "ff" in m:
        assert case.plain == b"\xff" * len(case.plain)
    if "length" in m:
        assert len(case.plain) == m["length"]
    if case.family == "H" and m["cut"] is not None:
        assert 8 * m["cut"] not in dict(case.starts) and max(b for b, _ in case.starts if b < 8 * m["cut"]) in m["predicted"]["de"]


def test_the_families_hold_what_the_issue_lists():
    c = {x.name: x for x in lc.family("C")}
    assert {x.meta["residue"] for x in c.values() if x.name.startswith("C zlib")} == set(lc.ADLER_RES)
    assert {x.meta["length"] for x in c.values() if "gzip" in x.name} == {2**20 - 1, 2**20, 2**20 + 1, 2 * 2**20 + 17}
    h = lc.family("H")
    assert {len(x.meta["hist"]) for x in h} >= {1, WIN - 1, WIN} and {x.status for x in h} == {dw.OK, dw.INVALID_DISTANCE}
    assert sorted(x.meta["want"] for x in lc.family("G")) == [1023, 1024, 1025, 1026, 1100]


def test_stored_blocks_written_directly_are_the_writer_s():
    data = bytes(range(200)) * 3
    assert lc.stored_unit(data).raw == dw.write([Block("stored", data, last=False)])
    assert lc.stored_unit(b"", last=True).raw == dw.write([Block("stored", b"", last=True)])
    st = []
    raw = dw.write([Block("fixed", [1, 200], last=False), Block("stored", b"ab", last=False), Block("dynamic", [5, 5, (3, 1)])], starts=st)
    assert st == [0, 3 + 8 + 9 + 7, 8 * (4 + 4 + 2)] and zlib.decompress(raw, -15) == b"\x01\xc8ab" + b"\x05" * 5


def test_predict_by_hand():
    """chunks of 64 bytes.  A stored block of 70 bytes at the stream's start: the host follows it, the block behind it
    (bit 600) is a seed.  Then three units `fixed block, empty stored block` of 8 bytes (4a 4a 06 00 00 00 ff ff) at bytes
    75, 83 and - behind 35 bytes of stored ff - 126: their markers end at bytes 83 and 91, both in chunk 1 (the first one
    counts), and 134 in chunk 2.  The final block is 03 00: behind bit 1072 the body has 16 bits left, a candidate needs 29 -
    with a four-byte trailer behind the stream it is one.  ff bytes hold no header (BTYPE 3 at every bit)."""
    ff = lambda n: lc.stored_unit(b"\xff" * n).raw
    unit = lc.Unit([Block("fixed", [98, 99], last=False)]).raw
    assert unit == bytes.fromhex("4a4a06000000ffff")
    body = ff(70) + unit + unit + ff(30) + unit + bytes.fromhex("0300")
    assert zlib.decompress(body, -15) == b"\xff" * 70 + b"bcbc" + b"\xff" * 30 + b"bc" and len(body) == 136
    assert lc.predict(body, k=64) == [0, 600, 664]
    assert lc.predict(body + b"\x00\x00\x00\x01", k=64) == [0, 600, 664, 1072]
    assert lc.judge([0, 600, 664, 1072], [(0, 0), (600, 70), (664, 72), (728, 74), (1072, 106)], 1072) == (4, [])
    assert lc.judge([0, 600, 660], [(0, 0), (600, 70), (664, 72)], 1072) == (None, [660])
    # a dynamic header is a candidate where it stands, whatever the bit: one byte into chunk 2, behind a fixed block
    dyn = lc.Unit([Block("fixed", [200, 65], last=False), Block("dynamic", [1, 2, 3, (3, 1)], last=False)])
    body = ff(120) + dyn.raw + bytes.fromhex("0300")
    q = 8 * 125 + dyn.starts[1]
    assert q % 8 == 3 + 9 + 8 + 7 - 24 and lc.header_parses(body, q) and not lc.header_parses(body, q + 1)
    assert lc.predict(body, k=64) == [0, 1000, q]
