"""GZip files of many members on the GPU (md_gz_members_*, md_bgzf_compress; csrc/gz_members.hip).  Needs an
MI355X: `pytest -m gpu`.  Yardsticks: Python's gzip.decompress and zlib with wbits 31 (libz's reading of RFC 1952,
tests/gz_members_util.libz_members) for validity and output bytes, oracle.gz_deflate for the bytes the writer's members
hold - never the code under test.

The writer's rule for the stored form: the issue that asked for this gave two conditions that cannot both hold - a
member's body is the oracle's unless that member would pass 65 536 bytes, AND written <= md_bgzf_compress_bound with 31
bytes per block.  The oracle's body for 4 096 random bytes is about 4 250 bytes at levels 1-9 (and 4 106 at level 0), more than
the 4 101 of the stored form, so a file of such blocks passes the bound.  The bound is what callers size buffers by, so it
holds, and the rule tested here is: the oracle's body, or - only where that body is longer than 5 + the block's bytes,
which covers every member that would pass 65 536 - the stored form."""
import gzip
import random
import struct
import zlib

import pytest

from tests import gz_members_util as gu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gz():
    from decompress_amd import gz
    gz.Members.scan(b"")  # (creates the engine)
    return gz


@pytest.fixture(scope="module")
def corpus():
    from decompress_amd import workloads
    return workloads.corpus()


def _text(n, seed=1):
    from decompress_amd import workloads
    return workloads.text(seed, n)


def _rand(n, seed=1):
    return random.Random(seed).randbytes(n)


def _check_indexed(gz, f, idx, plain, members=None):
    assert gzip.decompress(f) == plain
    r = gz.Members.uncompress(f, len(plain))
    assert r[0] == "Ok", r[:2]
    assert r[2] == plain
    assert r[1] == {"members": len(idx) if members is None else members, "consumed": len(f), "written": len(plain), "indexed": 1}
    s = gz.Members.scan(f)
    assert s is not None and s["members"] == len(idx) and s["size"] == len(plain)
    assert list(zip(s["c_off"], s["u_off"])) == idx
    assert gz.Members.uncompress(f)[2] == plain  # (room from the scan)


# ---- 1. reader, indexed ----
def test_indexed_member_counts(gz):
    for n, block in ((1, 0xff00), (0xff00, 0xff00), (0xff00 + 1, 0xff00), (999 * 700, 700)):
        for eof in (True, False):
            plain = _text(n, seed=n)
            f, idx = gu.bgzf_file(plain, block=block, eof=eof)
            _check_indexed(gz, f, idx, plain)
    assert len(gu.bgzf_file(_text(999 * 700), block=700)[1]) == 1000


def test_indexed_shapes(gz):
    plain = _text(300000, seed=3)
    f, idx = gu.bgzf_of_members([b"ab", b"", b"", plain[:70000 - 5000], b"", b"cd"])
    _check_indexed(gz, f, idx, b"ab" + plain[:65000] + b"cd")
    # BC behind another subfield, XLEN > 6
    f, idx = gu.bgzf_file(plain, block=30000, before=gu.subfield(b"XY", b"12345"), after=gu.subfield(b"ZZ", b"\x1f\x8b\x08\x04"))
    _check_indexed(gz, f, idx, plain)
    # FNAME / FCOMMENT / FHCRC beside the size field
    f, idx = gu.bgzf_file(plain, block=50000, name=b"file.txt", comment=b"a comment", hcrc=True)
    _check_indexed(gz, f, idx, plain)
    # NUL padding behind the end, with and without the EOF marker
    for eof in (True, False):
        f, idx = gu.bgzf_file(plain, eof=eof)
        for pad in (1, 7, 70000):
            assert gzip.decompress(f + b"\0" * pad) == plain
            r = gz.Members.uncompress(f + b"\0" * pad, len(plain))
            assert r[0] == "Ok" and r[2] == plain and r[1]["indexed"] == 1 and r[1]["consumed"] == len(f) + pad and r[1]["members"] == len(idx)
    # blocks of one byte
    f, idx = gu.bgzf_file(plain[:3000], block=1)
    _check_indexed(gz, f, idx, plain[:3000])
    # nothing but the EOF marker; nothing at all
    _check_indexed(gz, gu.EOF_MARKER, [(0, 0)], b"")
    assert gz.Members.uncompress(b"", 0) == ("Ok", {"members": 0, "consumed": 0, "written": 0, "indexed": 0}, b"")
    assert gz.Members.scan(b"") is None


def test_indexed_corpus(gz, corpus):
    plain = b"".join(corpus.values())
    assert len(corpus) == 15
    f, idx = gu.bgzf_file(plain)
    _check_indexed(gz, f, idx, plain)
    # random bytes: members near the size limit (libz's level 6 stores what does not compress)
    plain = _rand(5 * 0xff00 + 17)
    f, idx = gu.bgzf_file(plain)
    _check_indexed(gz, f, idx, plain)


# ---- 2. reader, general ----
def test_general_path(gz):
    parts = [_text(n, seed=n) for n in (100, 0, 70000, 1, 300000)]
    plain = b"".join(parts)
    cases = [b"".join(gzip.compress(p, mtime=0) for p in parts),
             b"".join(gu.bgzf_member(p[:60000]) if k % 2 else gu.member(p[:60000]) for k, p in enumerate(parts)),
             b"".join(gu.member(p, hcrc=True, name=b"n%d" % k, extra=gu.subfield(b"AB", b"x" * k)) for k, p in enumerate(parts)),
             gzip.compress(parts[0], mtime=0) + b"\0" * 9 + gzip.compress(parts[2], mtime=0) + b"\0" * 3]
    for f in cases:
        want = gzip.decompress(f)
        assert gu.libz_members(f)[:2] == ("ok", want)
        r = gz.Members.uncompress(f, len(want))
        assert r[0] == "Ok" and r[2] == want, r[:2]
        assert r[1]["indexed"] == 0 and r[1]["consumed"] == len(f) and r[1]["written"] == len(want)
        assert gz.Members.scan(f) is None
        assert gz.Members.uncompress(f)[2] == want  # (room grown until it fits)
    assert gz.Members.uncompress(cases[0], len(plain))[1]["members"] == 5


def test_general_long_member_among_small(gz):
    big = _text(8 << 20, seed=8)
    f = gzip.compress(b"head", mtime=0) + gzip.compress(big, 6, mtime=0) + gu.bgzf_member(b"tail")
    r = gz.Members.uncompress(f, len(big) + 8)
    assert r[0] == "Ok" and r[2] == b"head" + big + b"tail" and r[1]["indexed"] == 0 and r[1]["members"] == 3


# ---- 3. false candidates ----
def test_planted_magic_changes_nothing(gz):
    plain = _text(100000, seed=4)
    fake = gu.bgzf_member(b"not a member")  # a whole valid indexed member, as payload
    stored = b"\x01" + struct.pack("<HH", len(fake), len(fake) ^ 0xffff) + fake
    parts = [gu.bgzf_member(plain[:50000]), gu.bgzf_member(fake, body=stored),
             gu.bgzf_member(plain[50000:], before=gu.subfield(b"FK", fake)), gu.EOF_MARKER]
    f = b"".join(parts)
    want = plain[:50000] + fake + plain[50000:]
    assert gzip.decompress(f) == want
    r = gz.Members.uncompress(f, len(want))
    assert r[0] == "Ok" and r[2] == want and r[1] == {"members": 4, "consumed": len(f), "written": len(want), "indexed": 1}
    s = gz.Members.scan(f)
    assert s["c_off"] == [0, len(parts[0]), len(parts[0]) + len(parts[1]), len(f) - 28]


# ---- 4. failures ----
def _fails(gz, f, cap, status=None, python_too=True):
    """libz refuses f (and Python's gzip, which however ignores the reserved flag bits and FHCRC); so do we, at the same
    member, with the bytes of the members in front of it"""
    z = gu.libz_members(f)
    assert z[0] == "error", "the yardstick accepts this file"
    if python_too:
        with pytest.raises((OSError, EOFError, zlib.error)):
            gzip.decompress(f)
    r = gz.Members.uncompress(f, cap)
    assert r[0] == "Error", r[:2]
    if status is not None:
        assert r[1] == status, r[1]
    assert r[2]["members"] == z[2] and r[2]["consumed"] == z[3] and r[2]["written"] == len(z[1]) and r[3] == z[1]
    return r


def _patched(f, at, fn):
    b = bytearray(f)
    b[at] = fn(b[at])
    return bytes(b)


def test_failures(gz):
    plain = _text(200000, seed=6)
    for make in (lambda: gu.bgzf_file(plain, block=40000), lambda: (b"".join(gu.member(plain[k:k + 40000]) for k in range(0, 200000, 40000)), None)):
        f = make()[0]
        offs = [m for m in range(len(f) - 3) if f[m:m + 3] == b"\x1f\x8b\x08" and (m == 0 or gu.libz_members(f[:m])[0] == "ok")]
        m2, m3 = offs[2], offs[3]
        flip = lambda v: v ^ 0x10
        _fails(gz, _patched(f, m3 - 8, flip), len(plain), "Invalid_checksum")                  # CRC-32
        _fails(gz, _patched(f, m3 - 4, lambda v: (v + 1) & 255), len(plain), "Invalid input size")   # ISIZE up
        _fails(gz, _patched(f, m3 - 4, lambda v: (v - 1) & 255), len(plain), "Invalid input size")   # ISIZE down
        _fails(gz, _patched(f, m2 + 2, lambda v: 7), len(plain), "Invalid GZip header")         # CM 7
        _fails(gz, _patched(f, m2 + 3, lambda v: v | 0x20), len(plain), "Invalid GZip header", python_too=False)  # a reserved flag bit
        hdr = 18 if f[m2 + 3] & 4 else 10
        for cut in (m2 + 5, m2 + hdr + 100, m3 - 3):  # inside header / body / trailer
            _fails(gz, f[:cut], len(plain), "Unexpected_end_of_input")
        _fails(gz, f + b"garbage", len(plain), "Invalid GZip header")
        _fails(gz, f + b"\0\0\0garbage", len(plain), "Invalid GZip header")
    # FHCRC, with and without a size field
    for f in (gu.bgzf_file(plain, block=40000, hcrc=True)[0], b"".join(gu.member(plain[k:k + 40000], hcrc=True, name=b"x") for k in range(0, 200000, 40000))):
        d = zlib.decompressobj(31)
        d.decompress(f)
        m1 = len(f) - len(d.unused_data)  # the second member; its FHCRC sits behind the fixed bytes, the extra field and "x\0"
        at = m1 + (18 if f[m1 + 3] & 4 else 10) + (2 if f[m1 + 3] & 8 else 0)
        z = gu.libz_members(_patched(f, at, lambda v: v ^ 1))
        assert z[0] == "error" and z[2] == 1 and z[3] == m1
        r = gz.Members.uncompress(_patched(f, at, lambda v: v ^ 1), len(plain))
        assert r[:2] == ("Error", "Invalid GZip header checksum") and r[2]["consumed"] == m1 and r[2]["members"] == 1 and r[3] == z[1]


def test_bsize_wrong_falls_to_general_path(gz):
    plain = _text(150000, seed=7)
    f, idx = gu.bgzf_file(plain, block=50000)
    m1 = idx[1][0]
    for delta in (-1, 1, 3000):
        bs = struct.unpack_from("<H", f, m1 + 16)[0] + delta
        g = f[:m1 + 16] + struct.pack("<H", bs) + f[m1 + 18:]
        assert gzip.decompress(g) == plain  # (the size field means nothing to libz)
        r = gz.Members.uncompress(g, len(plain))
        assert r[0] == "Ok" and r[2] == plain and r[1]["indexed"] == 0 and r[1]["members"] == 4
        assert gz.Members.scan(g) is None
    # the last member's BSIZE past the end of the file
    last = idx[-2][0]
    g = f[:last + 16] + b"\xff\xff" + f[last + 18:]
    assert gzip.decompress(g) == plain
    r = gz.Members.uncompress(g, len(plain))
    assert r[0] == "Ok" and r[2] == plain and r[1]["indexed"] == 0


def test_room_one_short(gz):
    plain = _text(150000, seed=8)
    f, idx = gu.bgzf_file(plain, block=50000)
    r = gz.Members.uncompress(f, len(plain) - 1)
    assert r[:2] == ("Error", "Unexpected_end_of_output") and r[2]["written"] == len(plain) and r[2]["indexed"] == 1
    g = b"".join(gu.member(plain[k:k + 50000]) for k in range(0, 150000, 50000))
    r = gz.Members.uncompress(g, len(plain) - 1)
    assert r[:2] == ("Error", "Unexpected_end_of_output") and r[2]["members"] == 2 and r[2]["written"] == 100000 and r[3] == plain[:100000]


# ---- 5. writer ----
def _check_written(gz, oracle, src, level, block, expect_stored=None):
    from decompress_amd import _lib
    out = gz.Bgzf.compress(src, level=level, block=block)
    assert gzip.decompress(out) == src
    assert out[-28:] == gu.EOF_MARKER
    offs, end = gu.walk_bsize(out)
    assert end == len(out) and offs[-1] == len(out) - 28 and len(offs) == -(-len(src) // block) + 1
    assert len(out) <= _lib.load().md_bgzf_compress_bound(len(src), block)
    stored = 0
    for k, a in enumerate(offs[:-1]):
        b = offs[k + 1]
        blk = src[k * block:(k + 1) * block]
        assert b - a <= 65536
        assert out[a:a + 16] == bytes.fromhex("1f8b08040000000000ff060042430200")
        assert out[b - 8:b] == struct.pack("<II", zlib.crc32(blk), len(blk))
        want = oracle.gz_deflate(blk, level=level)[10:-8]
        if len(want) > 5 + len(blk):  # (see the module's docstring; 26 + len(want) > 65 536 implies this)
            want = b"\x01" + struct.pack("<HH", len(blk), len(blk) ^ 0xffff) + blk
            stored += 1
        assert out[a + 18:b - 8] == want, (k, level, block)
    if expect_stored is not None:
        assert (stored > 0) == expect_stored
    return out


def test_writer(gz, oracle, corpus):
    big = (1 << 20) + 3
    names = sorted(corpus)
    for block in (0xff00, 4096):
        for level in (0, 1, 4, 6, 9):
            for n in (0, 1, block - 1, block, block + 1):
                _check_written(gz, oracle, _text(n, seed=n + level), level, block)
                _check_written(gz, oracle, _rand(n, seed=n + level), level, block)
            _check_written(gz, oracle, bytes(3 * block + 5), level, block, expect_stored=level == 0)  # (level 0: several stored blocks, 5 bytes each)
        for level, src in ((6, _text(big)), (1, _rand(big)), (4, corpus[names[0]][:big]), (9, corpus[names[-1]][:300000]), (0, _text(200000))):
            _check_written(gz, oracle, src, level, block)
    # 0xff00 random bytes: the reference's body would make a member of 65 898 bytes - the stored form is taken
    for level in (1, 6, 9):
        src = _rand(0xff00 * 2, seed=level)
        assert len(oracle.gz_deflate(src[:0xff00], level=level)) + 8 > 65536
        out = _check_written(gz, oracle, src, level, 0xff00, expect_stored=True)
        assert len(out) == 2 * (26 + 5 + 0xff00) + 28
    src = _text(300000, seed=11)
    assert gz.Bgzf.compress(src, level=6) == gz.Bgzf.compress(src, level=6)
    assert gz.Bgzf.compress(src, level=6) == gz.Bgzf.compress(src, level=6, block=0)
    from decompress_amd import engine
    out = gz.Bgzf.compress(src, level=6)
    assert gz.Bgzf.compress(src, level=6, dst_len=len(out)) == out
    with pytest.raises(engine.Error, match="Unexpected_end_of_output"):
        gz.Bgzf.compress(src, level=6, dst_len=len(out) - 1)
    with pytest.raises(engine.Error):
        gz.Bgzf.compress(src, level=6, block=0xff01)
    with pytest.raises(engine.Error):
        gz.Bgzf.compress(src, level=10)
    for corpus_file in names:
        assert gzip.decompress(gz.Bgzf.compress(corpus[corpus_file], level=4)) == corpus[corpus_file]


# ---- 6. round trip at size ----
def test_round_trip_64_mib(gz, corpus):
    cat = b"".join(corpus.values())
    src = (cat * ((64 << 20) // len(cat) + 1))[:64 << 20]
    f = gz.Bgzf.compress(src, level=6)
    r = gz.Members.uncompress(f, len(src))
    assert r[0] == "Ok" and r[1] == {"members": -(-len(src) // 0xff00) + 1, "consumed": len(f), "written": len(src), "indexed": 1}
    assert r[2] == src
    assert gzip.decompress(f) == src


# ---- 7. seeded fuzz ----
def test_fuzz_200_files(gz):
    rng = random.Random(0xb62f)
    damaged = agree_ok = agree_bad = 0
    for case in range(200):
        kind = rng.choice(("bgzf", "bgzf", "plain", "mixed"))
        parts, plain = [], []
        for _ in range(rng.randint(1, 12)):
            n = rng.choice((0, 1, 2, rng.randint(3, 300), rng.randint(300, 40000)))
            p = _text(n, seed=rng.getrandbits(20)) if rng.random() < 0.7 else rng.randbytes(n)
            opts = {}
            if rng.random() < 0.2:
                opts["name"] = b"n" * rng.randint(0, 20)
            if rng.random() < 0.2:
                opts["comment"] = b"c" * rng.randint(0, 20)
            if rng.random() < 0.3:
                opts["hcrc"] = True
            lvl = rng.choice((0, 1, 6, 9))
            if kind == "bgzf" or (kind == "mixed" and rng.random() < 0.5):
                before = gu.subfield(b"AA", rng.randbytes(rng.randint(0, 9))) if rng.random() < 0.3 else b""
                parts.append(gu.bgzf_member(p, lvl, before=before, **opts))
            else:
                extra = gu.subfield(b"QQ", rng.randbytes(rng.randint(0, 9))) if rng.random() < 0.3 else None
                parts.append(gu.member(p, lvl, extra=extra, **opts))
            plain.append(p)
        if rng.random() < 0.5:
            parts.append(gu.EOF_MARKER)
        f = b"".join(parts) + b"\0" * rng.choice((0, 0, 0, 5))
        if case % 3 == 0:
            at = rng.randrange(len(f))
            f = _patched(f, at, lambda v: v ^ (1 << rng.randrange(8)))
            damaged += 1
        z = gu.libz_members(f)
        r = gz.Members.uncompress(f, sum(map(len, plain)) + 64)
        if z[0] == "ok":
            assert r[0] == "Ok" and r[2] == z[1], (case, r[:2])
            assert r[1]["consumed"] == len(f) and r[1]["members"] == z[2]
            if case % 3:
                assert gzip.decompress(f) == z[1] and r[1]["indexed"] == (1 if kind == "bgzf" else r[1]["indexed"])
            agree_ok += 1
        else:
            assert r[0] == "Error", (case, r[:2])
            assert r[2]["members"] == z[2] and r[2]["consumed"] == z[3] and r[3] == z[1], case
            agree_bad += 1
    assert damaged == 67 and agree_ok + agree_bad == 200 and agree_bad >= 20
