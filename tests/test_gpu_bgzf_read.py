"""Random access to blocked GZip on the GPU (md_bgzf_index_*, md_bgzf_read*; csrc/capi_bgzf_read.cpp, bgzf_read.hip, DESIGN
4f).  Needs an MI355X: `pytest -m gpu`.  The witness is Python slicing of the plaintext; the files come from
tests/gz_members_util (zlib and struct alone), never from the code under test; the statuses of damaged members are compared
with what md_gz_members_uncompress says of the same file."""
import ctypes
import random
import struct
import zlib

import numpy as np
import pytest

from tests import gz_members_util as gu

pytestmark = pytest.mark.gpu
OK, INVALID_ARGUMENT, INVALID_INDEX = 0, -1, 21
BAD_INDEX, BAD_CRC, BAD_SIZE = "Invalid index", "Invalid_checksum", "Invalid input size"


@pytest.fixture(scope="module")
def eng():
    from decompress_amd import engine
    return engine.default_engine(0)


def _gz():
    from decompress_amd import gz
    return gz


def _text(n, seed):
    rng = random.Random(seed)
    words = [b"alpha", b"beta", b"gamma", b"delta", b"chr1", b"chr22", b"ACGT", b"TTGACA", b"0/1", b"PASS", b"."]
    out, size = [], 0
    while size < n:
        line = b"\t".join(rng.choice(words) if rng.random() < 0.7 else b"%d" % rng.randrange(10 ** 7) for _ in range(9)) + b"\n"
        out.append(line)
        size += len(line)
    return b"".join(out)[:n]


def gzi(pairs):
    return struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", c, u) for c, u in pairs)


_FILES = {}


def _file(block):
    """(file, table of M + 1 pairs, plaintext, index loaded from the util's own table) - made once"""
    if block not in _FILES:
        plain = _text({0xff00: 200000, 4096: 200000, 300: 40000}[block], block)
        f, idx = gu.bgzf_file(plain, block=block)
        _FILES[block] = (f, idx + [(len(f), len(plain))], plain, _gz().BgzfIndex.from_gzi(gzi(idx[1:]), f))
    return _FILES[block]


def _check(idx, src, plain, ranges):
    got = idx.read_many(src, ranges)
    assert len(got) == len(ranges)
    for (off, n), (st, data) in zip(ranges, got):
        assert st == "Ok" and data == plain[off:off + n], (off, n, st)


def _raw_read(eng, idx, src, where, lens, dst_offs, room, virtual=False):
    """the C call as it is -> (return value, statuses, the room bytes of dst: 0xa5 where nothing was written)"""
    n = len(where)
    a = lambda v: np.array(v if n else [0], dtype=np.uint64)
    off, ln, dof = a(where), a(lens), a(dst_offs)
    dst = np.full(max(room, 1), 0xa5, dtype=np.uint8)
    status = np.full(max(n, 1), 77, dtype=np.int32)
    fn = eng.lib.md_bgzf_read_virtual if virtual else eng.lib.md_bgzf_read
    rc = fn(eng.ctx, idx._h, src, len(src), n, off.ctypes.data, ln.ctypes.data, dst.ctypes.data, dof.ctypes.data, status.ctypes.data)
    return rc, [int(s) for s in status[:n]], dst


@pytest.mark.parametrize("block", [0xff00, 4096, 300])
def test_positions(eng, block):
    f, tab, plain, idx = _file(block)
    size, M = len(plain), len(tab) - 1
    assert idx.info() == {"src_len": len(f), "members": M, "size": size} and idx.entries() == tab
    edges = [u for _, u in tab[1:-2]]  # the edges between members with bytes
    e1, e2 = edges[0], edges[len(edges) // 2]
    ranges = [(5, 40), (e2 + 7, block - 20),           # inside one member
              (e1 - 30, 30), (e1 - 30, 31), (0, e1), (0, e1 + 1),  # ending exactly on and one byte past an edge
              (e1, 10), (e2, block), (e2, block + 1),  # starting on an edge
              (e1 - 1, 2), (e2 - 100, 200),            # crossing 2
              (e1 - 5, min(block + 10, size - e1 + 5)),  # crossing 3 where there are 3
              (0, size), (1, size - 2),                # all members
              (size, 0), (0, 0), (e1, 0), (77, 0),     # zero-length ranges
              (size - 1, 1), (size - 1, 0), (size - 300, 300)]  # the last byte
    _check(idx, f, plain, ranges)
    stats = idx.last_stats()
    assert stats["members"] == M - 1 and stats["launches"] == 1 and stats["bytes_in"] == tab[M - 1][0]
    assert idx.read(f, 0, size) == plain
    assert idx.read(f, size, 0) == b"" and idx.last_stats() == {"members": 0, "launches": 0, "bytes_in": 0, "bytes_scratch": 0}
    # a range behind the end is the call's error, whatever else is asked
    rc, _, dst = _raw_read(eng, idx, f, [0, size - 1], [10, 2], [0, 16], 32)
    assert rc == INVALID_ARGUMENT and bytes(dst) == b"\xa5" * 32
    assert _raw_read(eng, idx, f, [size + 1], [0], [0], 1)[0] == INVALID_ARGUMENT
    assert _raw_read(eng, idx, f, [], [], [], 1)[0] == OK


def test_empty_members_are_never_decoded(eng):
    a, b, c = _text(5000, 1), _text(300, 2), _text(70000, 3)[:0x10000]
    chunks = [b"", a, b"", b"", b, c, b"", b"x", b""]
    f, idx = gu.bgzf_of_members(chunks)
    plain = b"".join(chunks)
    tab = idx + [(len(f), len(plain))]
    built = _gz().BgzfIndex.build(f)
    loaded = _gz().BgzfIndex.from_gzi(gzi(idx[1:]), f)
    assert built.entries() == loaded.entries() == tab
    with_bytes = [k for k, ch in enumerate(chunks) if ch]
    for x in (built, loaded):
        _check(x, f, plain, [(0, len(plain))])
        assert x.last_stats()["members"] == len(with_bytes) == 4
        assert x.last_stats()["bytes_in"] == sum(tab[k + 1][0] - tab[k][0] for k in with_bytes)
        # across the empty members between a and b; the byte behind the last empty ones
        _check(x, f, plain, [(4990, 20), (5000, 1), (4999, 1), (len(plain) - 1, 1), (5299, 3), (len(plain), 0)])
        _check(x, f, plain, [(4999, 2)])
        assert x.last_stats()["members"] == 2
    # a file of the EOF marker alone, and an empty file
    for src in (gu.EOF_MARKER, b""):
        x = _gz().BgzfIndex.build(src)
        assert x.info() == {"src_len": len(src), "members": len(src) // 28, "size": 0}
        assert x.read_many(src, [(0, 0)]) == [("Ok", b"")]


def test_many_ranges_one_member_and_bytes_in(eng):
    f, tab, plain, idx = _file(4096)
    length = lambda k: tab[k + 1][0] - tab[k][0]
    rng = random.Random(5)
    u = tab[5][1]
    ranges = [(u + rng.randrange(4000), rng.randrange(1, 96)) for _ in range(64)]
    _check(idx, f, plain, ranges)
    assert idx.last_stats() == {"members": 1, "launches": 1, "bytes_in": length(5), "bytes_scratch": 4096 + 64}
    # overlapping, duplicate and unsorted ranges: every touched member goes in once
    ranges = [(tab[30][1] + 10, 5000), (tab[3][1] + 4000, 200), (tab[30][1] + 10, 5000), (tab[31][1], 4096), (tab[3][1], 4096),
              (tab[29][1] + 4095, 2), (tab[10][1] + 1, 1), (tab[3][1] + 4000, 200)]
    touched = {3, 4, 10, 29, 30, 31}
    _check(idx, f, plain, ranges)
    assert idx.last_stats()["members"] == len(touched) and idx.last_stats()["bytes_in"] == sum(length(k) for k in touched)


def test_gather_alignment_and_guard_bytes(eng):
    f, tab, plain, idx = _file(4096)
    lens = list(range(41)) + [16383, 16384, 16385]
    where, ln, dof, cursor = [], [], [], 0
    for dm in range(16):
        for om in range(16):
            for k, n in enumerate(lens):
                base = tab[3 + k % 7][1] - 20 if n <= 40 else tab[2 + dm][1] + 4096 - 48  # (short ones about a member's edge)
                start = ((cursor + 32 + 15) & ~15) + dm
                where.append(base + om)
                ln.append(n)
                dof.append(start)
                cursor = start + n
    room = cursor + 32
    rc, status, dst = _raw_read(eng, idx, f, where, ln, dof, room)
    assert rc == OK and status == [OK] * len(where)
    want = np.full(room, 0xa5, dtype=np.uint8)
    flat = np.frombuffer(plain, dtype=np.uint8)
    for o, n, d in zip(where, ln, dof):
        want[d:d + n] = flat[o:o + n]
    bad = np.nonzero(dst != want)[0]
    assert bad.size == 0, (bad[:8], len(where))


def test_rounds(eng):
    f, tab, plain, idx = _file(0xff00)
    for bad in (-1, (1 << 20) + 1):
        assert eng.lib.md_set_option(eng.ctx, b"bgzf_read_workspace", bad) == -1
    # sixteen stored members of 0xff00 random bytes: about 128 KiB of input and slot each, so 1 MiB holds eight
    rnd = random.Random(9).randbytes(16 * 0xff00)
    g, gidx = gu.bgzf_file(rnd, level=0)
    gx = _gz().BgzfIndex.from_gzi(gzi(gidx[1:]), g)
    ranges = [(0, len(rnd)), (0xff00 * 3 - 5, 0xff00 * 9), (0xff00 * 15, 0xff00), (100, 1)]
    one = gx.read_many(g, ranges)
    assert one == [("Ok", rnd[o:o + n]) for o, n in ranges] and gx.last_stats()["launches"] == 1
    whole = gx.last_stats()
    eng.set_option("bgzf_read_workspace", 0)
    try:
        assert idx.read(f, 0, len(plain)) == plain  # (the text file has four members with bytes)
        assert idx.last_stats()["launches"] == idx.last_stats()["members"] == 4
        five = (0xff00 - 10, 20 + 3 * 0xff00)     # over 5 members of the stored file
        assert gx.read(g, *five) == rnd[five[0]:five[0] + five[1]]
        assert gx.last_stats()["launches"] == gx.last_stats()["members"] == 5
        eng.set_option("bgzf_read_workspace", 1)
        assert gx.read_many(g, ranges) == one
        half = gx.last_stats()
        assert half["launches"] == 2 and (half["members"], half["bytes_in"], half["bytes_scratch"]) == \
               (whole["members"], whole["bytes_in"], whole["bytes_scratch"]) == (16, gidx[16][0], 16 * (0xff00 + 64))
    finally:
        eng.set_option("bgzf_read_workspace", 256)


def test_member_kinds(eng):
    rng = random.Random(11)
    parts = [
        (_text(3000, 21), dict(level=0)),                                    # stored by choice
        (rng.randbytes(5000), dict()),                                       # stored because nothing else pays
        (_text(4000, 22), dict(before=gu.subfield(b"AB", b"xyz"))),          # another subfield in front of BC
        (_text(4100, 23), dict(after=gu.subfield(b"ZZ", b""))),              # ... behind it
        (_text(900, 24), dict(before=gu.subfield(b"Q1", b"12345"), after=gu.subfield(b"Q2", b"\0" * 9))),
        (_text(6000, 25), dict(name=b"reads.bam", comment=b"a comment")),    # FNAME and FCOMMENT
        (_text(2000, 26), dict(name=b"n", hcrc=True)),                       # ... and a header CRC
        (_text(0x10000, 27), dict(level=9)),                                 # the most a member holds
    ]
    members = [gu.bgzf_member(data, **kw) for data, kw in parts] + [gu.EOF_MARKER]
    f, plain = b"".join(members), b"".join(data for data, _ in parts)
    tab, c, u = [], 0, 0
    for m, data in zip(members, [d for d, _ in parts] + [b""]):
        tab.append((c, u))
        c, u = c + len(m), u + len(data)
    tab.append((c, u))
    built, loaded = _gz().BgzfIndex.build(f), _gz().BgzfIndex.from_gzi(gzi(tab[1:-1]), f)
    assert built.entries() == loaded.entries() == tab
    ranges = [(0, len(plain))] + [(tab[k][1], tab[k + 1][1] - tab[k][1]) for k in range(len(parts))] + \
             [(tab[k][1] - 9, 20) for k in range(1, len(parts))]
    _check(built, f, plain, ranges)
    _check(loaded, f, plain, ranges)


def test_virtual_offsets(eng):
    chunks = [_text(500, 31), b"", _text(70000, 32)[:0xffff], _text(40, 33), b"y", _text(3000, 34)]
    f, idx = gu.bgzf_of_members(chunks)
    plain = b"".join(chunks)
    tab = idx + [(len(f), len(plain))]
    x = _gz().BgzfIndex.from_gzi(gzi(idx[1:]), f)
    ranges, want = [], []
    for k in range(len(idx)):  # every member start (the empty ones and the EOF marker too)
        c, u = tab[k]
        n = tab[k + 1][1] - u
        for inside in sorted({0, 1, n - 1, n} & set(range(n + 1))):
            take = min(600, len(plain) - (u + inside))  # (runs on into the following members)
            ranges.append((c << 16 | inside, take))
            want.append(("Ok", plain[u + inside:u + inside + take]))
        if n < 0xffff:
            ranges.append((c << 16 | (n + 1), 1))  # an offset behind the member's output
            want.append(("Error", BAD_INDEX))
    ranges += [((tab[2][0] + 1) << 16, 10), (tab[-1][0] << 16, 0), ((1 << 48) - 1, 5), (7, 5)]  # no member starts there
    want += [("Error", BAD_INDEX)] * 3 + [("Ok", plain[7:12])]
    assert x.read_virtual_many(f, ranges) == want
    # the bad ones touch nothing and do not count
    rc, status, dst = _raw_read(eng, x, f, [(tab[2][0] + 1) << 16, tab[3][0] << 16 | 5], [8, 8], [0, 16], 32, virtual=True)
    assert rc == OK and status == [INVALID_INDEX, OK]
    assert bytes(dst) == b"\xa5" * 16 + plain[tab[3][1] + 5:tab[3][1] + 13] + b"\xa5" * 8
    assert x.last_stats()["members"] == 1
    # a valid virtual offset whose range ends behind the output is the call's error
    assert _raw_read(eng, x, f, [tab[5][0] << 16], [3001], [0], 4000, virtual=True)[0] == INVALID_ARGUMENT


def _isolated(idx, src, plain, tab, bad_members, want_status):
    """one range per member with bytes, and ranges across every edge: those over a bad member fail with want_status (a
    set of names), the others are exact"""
    M = len(tab) - 1
    ranges = [(tab[k][1], tab[k + 1][1] - tab[k][1]) for k in range(M) if tab[k + 1][1] > tab[k][1]]
    ranges += [(u - 50, 100) for _, u in tab[1:-2]] + [(0, len(plain))]
    got = idx.read_many(src, ranges)  # (the call itself is MD_OK: read_many raises otherwise)
    seen = set()
    for (off, n), (st, data) in zip(ranges, got):
        hit = [k for k in bad_members if tab[k][1] < off + n and off < tab[k + 1][1]]
        if hit:
            assert st == "Error" and data in want_status, (off, n, st, data)
            seen.add(data)
        else:
            assert (st, data) == ("Ok", plain[off:off + n]), (off, n, st)
    return seen


def _general_path_says(src):
    """the status md_gz_members_uncompress gives the file: its first failing member's"""
    r = _gz().Members.uncompress(src)
    assert r[0] == "Error"
    return r[1]


def test_damage_is_isolated(eng):
    f, tab, plain, idx = _file(4096)
    k = 7
    c0, c1 = tab[k][0], tab[k + 1][0]
    # a flipped byte in one body: what the same member gets without an index
    flip = lambda at: f[:at] + bytes([f[at] ^ 0x10]) + f[at + 1:]
    seen = set()
    for at in (c0 + 18 + 3, c0 + 18 + (c1 - c0 - 26) // 2):  # in the block's header, among its symbols
        g = flip(at)
        seen |= _isolated(idx, g, plain, tab, [k], {_general_path_says(g)})
    assert BAD_CRC in seen and len(seen) == 2, seen  # (one flip stops the decoder, the other only changes bytes)
    # A flip that loses the end of the last block: the stream runs on behind its 4 096 bytes.  Without an index the decoder
    # has the rest of the file as input and of dst as room, and what it says depends on the members behind this one; here
    # the member has its own bytes and a slot of the size that index and ISIZE agree on, and overrunning that is
    # MD_INVALID_SIZE (md_gz_members_uncompress' word for it on the device, too)
    g = flip(c1 - 8 - 4)
    d = zlib.decompressobj(-15)
    assert len(d.decompress(g[c0 + 18:c1 - 8])) > 4096 and not d.eof
    assert _isolated(idx, g, plain, tab, [k], {BAD_SIZE}) == {BAD_SIZE}
    # a flipped CRC, a changed ISIZE
    g = f[:c1 - 8] + bytes([f[c1 - 8] ^ 1]) + f[c1 - 7:]
    assert _isolated(idx, g, plain, tab, [k], {BAD_CRC}) == {BAD_CRC} == {_general_path_says(g)}
    for delta in (1, -1):
        g = f[:c1 - 4] + struct.pack("<I", 4096 + delta) + f[c1:]
        assert _isolated(idx, g, plain, tab, [k], {BAD_SIZE}) == {BAD_SIZE}
    # two damaged members: a range over both gets the first one's status
    g = f[:c1 - 4] + struct.pack("<I", 4097) + f[c1:tab[21][0] - 8] + b"\0\0\0\0" + f[tab[21][0] - 4:]
    assert _isolated(idx, g, plain, tab, [k, 20], {BAD_SIZE, BAD_CRC}) == {BAD_SIZE, BAD_CRC}
    assert idx.read_many(g, [(0, len(plain)), (tab[20][1], 5)]) == [("Error", BAD_SIZE), ("Error", BAD_CRC)]
    # the same through rounds of one member
    eng.set_option("bgzf_read_workspace", 0)
    try:
        assert idx.read_many(g, [(tab[5][1], 20000), (tab[20][1] - 1, 2), (0, 4096)]) == [("Error", BAD_SIZE), ("Error", BAD_CRC), ("Ok", plain[:4096])]
    finally:
        eng.set_option("bgzf_read_workspace", 256)


def test_an_index_that_is_not_this_files(eng):
    f, tab, plain, idx = _file(4096)
    # u_off of one member shifted by one, the file sound: the members on both sides of that entry are not as the index says
    for delta in (1, -1):
        bent = [(c, u + delta if j == 12 else u) for j, (c, u) in enumerate(tab)]
        x = _gz().BgzfIndex.from_gzi(gzi(bent[1:-1]), f)
        assert x.entries() == bent
        assert _isolated(x, f, plain, tab, [11, 12], {BAD_INDEX}) == {BAD_INDEX}
    # c_off of one entry moved into the member in front of it
    bent = [(c - 9 if j == 12 else c, u) for j, (c, u) in enumerate(tab)]
    x = _gz().BgzfIndex.from_gzi(gzi(bent[1:-1]), f)
    seen = _isolated(x, f, plain, tab, [11, 12], set(_gz()._engine.STATUS_NAMES.values()) - {"Ok"})
    assert seen
    # the index of file A with file B of the same length and other member boundaries: never wrong bytes with MD_OK
    other = _text(150000, 77)
    b, _ = gu.bgzf_file(other, block=3000)
    assert len(b) < len(f)
    b += bytes(len(f) - len(b))  # (NUL padding: a valid file of A's length)
    size = len(plain)
    ranges = [(0, 100), (0, size), (tab[9][1], 4096), (tab[30][1] + 5, 9000), (size - 1, 1)]
    got = idx.read_many(b, ranges)
    assert got[0][0] == "Error"  # (B's first member is not as long as A's)
    for (off, n), (st, data) in zip(ranges, got):
        assert st == "Error" or data == other[off:off + n], (off, n)
    # another length: the call's return value
    rc, status, dst = _raw_read(eng, idx, f + b"\0", [0], [10], [0], 16)
    assert rc == INVALID_INDEX and bytes(dst) == b"\xa5" * 16
    with pytest.raises(_gz()._engine.Error):
        idx.read(f[:-1], 0, 10)


def test_agreement_with_the_member_scan_and_the_writer(eng):
    gz = _gz()
    for block in (0xff00, 4096, 300):
        f, tab, plain, _ = _file(block)
        built = gz.BgzfIndex.build(f)
        scan = gz.Members.scan(f)
        assert built.entries() == tab and list(zip(scan["c_off"], scan["u_off"])) == tab[:-1] and scan["size"] == tab[-1][1]
        assert built.to_gzi() == gzi(tab[1:-1])
        padded = gz.BgzfIndex.build(f + bytes(100))
        assert padded.entries() == tab and padded.info()["src_len"] == len(f) + 100
        assert padded.read(f + bytes(100), tab[-1][1] - 10, 10) == plain[-10:]
    # members without the BC field: no index
    plain_gz = gu.member(_text(3000, 41)) + gu.member(_text(3000, 42))
    with pytest.raises(gz._engine.Error, match="Invalid index"):
        gz.BgzfIndex.build(plain_gz)
    h = ctypes.c_void_p(1)
    assert eng.lib.md_bgzf_index_build(eng.ctx, plain_gz, len(plain_gz), ctypes.byref(h)) == INVALID_INDEX and not h.value
    # a file from md_bgzf_compress reads back through its index
    data = _text(300000, 43)
    for block in (0xff00, 5000):
        w = gz.Bgzf.compress(data, level=4, block=block)
        x = gz.BgzfIndex.build(w)
        assert x.info() == {"src_len": len(w), "members": -(-len(data) // block) + 1, "size": len(data)}
        ranges = [(0, len(data)), (block - 1, 2), (123456, 7890), (len(data) - 1, 1)]
        _check(x, w, data, ranges)
        y = gz.BgzfIndex.from_gzi(x.to_gzi(), w)
        assert y.entries() == x.entries()
        _check(y, w, data, ranges)
