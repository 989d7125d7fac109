"""GZip files of many members WITHOUT size fields, read by speculation (md_gz_members_uncompress, csrc/gz_spec.hip, DESIGN
4f).  Needs an MI355X: `pytest -m gpu`.  Yardsticks: Python's gzip.decompress and gz_members_util.libz_members (zlib with
wbits 31), never the code under test; the candidates of a file are counted in Python by the rule the issue states
(1f 8b 08, no reserved flag bit, 18 bytes left).  The files are the smallest at which each rule of the path can go wrong;
`_files()` builds those of tests 1-6 once, and test 7 runs every one of them down both paths."""
import bisect
import functools
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


@functools.lru_cache(maxsize=None)
def _pool():
    from decompress_amd import workloads
    return workloads.text(11, 3 << 20)


def _text(n, at=0):
    return _pool()[at:at + n]


def _candidates(f):
    """positions that look like a member's start, by the rule of the issue"""
    out, p = [], f.find(b"\x1f\x8b\x08")
    while p >= 0:
        if p + 18 <= len(f) and not f[p + 3] & 0xe0:
            out.append(p)
        p = f.find(b"\x1f\x8b\x08", p + 1)
    return out


def _starts(parts):
    out, pos = [], 0
    for p in parts:
        out.append(pos)
        pos += len(p)
    return out


def _patched(f, at, fn):
    b = bytearray(f)
    b[at] = fn(b[at])
    return bytes(b)


def _stored(payload):
    return b"\x01" + struct.pack("<HH", len(payload), len(payload) ^ 0xffff) + payload


# ---- the files of tests 1-6: name -> (file, dst_cap) ----
def _plain_parts():
    rng = random.Random(0x51ec)
    parts, plain = [], []
    for k in range(300):
        n = 0 if k % 37 == 5 else rng.randint(0, 3000)
        p = _text(n, rng.randrange(1 << 20))
        kind = k % 8
        if kind == 1:
            m = gzip.compress(p, mtime=0)
        elif kind == 2:
            m = gu.member(p, name=b"file%d.txt" % k)
        elif kind == 3:
            m = gu.member(p, comment=b"a comment", hcrc=True)
        elif kind == 4:
            m = gu.member(p, extra=gu.subfield(b"AB", b"x" * (k % 11)), hcrc=k % 16 == 4)
        else:
            m = gu.member(p, level=rng.choice((1, 6, 9)))
        parts.append(m)
        plain.append(p)
    return parts, plain


def _false_parts():
    """test_planted_magic_changes_nothing's construction without BC fields -> parts, plain, indices of the planted ones"""
    plain = _text(100000, 5000)
    fake = gu.member(b"not a member")  # a whole valid member, as the payload of a stored block
    magic = b"\x1f\x8b\x08\x00"
    parts = [gu.member(plain[:30000]), gu.member(fake, body=_stored(fake)), gu.member(plain[30000:50000]),
             gu.member(plain[50000:70000], extra=gu.subfield(b"FK", b"ab" + magic + b"cdefghijklmnopqrstuvwxyz")),
             gu.member(plain[70000:90000]), gu.member(plain[90000:], name=b"n" + magic[:3]),  # (the name's NUL is the FLG byte)
             gu.member(b"tail")]
    return parts, [plain[:30000], fake, plain[30000:50000], plain[50000:70000], plain[70000:90000], plain[90000:], b"tail"], (1, 3, 5)


def _pad_parts():
    """(member, NUL bytes behind it)"""
    t = [_text(4000, 7000 * k) for k in range(6)]
    return [(gu.member(t[0]), 1), (gu.member(t[1]), 0), (gu.member(t[2]), 9), (gu.member(t[3]), 70000), (gu.member(b""), 0),
            (gu.member(t[4]), 0), (gu.member(b""), 3), (gu.member(t[5]), 70000)], t[:4] + [b"", t[4], b"", t[5]]


def _long_parts():
    small = [_text(1500, 3000 * k) for k in range(40)]
    big = _text(1 << 20, 12345)
    plain = small[:20] + [big] + small[20:]
    return [gu.member(p) for p in plain], plain


ROOM_GUESS = 300 << 10


def _room_parts():
    """five members, then one whose stored block holds ROOM_GUESS as four bytes in front of a planted 1f 8b 08 00, then two"""
    t = [_text(2000, 9000 * k) for k in range(7)]
    payload = _text(600, 99) + struct.pack("<I", ROOM_GUESS) + b"\x1f\x8b\x08\x00" + _text(400, 77)
    plain = t[:5] + [payload] + t[5:]
    parts = [gu.member(p) for p in t[:5]] + [gu.member(payload, body=_stored(payload))] + [gu.member(p) for p in t[5:]]
    return parts, plain


def _damages(f, starts, which, hcrc):
    """the damage matrix of test_failures on member `which` of f -> [(name, file, status)]"""
    m, nxt = starts[which], starts[which + 1] if which + 1 < len(starts) else len(f)
    if hcrc:
        at = m + 10 + 2  # behind the fixed bytes and "x\0"
        return [("fhcrc", _patched(f, at, lambda v: v ^ 1), "Invalid GZip header checksum")]
    return [("crc", _patched(f, nxt - 8, lambda v: v ^ 0x10), "Invalid_checksum"),
            ("isize_up", _patched(f, nxt - 4, lambda v: (v + 1) & 255), "Invalid input size"),
            ("isize_down", _patched(f, nxt - 4, lambda v: (v - 1) & 255), "Invalid input size"),
            ("cm", _patched(f, m + 2, lambda v: 7), "Invalid GZip header"),
            ("flag", _patched(f, m + 3, lambda v: v | 0x20), "Invalid GZip header"),
            ("cut_header", f[:m + 5], "Unexpected_end_of_input"),
            ("cut_body", f[:m + 10 + 100], "Unexpected_end_of_input"),
            ("cut_trailer", f[:nxt - 3], "Unexpected_end_of_input")]


@functools.lru_cache(maxsize=None)
def _files():
    out = {}
    parts, plain = _plain_parts()
    out["plain"] = (b"".join(parts), sum(map(len, plain)))
    out["two"] = (gu.member(_text(700)) + gzip.compress(_text(900, 700), mtime=0), 1600)
    parts, plain, _ = _false_parts()
    out["false"] = (b"".join(parts), sum(map(len, plain)))
    padded, plain = _pad_parts()
    out["pads"] = (b"".join(m + b"\0" * pad for m, pad in padded), sum(map(len, plain)))
    parts, plain = _long_parts()
    out["long"] = (b"".join(parts), sum(map(len, plain)))
    three = b"".join(gu.member(_text(50000, 50000 * k)) for k in range(3))
    out["room_exact"] = (three, 150000)
    out["room_short"] = (three, 149999)
    parts, plain = _room_parts()
    out["room_guess"] = (b"".join(parts), sum(map(len, plain)))
    for hcrc in (False, True):
        parts = [gu.member(_text(5000, 5000 * k), hcrc=hcrc, name=b"x" if hcrc else None) for k in range(9)]
        f, starts = b"".join(parts), _starts(parts)
        for which in (0, 4, 8):
            for name, g, _ in _damages(f, starts, which, hcrc):
                out["fail_%s_%d" % (name, which)] = (g, 45000)
        if not hcrc:
            out["fail_garbage"] = (f + b"garbage", 45000)
            out["fail_nul_garbage"] = (f + b"\0\0\0garbage", 45000)
    return out


def _run(gz, name):
    f, cap = _files()[name]
    r = gz.Members.uncompress(f, cap)
    return f, cap, r, gz.Members.last_stats()


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


# ---- 1. plain members ----
def test_plain_members(gz):
    from decompress_amd import engine
    eng = engine.default_engine(0)
    assert eng.lib.md_gz_members_last(eng.ctx, None) < 0  # (NULL out, a live context)
    f, cap, r, s = _run(gz, "plain")
    want = gzip.decompress(f)
    assert len(want) == cap and any(f[p + 3] & 2 for p in _candidates(f)) and any(f[p + 3] & 4 for p in _candidates(f))
    assert r[0] == "Ok" and r[2] == want, r[:2]
    assert r[1] == {"members": 300, "consumed": len(f), "written": cap, "indexed": 0}
    assert s["path"] == 2 and s["members_device"] == 300 and s["members_host"] == 0, s
    assert s["candidates"] == len(_candidates(f)) and s["spans_decoded"] >= 300


def test_two_members(gz):
    f, cap, r, s = _run(gz, "two")
    assert r[0] == "Ok" and r[2] == gzip.decompress(f) and r[1] == {"members": 2, "consumed": len(f), "written": cap, "indexed": 0}
    assert s["path"] == 2 and s["candidates"] == 2 and s["members_device"] == 2 and s["members_host"] == 0, s
    # one member: nothing to speculate about
    one = gu.member(_text(700))
    r = gz.Members.uncompress(one, 700)
    assert r[0] == "Ok" and r[2] == _text(700) and gz.Members.last_stats()["path"] == 0
    # an indexed file says so
    g = gu.bgzf_file(_text(3000), block=1000)[0]
    assert gz.Members.uncompress(g, 3000)[1]["indexed"] == 1 and gz.Members.last_stats()["path"] == 1


# ---- 2. false candidates ----
def test_false_candidates(gz):
    parts, plain, planted = _false_parts()
    f, cap, r, s = _run(gz, "false")
    want = b"".join(plain)
    assert gzip.decompress(f) == want and gu.libz_members(f) == ("ok", want, len(parts))
    assert len(_candidates(f)) == len(parts) + len(planted)  # (every planted magic is a candidate)
    assert r[0] == "Ok" and r[2] == want and r[1] == {"members": len(parts), "consumed": len(f), "written": cap, "indexed": 0}
    assert s["path"] == 2 and s["candidates"] == len(parts) + len(planted), s
    assert s["members_host"] == len(planted) >= 1 and s["members_device"] == len(parts) - len(planted), s


# ---- 3. NUL padding ----
def test_nul_padding(gz):
    padded, plain = _pad_parts()
    f, cap, r, s = _run(gz, "pads")
    want = b"".join(plain)
    assert f[-70000:] == bytes(70000) and padded[4][0][-8:] == bytes(8)
    assert gzip.decompress(f) == want and gu.libz_members(f) == ("ok", want, len(padded))
    assert r[0] == "Ok" and r[2] == want and r[1] == {"members": len(padded), "consumed": len(f), "written": cap, "indexed": 0}
    n_pad = sum(1 for _, pad in padded if pad)
    assert s["path"] == 2 and s["members_host"] == n_pad == 5 and s["members_device"] == len(padded) - n_pad, s


# ---- 4. a long member among small ones ----
def test_long_member_among_small(gz):
    from decompress_amd import engine
    parts, plain = _long_parts()
    f, cap, r, s = _run(gz, "long")
    want = b"".join(plain)
    assert len(parts[20]) - 18 >= 96 << 10 and (len(parts[20]) - 18) * 1024 >= len(f)  # rule (c) holds for the long one alone
    assert len(_candidates(f)) == 41
    assert r[0] == "Ok" and r[2] == want and r[1]["members"] == 41
    assert s["path"] == 2 and s["spans_long"] == 1 and s["members_host"] == 1 and s["members_device"] == 40, s
    eng = engine.default_engine(0)
    eng.set_option("inflate_parallel_min", 4096)  # above the member's size: no span is long
    try:
        r = gz.Members.uncompress(f, cap)
        s = gz.Members.last_stats()
    finally:
        eng.set_option("inflate_parallel_min", 96)
    assert r[0] == "Ok" and r[2] == want
    assert s["spans_long"] == 0 and s["members_device"] == 41 and s["members_host"] == 0, s


# ---- 5. room ----
def test_room(gz):
    f, cap, r, s = _run(gz, "room_exact")
    assert r[0] == "Ok" and r[2] == _text(150000) and s["members_device"] == 3 and s["spans_no_room"] == 0, (r[:2], s)
    f, cap, r, s = _run(gz, "room_short")
    assert r[:2] == ("Error", "Unexpected_end_of_output") and r[2]["members"] == 2 and r[2]["written"] == 100000 and r[3] == _text(100000)
    assert r[2]["consumed"] == len(f) - len(gu.member(_text(50000, 100000))) and r[2]["indexed"] == 0
    assert s["path"] == 2 and s["spans_no_room"] == 1 and s["members_device"] == 2, s
    # a guess that is plausible and too large: the span in front of the planted magic
    parts, plain = _room_parts()
    f, cap, r, s = _run(gz, "room_guess")
    want = b"".join(plain)
    starts, cands = _starts(parts), _candidates(f)
    assert len(cands) == len(parts) + 1 and cands[:6] == starts[:6] and starts[5] < cands[6] < starts[6]
    body_len = cands[6] - cands[5] - 10 - 8
    guess = struct.unpack_from("<I", f, cands[6] - 4)[0]
    assert guess == ROOM_GUESS and guess <= 1032 * body_len + 8   # rule (b) lets it through
    assert body_len < 96 << 10                                     # so does rule (c)
    assert sum(map(len, plain[:5])) + guess > cap == len(want)     # and rule (d) stops it
    assert gzip.decompress(f) == want
    assert r[0] == "Ok" and r[2] == want and r[1] == {"members": len(parts), "consumed": len(f), "written": cap, "indexed": 0}
    assert s["path"] == 2 and s["spans_no_room"] >= 1 and s["members_device"] == 5 and s["members_host"] == 3, s


# ---- 6. failures ----
def test_failures(gz):
    for hcrc in (False, True):
        parts = [gu.member(_text(5000, 5000 * k), hcrc=hcrc, name=b"x" if hcrc else None) for k in range(9)]
        f, starts = b"".join(parts), _starts(parts)
        assert gu.libz_members(f)[0] == "ok"
        for which in (0, 4, 8):
            for name, g, status in _damages(f, starts, which, hcrc):
                assert g == _files()["fail_%s_%d" % (name, which)][0]
                r = _fails(gz, g, 45000, status, python_too=name not in ("flag", "fhcrc"))
                assert r[2]["members"] == which, (name, which)
                if which:  # (member 0 without its magic is no candidate: such a file is the host loop's)
                    assert gz.Members.last_stats()["path"] == 2, (name, which)
    f = _files()["fail_garbage"][0][:-7]
    r = _fails(gz, f + b"garbage", 45000, "Invalid GZip header")
    assert r[2]["members"] == 9 and gz.Members.last_stats()["members_device"] == 8
    _fails(gz, f + b"\0\0\0garbage", 45000, "Invalid GZip header")


# ---- 7. parity with the path it replaces ----
def test_parity_with_general_path(gz):
    from decompress_amd import engine
    eng = engine.default_engine(0)
    files = dict(_files())
    g, idx = gu.bgzf_file(_text(150000), block=50000)
    m1 = idx[1][0]
    for delta in (-1, 1):
        bs = struct.unpack_from("<H", g, m1 + 16)[0] + delta
        files["bsize%+d" % delta] = (g[:m1 + 16] + struct.pack("<H", bs) + g[m1 + 18:], 150000)
    got = {}
    try:
        for spec in (0, 1):
            eng.set_option("gz_members_speculate", spec)
            for name, (f, cap) in files.items():
                got[name, spec] = gz.Members.uncompress(f, cap)
                assert gz.Members.last_stats()["path"] in ((0,) if spec == 0 else (0, 2)), name
                if name.startswith("bsize"):
                    assert got[name, spec][0] == "Ok" and got[name, spec][1]["indexed"] == 0 and gz.Members.last_stats()["path"] == 2 * spec
    finally:
        eng.set_option("gz_members_speculate", 1)
    for name in files:
        assert got[name, 0] == got[name, 1], name


# ---- 8. seeded fuzz ----
FUZZ_SEED = 0x5bec


def _fuzz_cases():
    """200 files in the style of test_fuzz_200_files, kinds plain and mixed -> (file, cap, kind, damaged)"""
    rng = random.Random(FUZZ_SEED)
    for case in range(200):
        kind = rng.choice(("plain", "mixed"))
        parts, size = [], 0
        for _ in range(rng.randint(1, 40)):
            n = rng.choice((0, 1, 2, rng.randint(3, 300), rng.randint(300, 8000)))
            p = _text(n, rng.randrange(1 << 20)) if rng.random() < 0.7 else rng.randbytes(n)
            opts = {}
            if rng.random() < 0.2:
                opts["name"] = b"n" * rng.randint(0, 20)
            if rng.random() < 0.2:
                opts["comment"] = b"c" * rng.randint(0, 20)
            if rng.random() < 0.3:
                opts["hcrc"] = True
            lvl = rng.choice((0, 1, 6, 9))
            if kind == "mixed" and rng.random() < 0.5:
                before = gu.subfield(b"AA", rng.randbytes(rng.randint(0, 9))) if rng.random() < 0.3 else b""
                parts.append(gu.bgzf_member(p, lvl, before=before, **opts))
            else:
                extra = gu.subfield(b"QQ", rng.randbytes(rng.randint(0, 9))) if rng.random() < 0.3 else None
                parts.append(gu.member(p, lvl, extra=extra, **opts))
            size += n
        if rng.random() < 0.5:
            parts.append(gu.EOF_MARKER)
        f = b"".join(parts) + b"\0" * rng.choice((0, 0, 0, 5))
        if case % 3 == 0:
            at = rng.randrange(len(f))
            f = _patched(f, at, lambda v: v ^ (1 << rng.randrange(8)))
        yield f, size + 64, kind, case % 3 == 0


def test_fuzz_200_files(gz):
    spec = agree_ok = agree_bad = 0
    for case, (f, cap, kind, damaged) in enumerate(_fuzz_cases()):
        z = gu.libz_members(f)
        r = gz.Members.uncompress(f, cap)
        spec += gz.Members.last_stats()["path"] == 2
        if z[0] == "ok":
            assert r[0] == "Ok" and r[2] == z[1], (case, r[:2])
            assert r[1]["consumed"] == len(f) and r[1]["members"] == z[2]
            if not damaged:
                assert gzip.decompress(f) == z[1]
            agree_ok += 1
        else:
            assert r[0] == "Error", (case, r[:2])
            assert r[2]["members"] == z[2] and r[2]["consumed"] == z[3] and r[3] == z[1], case
            agree_bad += 1
    assert agree_ok + agree_bad == 200 and agree_bad >= 20 and spec >= 120, (agree_ok, agree_bad, spec)


# ---- 9. at size ----
def test_64_mib_of_plain_members(gz):
    from decompress_amd import workloads
    cat = b"".join(workloads.corpus().values())
    src = (cat * ((64 << 20) // len(cat) + 1))[:64 << 20]
    parts = [gu.member(src[k:k + 0xff00], level=1) for k in range(0, len(src), 0xff00)]
    f, starts = b"".join(parts), set(_starts(parts))
    assert len(parts) == 1029
    cands = _candidates(f)
    assert starts <= set(cands)
    ends = sorted(starts) + [len(f)]
    false = [p for p in cands if p not in starts]
    cut = {bisect.bisect_right(ends, p) - 1 for p in false}  # the members a false candidate lies in
    r = gz.Members.uncompress(f, len(src))
    s = gz.Members.last_stats()
    assert r[0] == "Ok" and r[1] == {"members": len(parts), "consumed": len(f), "written": len(src), "indexed": 0}
    assert r[2] == src and gzip.decompress(f) == src
    assert s["path"] == 2 and s["candidates"] == len(cands), s
    assert s["members_host"] == len(cut) and s["members_device"] + s["members_host"] == len(parts), (s, len(cut))
