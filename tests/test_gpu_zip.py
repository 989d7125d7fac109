"""ZIP archives on the GPU (md_zip_uncompress, md_zip_compress; csrc/zip_kernels.hip).  Needs an MI355X:
`pytest -m gpu`.  Yardsticks: Python's zipfile and zlib for validity and plaintext, oracle.deflate_raw for the bytes of the
writer's bodies, the test's own construction (tests/zip_util.py) for hand-built and damaged archives - never the code
under test."""
import ctypes
import io
import random
import struct
import zipfile
import zlib

import pytest

from tests import zip_util as zu

pytestmark = pytest.mark.gpu
ALNUM = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
OK, END_OF_OUTPUT, CHECKSUM, SIZE, ZIP_HEADER, UNSUPPORTED = 0, 2, 9, 12, 19, 20


@pytest.fixture(scope="module")
def eng():
    from decompress_amd import engine
    return engine.default_engine(0)


@pytest.fixture(scope="module")
def zp():
    from decompress_amd import zp
    return zp


def _text(n, seed=1):
    from decompress_amd import workloads
    return workloads.text(seed, n)


def _rand(n, seed=1):
    return random.Random(seed).randbytes(n)


def _contents(blob):
    with zipfile.ZipFile(io.BytesIO(blob)) as z:
        assert z.testzip() is None
        return [z.read(i) for i in z.infolist()]


def _run(eng, blob, select=None, cap=None):
    """md_zip_uncompress as a C caller sees it -> (rc, status[], out_off[], (entries, failed, written), dst bytes)"""
    from decompress_amd import _lib, zp
    ents, info = zp.directory(blob)
    idx = list(range(len(ents))) if select is None else list(select)
    k = len(idx)
    need = sum(ents[i]["usize"] for i in idx if 0 <= i < len(ents))
    cap = need if cap is None else cap
    dst = ctypes.create_string_buffer(b"\xa5" * (cap + 1), cap + 1)
    off, st, res = (ctypes.c_uint64 * (k + 1))(), (ctypes.c_int32 * max(k, 1))(), _lib.ZipResult()
    sel = (ctypes.c_uint64 * max(k, 1))(*idx) if select is not None else None
    rc = eng.lib.md_zip_uncompress(eng.ctx, blob, len(blob), sel, k if select is not None else 0, dst, cap, off, st, ctypes.byref(res))
    assert dst.raw[cap:] == b"\xa5"
    return rc, list(st)[:k], list(off), (res.entries, res.failed, res.written), dst.raw[:cap]


def _check_all(eng, blob, want, label=""):
    """every entry MD_OK, the bytes `want` back to back, out_off their running sizes"""
    rc, st, off, res, out = _run(eng, blob)
    assert rc == 0 and st == [OK] * len(want), (label, rc, st)
    sizes = [len(d) for d in want]
    assert off == [sum(sizes[:j]) for j in range(len(want) + 1)], label
    assert res == (len(want), 0, sum(sizes)), label
    assert out == b"".join(want), label


def _segment(eng, kib):
    assert eng.lib.md_set_option(eng.ctx, b"zip_crc_segment", kib) == 0


# ---- segments ----
def test_segment_option_range(eng):
    for bad in (-1, 1, 3, (1 << 20) + 1):
        assert eng.lib.md_set_option(eng.ctx, b"zip_crc_segment", bad) == -1
    for good in (4, 1 << 20, 0):
        _segment(eng, good)


def test_segments_of_4_kib(eng):
    sizes = (0, 1, 4095, 4096, 4097, 3 * 4096 + 17)
    files = [("s%d" % n, _rand(n, n)) for n in sizes] + [("d%d" % n, _text(n, n)) for n in sizes]
    blob = zu.archive([zu.entry(n, d, method=0 if n[0] == "s" else 8) for n, d in files])[0]
    assert _contents(blob) == [d for _, d in files]
    _segment(eng, 4)
    try:
        _check_all(eng, blob, [d for _, d in files])
    finally:
        _segment(eng, 0)


def test_segments_around_every_default(eng):
    sizes = [(1 << k) + d for k in range(16, 21) for d in (-1, 0, 1)]
    text = _text((1 << 20) + 1, 7)
    files = [("s%d" % n, text[-n:]) for n in sizes] + [("d%d" % n, text[:n]) for n in sizes]
    blob = zu.archive([zu.entry(n, d, method=0 if n[0] == "s" else 8, level=1) for n, d in files])[0]
    with zipfile.ZipFile(io.BytesIO(blob)) as z:
        assert [(i.file_size, i.CRC) for i in z.infolist()] == [(len(d), zlib.crc32(d)) for _, d in files]
    _check_all(eng, blob, [d for _, d in files])


# ---- the stored copy: every (source, destination) alignment ----
def test_stored_copy_alignments(eng):
    rng = random.Random(3)
    missing = {(s, d) for s in range(16) for d in range(16)}
    files, pos, out, count = [], 0, 0, {}
    while missing and len(files) < 600:
        # a name length that puts the body on a source residue still missing for this destination residue, if there is one
        free = [n for n in range(1, 18) if count.get(n, 0) < 62 ** n]  # (names are counters in base 62: 62 of length 1)
        name_len = rng.choice([n for n in free if ((pos + 30 + n) % 16, out % 16) in missing] or free)
        # a size that leaves the next entry on a destination residue that still misses a pair; now and then a short entry
        wanted = [n for n in range(16, 41) if any(d == (out + n) % 16 for _, d in missing)]
        size = rng.choice(wanted or range(16, 41)) if rng.random() < 0.8 else rng.randrange(0, 16)
        if size >= 16:
            missing.discard(((pos + 30 + name_len) % 16, out % 16))
        count[name_len] = count.get(name_len, 0) + 1
        name = "".join(ALNUM[(count[name_len] - 1) // 62 ** p % 62] for p in range(name_len))
        files.append((name, _rand(size, len(files))))
        pos += 30 + name_len + size
        out += size
    assert len({n for n, _ in files}) == len(files) and len(files) < 400
    blob = zu.zipfile_bytes(files, zipfile.ZIP_STORED)
    pairs, at = set(), 0
    with zipfile.ZipFile(io.BytesIO(blob)) as z:
        for i in z.infolist():
            assert i.compress_type == 0 and blob[i.header_offset + 28:i.header_offset + 30] == b"\0\0"  # (no local extra field)
            if i.file_size >= 16:  # (long enough for one 16-byte store, with head or tail bytes around it)
                pairs.add(((i.header_offset + 30 + len(i.filename)) % 16, at % 16))
            at += i.file_size
    assert len(pairs) == 256
    _check_all(eng, blob, [d for _, d in files])


# ---- forms ----
def test_every_hand_built_form(eng):
    for label, blob, want in zu.forms():
        assert _contents(blob) == [d for _, d in want], label
        _check_all(eng, blob, [d for _, d in want], label)
    blob, want = zu.fake_end_archive()
    _check_all(eng, blob, [d for _, d in want], "fake end record")


def test_zipfile_written(eng, zp):
    files = zu.sample_files(5) + [("big.txt", _text(300000, 9))]
    for level in (1, 6, 9):
        blob = zu.zipfile_bytes(files, zipfile.ZIP_DEFLATED, level)
        _check_all(eng, blob, [d for _, d in files], level)
    blob = zu.zipfile_bytes(files, zipfile.ZIP_STORED)
    assert zp.uncompress(blob) == [(n.encode("utf-8"), "Ok", d) for n, d in files]
    rc, st, off, res, out = _run(eng, zu.zipfile_bytes([], zipfile.ZIP_STORED))
    assert (rc, st, off, res, out) == (0, [], [0], (0, 0, 0), b"")


# ---- selection ----
def test_selection(eng, zp):
    files = zu.sample_files(6)
    blob = zu.zipfile_bytes(files, zipfile.ZIP_DEFLATED, 6)
    for sel in ([1, 3, 5], [6, 5, 4, 3, 2, 1, 0], [2, 0, 0, 6, 0], [4], []):
        rc, st, off, res, out = _run(eng, blob, select=sel)
        want = [files[i][1] for i in sel]
        assert rc == 0 and st == [OK] * len(sel) and res == (len(sel), 0, sum(map(len, want))), sel
        assert out == b"".join(want) and off == [sum(len(d) for d in want[:j]) for j in range(len(sel) + 1)], sel
    assert zp.uncompress(blob, select=[6, 0]) == [(files[6][0].encode(), "Ok", files[6][1]), (files[0][0].encode(), "Ok", files[0][1])]
    for sel in ([7], [0, 1 << 40]):
        assert _run(eng, blob, select=sel)[0] == -1, sel


# ---- damage: one entry, the neighbours whole ----
def _damage_base():
    texts = [_text(3000 + 517 * k, 20 + k) for k in range(10)]
    ents = [zu.entry("f%d" % k, t, method=0 if k in (2, 6) else 8) for k, t in enumerate(texts)]
    blob, layout = zu.archive(ents)
    return bytearray(blob), layout, ents, texts


def _poke(blob, at, fmt, value):
    out = bytearray(blob)
    struct.pack_into(fmt, out, at, value)
    return bytes(out)


def test_damage_stays_with_its_entry(eng):
    blob, layout, ents, texts = _damage_base()
    assert _contents(bytes(blob)) == texts
    L = lambda k: layout[k]["local"]
    C = lambda k: layout[k]["central"]
    flipped = bytearray(blob)
    flipped[layout[3]["body"] + ents[3]["csize"] // 2] ^= 0x10
    cases = [
        ("a flipped body byte", 3, bytes(flipped), None),
        ("a flipped byte of a stored body", 2, _poke(blob, layout[2]["body"] + 100, "<B", blob[layout[2]["body"] + 100] ^ 1), CHECKSUM),
        ("the directory's crc off by one", 4, _poke(blob, C(4) + 16, "<I", (ents[4]["crc"] + 1) & 0xffffffff), CHECKSUM),
        ("usize + 1", 5, _poke(blob, C(5) + 24, "<I", ents[5]["usize"] + 1), SIZE),
        ("usize - 1", 5, _poke(blob, C(5) + 24, "<I", ents[5]["usize"] - 1), END_OF_OUTPUT),
        ("csize + 1", 3, _poke(blob, C(3) + 20, "<I", ents[3]["csize"] + 1), SIZE),
        ("stored, csize != usize", 6, _poke(blob, C(6) + 24, "<I", ents[6]["usize"] - 1), SIZE),
        ("a broken local signature", 1, _poke(blob, L(1), "<I", 0x04034b51), ZIP_HEADER),
        ("a changed local name", 7, _poke(blob, L(7) + 31, "<B", ord("9")), ZIP_HEADER),
        ("a local name of another length", 7, _poke(blob, L(7) + 26, "<H", 3), ZIP_HEADER),
        ("a body that reaches into the directory", 9, _poke(blob, C(9) + 20, "<I", ents[9]["csize"] + 1), ZIP_HEADER),
        ("a header offset inside the directory", 8, _poke(blob, C(8) + 42, "<I", C(0) + 1), ZIP_HEADER),
        ("encrypted", 0, _poke(blob, C(0) + 8, "<H", 1), UNSUPPORTED),
        ("method 12", 8, _poke(blob, C(8) + 10, "<H", 12), UNSUPPORTED),
    ]
    for label, j, bad, want in cases:
        rc, st, off, res, out = _run(eng, bad)
        assert rc == 0 and res[:2] == (10, 1), (label, rc, res, st)
        assert st[j] != OK and (want is None or st[j] == want), (label, st[j])
        assert [s for k, s in enumerate(st) if k != j] == [OK] * 9, (label, st)
        for k in range(10):
            if k != j:
                assert out[off[k]:off[k + 1]] == texts[k], (label, k)
    # two damaged entries side by side
    both = _poke(_poke(blob, C(4) + 16, "<I", 0), L(5), "<I", 0)
    rc, st, off, res, out = _run(eng, both)
    assert rc == 0 and res[:2] == (10, 2) and st[4] == CHECKSUM and st[5] == ZIP_HEADER and out[off[6]:off[7]] == texts[6]


def test_room(eng):
    files = zu.sample_files(8)
    blob = zu.zipfile_bytes(files, zipfile.ZIP_DEFLATED, 6)
    need = sum(len(d) for _, d in files)
    rc, st, off, res, out = _run(eng, blob, cap=need - 1)
    assert rc == END_OF_OUTPUT and res == (len(files), 0, need) and out == b"\xa5" * (need - 1)
    assert off[-1] == need
    rc, st, off, res, out = _run(eng, blob, cap=need + 5)
    assert rc == 0 and res == (len(files), 0, need) and out[:need] == b"".join(d for _, d in files)


def test_a_bad_directory_is_the_calls_status(eng):
    blob = zu.zipfile_bytes(zu.sample_files(8), zipfile.ZIP_DEFLATED, 6)
    from decompress_amd import _lib
    res, off, st = _lib.ZipResult(), (ctypes.c_uint64 * 16)(), (ctypes.c_int32 * 16)()
    dst = ctypes.create_string_buffer(1 << 20)
    for bad in (blob[:-1], blob + b"x", b""):
        assert eng.lib.md_zip_uncompress(eng.ctx, bad, len(bad), None, 0, dst, 1 << 20, off, st, ctypes.byref(res)) == 18


# ---- count ----
def test_4096_entries(eng):
    from decompress_amd import workloads
    files = [("c/%04d" % k, workloads.corpus_slice(k, 4096)) for k in range(4096)]
    blob = zu.zipfile_bytes(files, zipfile.ZIP_DEFLATED, 6)
    _check_all(eng, blob, [d for _, d in files])


def test_70000_empty_entries(eng):
    blob = zu.zipfile_bytes([("e%d" % k, b"") for k in range(70000)], zipfile.ZIP_STORED)
    rc, st, off, res, out = _run(eng, blob)
    assert rc == 0 and st == [OK] * 70000 and res == (70000, 0, 0) and off == [0] * 70001


# ---- the writer ----
def _written_ok(zp, oracle, files, level, out):
    names = [n.encode("utf-8") if isinstance(n, str) else n for n, _ in files]
    with zipfile.ZipFile(io.BytesIO(out)) as z:
        assert z.testzip() is None
        infos = z.infolist()
        assert [i.orig_filename.encode("utf-8" if i.flag_bits & 0x800 else "cp437") for i in infos] == names
        for i, (name, (_, data)) in zip(infos, zip(names, files)):
            assert z.read(i) == data
            assert i.flag_bits == (0x800 if any(b >= 0x80 for b in name) else 0), name
            at = i.header_offset + 30 + len(name)
            assert out[i.header_offset + 26:i.header_offset + 30] == struct.pack("<HH", len(name), 0)  # (no extra field)
            body = oracle.deflate_raw(data, level, 4096, 0, True)[0] if level and data else None
            if body is not None and len(body) < len(data):
                assert i.compress_type == 8 and i.extract_version == 20 and out[at:at + i.compress_size] == body, name
            else:
                assert i.compress_type == 0 and i.extract_version == 10 and out[at:at + i.compress_size] == data, name
    assert len(out) <= zp.compress_bound(files)
    assert zp.uncompress(out) == [(n, "Ok", d) for n, (_, d) in zip(names, files)]


def test_writer(zp, oracle):
    files = [("text.txt", _text(100000, 1)), ("noise.bin", _rand(30000, 2)), ("empty", b""), ("dir/", b""), ("one", b"x"),
             ("naïve/ü.txt", _text(5000, 3)), ("zeros", bytes(200000)), ("short", b"abcabcabcabcabcabcabcabcabcabcabc"), ("big", _text(700000, 4))]
    outs = {}
    for level in (0, 1, 6, 9):
        outs[level] = zp.compress(files, level=level)
        _written_ok(zp, oracle, files, level, outs[level])
        assert zu.SIG_END64 not in outs[level][-100:]
    with zipfile.ZipFile(io.BytesIO(outs[6])) as z:
        kinds = {i.filename: i.compress_type for i in z.infolist()}
    assert kinds["noise.bin"] == kinds["empty"] == kinds["dir/"] == kinds["one"] == 0 and kinds["text.txt"] == kinds["zeros"] == kinds["big"] == 8
    assert zp.compress(files, level=6) == outs[6]  # (the bytes depend on files and level alone)
    assert zp.compress([], level=6) == zu.zipfile_bytes([], zipfile.ZIP_STORED)
    with pytest.raises(Exception, match="Unexpected_end_of_output"):
        zp.compress(files, level=6, dst_len=len(outs[6]) - 1)
    assert zp.compress(files, level=6, dst_len=len(outs[6])) == outs[6]


def test_writer_many_files_and_zip64(zp, oracle):
    for n in (0xfffe, 0xffff, 70000):
        files = [("e%d" % k, b"") for k in range(n)]
        files[7] = ("seven", _text(9000, 7))
        out = zp.compress(files, level=6)
        assert (zu.SIG_END64 in out[-120:]) == (n > 0xfffe) and (zu.SIG_LOC64 in out[-60:]) == (n > 0xfffe), n
        with zipfile.ZipFile(io.BytesIO(out)) as z:
            assert len(z.infolist()) == n and z.read("seven") == files[7][1] and z.read("e%d" % (n - 1)) == b""
        if n == 70000:
            _written_ok(zp, oracle, files, 6, out)


def test_writer_refusals(eng):
    from decompress_amd import _lib
    src = _text(1 << 16, 5)
    dst = ctypes.create_string_buffer(1 << 18)
    w = ctypes.c_size_t()

    def call(level, files, src_len=len(src), cap=1 << 18):
        arr = (_lib.ZipSource * max(len(files), 1))(*files)
        return eng.lib.md_zip_compress(eng.ctx, level, len(files), arr, src, src_len, dst, cap, ctypes.byref(w))

    S = _lib.ZipSource
    assert call(6, [S(b"ok", 2, 0, 100, 0, 0, 0x21)]) == 0 and w.value > 0
    assert call(6, [S(b"ok", 2, len(src) - 99, 100, 0, 0, 0x21)]) == -1  # a file beyond src_len
    assert call(6, [S(b"ok", 2, len(src) + 1, 0, 0, 0, 0x21)]) == -1
    assert call(6, [S(b"ok", 2, 0, 0xfffffff1, 0, 0, 0x21)], src_len=1 << 33) == -1  # len > MD_MAX_STREAM
    assert call(6, [S(b"ok", 0, 0, 100, 0, 0, 0x21)]) == -1
    assert call(6, [S(b"ok", 0x10000, 0, 100, 0, 0, 0x21)]) == -1
    assert call(6, [S(None, 2, 0, 100, 0, 0, 0x21)]) == -1
    assert call(-1, [S(b"ok", 2, 0, 100, 0, 0, 0x21)]) == -1 and call(10, [S(b"ok", 2, 0, 100, 0, 0, 0x21)]) == -1
    # an archive whose bound reaches 4 GiB: the files may overlap, so 65 536 times the same 64 KiB will do
    many = [S(b"f", 1, 0, 1 << 16, 0, 0, 0x21)] * (1 << 16)
    assert eng.lib.md_zip_compress_bound(len(many), (_lib.ZipSource * len(many))(*many)) >= 1 << 32
    assert call(6, many) == -1
    assert call(6, [S(b"ok", 2, 0, 100, 0, 0, 0x21)], cap=50) == END_OF_OUTPUT
