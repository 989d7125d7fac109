"""CPU-side checks of the ZIP entry points (md_zip_*): declared, exported and bound; md_zip_directory against
Python's zipfile on every field it reports, for archives zipfile wrote and for every hand-built form; each rule of the
directory's reading broken alone; truncations; misuse refused without a device; the bound's arithmetic; the new kernels
use no scratch."""
import ctypes
import io
import os
import re
import struct
import zipfile

import pytest

from decompress_amd import _lib, build, zp
from tests import zip_util as zu
from tests.test_inf_batch_abi import _all_kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["md_zip_directory", "md_zip_uncompress", "md_zip_compress_bound", "md_zip_compress"]
KERNELS = ["local_kernel", "segment_kernel", "verdict_kernel", "sizes_kernel", "pack_kernel"]
BAD = 18  # MD_INVALID_ZIP_DIRECTORY


def test_declared_exported_bound():
    build.build()
    assert "zip_kernels.hip" in build.SOURCES and "capi_zip.cpp" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    so = ctypes.CDLL(_lib.SO)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert hasattr(so, f), f
        assert f in bound, f
    for s in ("md_zip_entry", "md_zip_info", "md_zip_result", "md_zip_source", "zip_crc_segment"):
        assert s in hdr
    assert ctypes.sizeof(_lib.ZipEntry) == 56 and ctypes.sizeof(_lib.ZipEntry) % 8 == 0
    assert ctypes.sizeof(_lib.ZipInfo) == ctypes.sizeof(ctypes.c_size_t) + 5 * 8 + 8
    assert ctypes.sizeof(_lib.ZipResult) == 2 * ctypes.sizeof(ctypes.c_size_t) + 8
    assert ctypes.sizeof(_lib.ZipSource) == ctypes.sizeof(ctypes.c_void_p) + ctypes.sizeof(ctypes.c_size_t) + 16 + 8
    lib = _lib.load()
    assert lib.md_version() == 0x000300
    assert [lib.md_status_string(k) for k in (18, 19, 20)] == [b"Invalid ZIP directory", b"Invalid ZIP local header", b"Unsupported ZIP entry"]
    from decompress_amd import engine
    assert [engine.STATUS_NAMES[k] for k in (18, 19, 20)] == ["Invalid ZIP directory", "Invalid ZIP local header", "Unsupported ZIP entry"]


def _same_as_zipfile(blob, label):
    ents, info = zp.directory(blob)
    with zipfile.ZipFile(io.BytesIO(blob)) as z:
        want = z.infolist()
        assert info["comment_len"] == len(z.comment) and blob[info["comment_off"]:info["comment_off"] + info["comment_len"]] == z.comment, label
    assert info["entries"] == len(ents) == len(want), label
    assert info["total_usize"] == sum(i.file_size for i in want), label
    for e, i in zip(ents, want):
        name = i.orig_filename.encode("utf-8" if i.flag_bits & 0x800 else "cp437")
        assert (e["header_off"], e["csize"], e["usize"], e["crc32"], e["method"], e["flags"], e["name"]) == \
               (i.header_offset, i.compress_size, i.file_size, i.CRC, i.compress_type, i.flag_bits, name), (label, name)
        assert e["external_attr"] == i.external_attr and blob[e["header_off"]:e["header_off"] + 4] == zu.SIG_LOCAL, (label, name)
    return info


def test_directory_equals_zipfile_on_zipfile_written_archives():
    files = zu.sample_files(2)
    stored = zu.zipfile_bytes(files, zipfile.ZIP_STORED)
    deflated = zu.zipfile_bytes(files, zipfile.ZIP_DEFLATED, 6)
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w") as z:  # mixed, with directory entries
        for k, (n, d) in enumerate(files):
            z.writestr(n, d, compress_type=zipfile.ZIP_DEFLATED if k & 1 else zipfile.ZIP_STORED)
        z.writestr("another/dir/", b"")
    empty = zu.zipfile_bytes([], zipfile.ZIP_STORED)
    assert len(empty) == 22
    for label, blob in (("stored", stored), ("deflated", deflated), ("mixed", buf.getvalue()), ("empty", empty),
                        ("comment", zu.zipfile_bytes(files, zipfile.ZIP_DEFLATED, 6, comment=b"hello" * 50)),
                        ("prefix", b"MZ" + bytes(1000) + deflated)):
        info = _same_as_zipfile(blob, label)
        assert info["prefix"] == (1002 if label == "prefix" else 0) and info["zip64"] == 0
        assert info["prefix"] + info["dir_off"] + info["dir_size"] + 22 + info["comment_len"] == len(blob)


def test_directory_of_70000_empty_entries():
    blob = zu.zipfile_bytes([("e%d" % k, b"") for k in range(70000)], zipfile.ZIP_STORED)
    assert zu.SIG_END64 in blob[-200:]  # (zipfile wrote the ZIP64 end record itself)
    info = _same_as_zipfile(blob, "70000")
    assert info["entries"] == 70000 and info["zip64"] == 1 and info["total_usize"] == 0


def test_directory_equals_zipfile_on_every_hand_built_form():
    n = 0
    for label, blob, want in zu.forms():
        info = _same_as_zipfile(blob, label)
        assert [e["name"] for e in zp.directory(blob)[0]] == [name for name, _ in want]
        assert info["zip64"] == (1 if "zip64_end" in label or "everything" in label else 0), label
        assert (info["prefix"] > 0) == ("prefix" in label), label
        n += 1
    assert n >= 20


def test_fake_end_record_is_not_taken():
    blob, want = zu.fake_end_archive()
    ents, info = zp.directory(blob)
    assert [(e["name"], e["usize"]) for e in ents] == [(n, len(d)) for n, d in want]
    assert info["comment_len"] == len(zu.FAKE_END_COMMENT) and info["entries"] == 3


def _status(blob):
    lib = _lib.load()
    info = _lib.ZipInfo()
    return lib.md_zip_directory(bytes(blob), len(blob), ctypes.byref(info), None, 0)


def _good(**kw):
    small = [("a", b"hello hello hello hello"), ("b/", b""), ("c.bin", bytes(range(40)))]
    extra = {k: kw.pop(k) for k in ("zip64_dir",) if k in kw}
    blob, layout = zu.archive([zu.entry(n, d, method=8 if d else 0, **extra) for n, d in small], **kw)
    assert _status(blob) == 0
    return bytearray(blob), layout


def _poke(blob, at, fmt, value):
    out = bytearray(blob)
    struct.pack_into(fmt, out, at, value)
    return out


def test_each_rule_broken_alone():
    blob, layout = _good()
    end = len(blob) - 22
    dir_size, dir_off = struct.unpack_from("<II", blob, end + 12)
    cases = {
        "bytes behind the comment": blob + b"\0",
        "no end record": blob[:end] + b"PK\5\7" + blob[end + 4:],
        "comment shorter than its length": _poke(blob, end + 20, "<H", 1),
        "this disk is not 0": _poke(blob, end + 4, "<H", 1),
        "the directory's disk is not 0": _poke(blob, end + 6, "<H", 1),
        "entries on this disk differ from the total": _poke(blob, end + 8, "<H", 2),
        "one entry more than headers": _poke(_poke(blob, end + 8, "<H", 4), end + 10, "<H", 4),
        "one entry fewer: the headers do not fill the directory": _poke(_poke(blob, end + 8, "<H", 2), end + 10, "<H", 2),
        "a negative prefix": _poke(blob, end + 16, "<I", dir_off + 1),
        "a directory larger than the file in front of it": _poke(blob, end + 12, "<I", end + 1),
        "a central header's signature": _poke(blob, layout[1]["central"], "<I", 0x02014b51),
        "a name that leaves the directory": _poke(blob, layout[2]["central"] + 28, "<H", 6),
        "a comment that leaves the directory": _poke(blob, layout[2]["central"] + 32, "<H", 1),
        "an entry on another disk": _poke(blob, layout[0]["central"] + 34, "<H", 1),
        "all-ones csize without a ZIP64 field": _poke(blob, layout[0]["central"] + 20, "<I", 0xffffffff),
        "all-ones offset without a ZIP64 field": _poke(blob, layout[0]["central"] + 42, "<I", 0xffffffff),
    }
    assert _status(_poke(blob, end + 16, "<I", dir_off - 1)) == 0  # (a smaller offset is a prefix of one byte: self-extracting archives)
    z, zl = _good(zip64_dir=True)
    x = zl[0]["central"] + 46 + 1  # entry 0's extra fields: 01 00 18 00 usize csize offset
    assert z[x:x + 4] == b"\1\0\x18\0"
    cases["a short ZIP64 field"] = _poke(z, x + 2, "<H", 16)
    cases["a ZIP64 field that leaves the extra fields"] = _poke(z, x + 2, "<H", 25)
    cases["another tag where the ZIP64 field was"] = _poke(z, x, "<H", 2)
    two = bytearray(z)
    for k in (0, 2):
        struct.pack_into("<Q", two, zl[k]["central"] + 46 + len(("a", "b/", "c.bin")[k]) + 4, 1 << 63)
    cases["a sum of sizes that overflows"] = two
    assert _status(_poke(z, zl[0]["central"] + 46 + 1 + 4, "<Q", 1 << 63)) == 0  # (one such size alone is only large)
    e64, _ = _good(zip64_end=True)
    loc = len(e64) - 22 - 20
    rec = loc - 56
    assert e64[loc:loc + 4] == zu.SIG_LOC64 and e64[rec:rec + 4] == zu.SIG_END64
    cases["a locator without its record"] = _poke(e64, rec, "<I", 0x06064b51)
    cases["a ZIP64 record with extensible data"] = _poke(e64, rec + 4, "<Q", 45)
    cases["a ZIP64 record on another disk"] = _poke(e64, rec + 16, "<I", 1)
    cases["a locator that names another disk"] = _poke(e64, loc + 4, "<I", 1)
    cases["a locator of two disks"] = _poke(e64, loc + 16, "<I", 2)
    cases["a disk number that is neither 0 nor all-ones"] = _poke(e64, len(e64) - 22 + 4, "<H", 7)
    cases["ZIP64 counts that differ"] = _poke(e64, rec + 24, "<Q", 2)
    cases["a locator with nothing in front"] = e64[loc:]
    for label, bad in cases.items():
        assert _status(bad) == BAD, label
    # and the end record's own fields are not looked at when the ZIP64 record replaces them
    assert _status(_poke(e64, len(e64) - 22 + 16, "<I", 5)) == 0


def test_truncation_at_every_length():
    for blob in (_good(comment=b"xyz")[0], _good(zip64_end=True, zip64_dir=True, prefix=b"stub")[0]):
        for n in range(len(blob)):
            assert _status(blob[:n]) in (BAD, 0), n
        assert sum(_status(blob[:n]) == BAD for n in range(len(blob))) >= len(blob) - 2


def test_misuse_refused_without_device():
    lib = _lib.load()
    blob = bytes(_good()[0])
    info, res, w = _lib.ZipInfo(), _lib.ZipResult(), ctypes.c_size_t()
    ents = (_lib.ZipEntry * 4)()
    assert lib.md_zip_directory(None, 0, ctypes.byref(info), None, 0) == -1
    assert lib.md_zip_directory(blob, len(blob), None, None, 0) == -1
    assert lib.md_zip_directory(blob, len(blob), ctypes.byref(info), None, 3) == -1
    assert lib.md_zip_directory(blob, len(blob), ctypes.byref(info), ents, 2) == 0 and info.entries == 3  # (cap below the count)
    assert ents[1].name_len == 2 and ents[2].name_len == 0
    dst = ctypes.create_string_buffer(64)
    off, st = (ctypes.c_uint64 * 4)(), (ctypes.c_int32 * 3)()
    assert lib.md_zip_uncompress(None, blob, len(blob), None, 0, dst, 64, off, st, ctypes.byref(res)) < 0
    src = _lib.ZipSource(b"n", 1, 0, 1, 0, 0, 0x21)
    assert lib.md_zip_compress(None, 6, 1, ctypes.byref(src), b"x", 1, dst, 64, ctypes.byref(w)) < 0


def test_compress_bound_formula():
    lib = _lib.load()
    for files in ([], [("a", b"")], [("name", b"x" * 1000), ("é", b"yy")], [("n%d" % k, bytes(k)) for k in range(300)]):
        want = sum(76 + 2 * len(n.encode("utf-8")) + len(d) for n, d in files) + 98
        assert zp.compress_bound(files) == want
    one = lambda name_len, length: lib.md_zip_compress_bound(1, ctypes.byref(_lib.ZipSource(b"n" * min(name_len, 8), name_len, 0, length, 0, 0, 0)))
    assert one(0, 5) == 0 and one(0x10000, 5) == 0 and one(0xffff, 5) == 76 + 2 * 0xffff + 5 + 98
    assert one(1, (1 << 64) - 1) == 0  # (a sum that does not fit)
    assert lib.md_zip_compress_bound(1, None) == 0 and lib.md_zip_compress_bound(0, None) == 98


def test_new_kernels_use_no_scratch(tmp_path):
    build.build()
    kernels = _all_kernel_metadata(_lib.SO, tmp_path)
    mine = {k: v for k, v in kernels.items() if "2md3zip" in k}  # namespace md::zip
    for want in KERNELS:
        assert any(want in k for k in mine), (want, sorted(mine))
    assert len(mine) == len(KERNELS), sorted(mine)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0, (name, k)


def test_zp_directory_refuses_what_is_no_archive():
    from decompress_amd import engine
    for blob in (b"", b"PK", bytes(100), b"PK\3\4" + bytes(60)):
        with pytest.raises(engine.Error, match="Invalid ZIP directory"):
            zp.directory(blob)
