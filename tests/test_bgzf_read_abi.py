"""CPU-side checks of random access to blocked GZip (md_bgzf_index_*, md_bgzf_read*; csrc/bgzf_index.hpp, capi_bgzf_read.cpp,
bgzf_read.hip): declared, exported and bound; .gzi blobs written with struct.pack load against files written with zlib and
struct alone and give the expected table, with and without an entry for the EOF marker; to_gzi / from_gzi round-trip; each
rule of the blob broken alone; misuse refused without a device; the new kernels use no scratch."""
import ctypes
import os
import re
import struct

from decompress_amd import _lib, build
from tests import gz_members_util as gu
from tests.test_inf_batch_abi import _all_kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["md_bgzf_index_build", "md_bgzf_index_from_gzi", "md_bgzf_index_gzi_size", "md_bgzf_index_to_gzi", "md_bgzf_index_get",
         "md_bgzf_index_entries", "md_bgzf_index_free", "md_bgzf_read", "md_bgzf_read_virtual", "md_bgzf_read_last"]
KERNELS = ["verdict_kernel", "gather_kernel"]
BAD, SHORT = 21, 2  # MD_INVALID_INDEX, MD_UNEXPECTED_END_OF_OUTPUT
TEXT = b"".join(b"line %d of the file, with some words in it\n" % k for k in range(700))


def gzi(pairs):
    return struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", c, u) for c, u in pairs)


def _load(blob, src):
    """(status, handle)"""
    h = ctypes.c_void_p()
    st = _lib.load().md_bgzf_index_from_gzi(bytes(blob), len(blob), bytes(src), len(src), ctypes.byref(h))
    assert (st == 0) == bool(h.value)
    return st, h


def _status(blob, src):
    st, h = _load(blob, src)
    _lib.load().md_bgzf_index_free(h)
    return st


def _entries(h):
    lib = _lib.load()
    info = _lib.BgzfIndexInfo()
    assert lib.md_bgzf_index_get(h, ctypes.byref(info)) == 0
    n = info.members + 1
    c, u = (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)()
    assert lib.md_bgzf_index_entries(h, c, u, n) == 0
    return info, list(zip(c, u))


def _to_gzi(h):
    lib = _lib.load()
    n = lib.md_bgzf_index_gzi_size(h)
    buf, got = ctypes.create_string_buffer(b"\xa5" * (n + 1), n + 1), ctypes.c_size_t()
    assert lib.md_bgzf_index_to_gzi(h, buf, n, ctypes.byref(got)) == 0 and got.value == n
    assert buf.raw[n:] == b"\xa5"
    return buf.raw[:n]


def test_declared_exported_bound():
    build.build()
    for f in ("bgzf_read.hip", "capi_bgzf_read.cpp"):
        assert f in build.SOURCES and os.path.exists(os.path.join(build.CSRC, f))
    hdr = open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    so = ctypes.CDLL(_lib.SO)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert hasattr(so, f), f
        assert f in bound, f
    for s in ("md_bgzf_index_info", "md_bgzf_read_stats", "bgzf_read_workspace"):
        assert s in hdr
    assert ctypes.sizeof(_lib.BgzfIndexInfo) == 3 * 8
    assert ctypes.sizeof(_lib.BgzfReadStats) == 4 * 8
    assert _lib.load().md_version() == 0x000300
    from decompress_amd import gz
    for m in ("build", "from_gzi", "to_gzi", "info", "entries", "read_many", "read", "read_virtual_many", "last_stats"):
        assert callable(getattr(gz.BgzfIndex, m)), m
    # bgzf_index.hpp is the host's alone
    txt = open(os.path.join(build.CSRC, "bgzf_index.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", txt).lower()


def test_hand_written_gzi_loads_with_and_without_the_eof_entry():
    for block, eof in ((0xff00, True), (4096, True), (300, True), (4096, False)):
        f, idx = gu.bgzf_file(TEXT, block=block, eof=eof)
        want = idx + [(len(f), len(TEXT))]  # the M + 1 pairs
        assert gu.walk_bsize(f) == ([c for c, _ in idx], len(f))
        last = len(idx) - (2 if eof else 1)  # the last member with bytes
        for listed in {len(idx), last + 1, last} - {0}:  # every member; without the EOF marker; without the last member too
            st, h = _load(gzi(idx[1:listed]), f)
            assert st == 0, (block, eof, listed)
            info, got = _entries(h)
            assert (info.src_len, info.members, info.size) == (len(f), len(idx), len(TEXT))
            assert got == want, (block, eof, listed)
            # to_gzi lists members 1 .. M - 1, whatever the blob it came from listed; and loads to the same table
            blob = _to_gzi(h)
            assert blob == gzi(idx[1:])
            _lib.load().md_bgzf_index_free(h)
            st, h = _load(blob, f)
            assert st == 0 and _entries(h)[1] == want and _to_gzi(h) == blob
            _lib.load().md_bgzf_index_free(h)


def test_small_indexes():
    lib = _lib.load()
    # an empty file: 0 members; one member: count 0, and the walk finds it
    for f, idx, size in ((b"", [], 0), (gu.EOF_MARKER, [(0, 0)], 0), gu.bgzf_file(b"abc", eof=False) + (3,), gu.bgzf_file(b"abc") + (3,)):
        st, h = _load(gzi([]), f)
        assert st == 0
        info, got = _entries(h)
        assert (info.src_len, info.members, info.size) == (len(f), len(idx), size)
        assert got == idx + [(len(f), size)]
        assert _to_gzi(h) == gzi(idx[1:])
        got_len, one = ctypes.c_size_t(), (ctypes.c_uint64 * 1)()
        if len(idx) > 1:
            assert lib.md_bgzf_index_to_gzi(h, ctypes.create_string_buffer(8), 8, ctypes.byref(got_len)) == SHORT and got_len.value == 24
        assert lib.md_bgzf_index_entries(h, one, one, 1) == 0 and one[0] == 0
        lib.md_bgzf_index_free(h)
    # empty members in the middle are ordinary entries
    f, idx = gu.bgzf_of_members([b"ab", b"", b"", b"cde", b""])
    st, h = _load(gzi(idx[1:]), f)
    assert st == 0 and _entries(h)[1] == idx + [(len(f), 5)]
    lib.md_bgzf_index_free(h)


def test_each_rule_broken_alone():
    f, idx = gu.bgzf_file(TEXT, block=4096)
    good = idx[1:]
    assert _status(gzi(good), f) == 0
    c3, u3 = good[2]
    inside = good[:2] + [(c3 + 5, u3)] + good[3:]  # (still ascending; the walk never looks at it: the read does)
    assert _status(gzi(inside), f) == 0
    cases = {
        "a byte short": (gzi(good)[:-1], f),
        "a trailing byte": (gzi(good) + b"\0", f),
        "one entry more than the count says": (gzi(good) + bytes(16), f),
        "one entry fewer than the count says": (struct.pack("<Q", len(good) + 1) + gzi(good)[8:], f),
        "a count that would need 2^64 bytes": (struct.pack("<Q", (1 << 60) + 1) + gzi(good)[8:], f),
        "no count": (b"\1\0\0", f),
        "empty": (b"", f),
        "compressed offsets repeat": (gzi(good[:2] + [good[1]] + good[2:]), f),
        "compressed offsets fall": (gzi([good[1], good[0]] + good[2:]), f),
        "a first entry at 0": (gzi([(0, 0)] + good), f),
        "an offset at src_len": (gzi(good + [(len(f), len(TEXT))]), f),
        "an offset behind src_len": (gzi(good[:-1] + [(len(f) + 7, len(TEXT))]), f),
        "uncompressed offsets fall": (gzi(good[:1] + [(good[1][0], good[0][1] - 1)] + good[2:]), f),
        "more output than DEFLATE can make": (gzi(good[:1] + [(good[1][0], good[1][1] + (1 << 40))]), f),
        "the last entry stands inside a member": (gzi(good[:-1] + [(good[-1][0] - 3, good[-1][1])]), f),
        "the last entry stands on no member (count 0, a file that begins with a NUL)": (gzi([]), b"\0" + f),
        "a file cut inside the EOF marker": (gzi(good), f[:-1]),
        "a file cut inside the last member with bytes": (gzi(good[:-1]), f[:good[-1][0] - 1]),
        "bytes that are no member behind the last": (gzi(good), f + b"x"),
        "padding that does not reach the end": (gzi(good), f + b"\0\0x"),
        "a member without the BC field at the last entry": (gzi([(len(f), len(TEXT))]), f + gu.member(b"tail")),
    }
    for label, (blob, src) in cases.items():
        assert _status(blob, src) == BAD, label
    # NUL padding behind the last member is accepted, and c_off[M] stays the byte behind the member
    for pad in (1, 7, 512):
        st, h = _load(gzi(good), f + bytes(pad))
        assert st == 0
        info, got = _entries(h)
        assert info.src_len == len(f) + pad and got == idx + [(len(f), len(TEXT))]
        _lib.load().md_bgzf_index_free(h)


def test_misuse_refused_without_device():
    lib = _lib.load()
    f, idx = gu.bgzf_file(TEXT, block=4096)
    blob = gzi(idx[1:])
    st, h = _load(blob, f)
    assert st == 0
    x = ctypes.c_void_p(1)
    assert lib.md_bgzf_index_from_gzi(None, 8, f, len(f), ctypes.byref(x)) == -1 and not x.value
    assert lib.md_bgzf_index_from_gzi(blob, len(blob), None, len(f), ctypes.byref(x)) == -1
    assert lib.md_bgzf_index_from_gzi(blob, len(blob), f, len(f), None) == -1
    assert lib.md_bgzf_index_from_gzi(None, 0, f, len(f), ctypes.byref(x)) == BAD  # (an empty blob is only invalid)
    info, stats, got = _lib.BgzfIndexInfo(), _lib.BgzfReadStats(), ctypes.c_size_t()
    assert lib.md_bgzf_index_get(None, ctypes.byref(info)) == -1 and lib.md_bgzf_index_get(h, None) == -1
    assert lib.md_bgzf_index_entries(None, None, None, 0) == -1 and lib.md_bgzf_index_entries(h, None, None, 1) == -1
    assert lib.md_bgzf_index_entries(h, None, None, 0) == 0
    big = (ctypes.c_uint64 * (len(idx) + 5))()  # (cap beyond M + 1: the M + 1 there are)
    assert lib.md_bgzf_index_entries(h, big, big, len(idx) + 5) == 0 and big[len(idx)] == len(TEXT) and big[len(idx) + 1] == 0
    assert lib.md_bgzf_index_gzi_size(None) == 0 and lib.md_bgzf_index_gzi_size(h) == len(blob)
    buf = ctypes.create_string_buffer(len(blob))
    assert lib.md_bgzf_index_to_gzi(None, buf, len(blob), ctypes.byref(got)) == -1
    assert lib.md_bgzf_index_to_gzi(h, buf, len(blob), None) == -1 and lib.md_bgzf_index_to_gzi(h, None, len(blob), ctypes.byref(got)) == -1
    assert lib.md_bgzf_index_to_gzi(h, buf, len(blob) - 1, ctypes.byref(got)) == SHORT and got.value == len(blob)
    assert lib.md_bgzf_index_to_gzi(h, None, 0, ctypes.byref(got)) == SHORT and got.value == len(blob)
    assert lib.md_bgzf_read_last(None, ctypes.byref(stats)) == -1
    lib.md_bgzf_index_free(None)
    # build and the reads need a context: a call-level error, and no index comes back
    x = ctypes.c_void_p(1)
    assert lib.md_bgzf_index_build(None, f, len(f), ctypes.byref(x)) < 0 and not x.value
    assert lib.md_bgzf_index_build(None, f, len(f), None) < 0
    off, ln, st32 = (ctypes.c_uint64 * 1)(0), (ctypes.c_uint64 * 1)(1), (ctypes.c_int32 * 1)()
    assert lib.md_bgzf_read(None, h, f, len(f), 1, off, ln, buf, off, st32) < 0
    assert lib.md_bgzf_read_virtual(None, h, f, len(f), 1, off, ln, buf, off, st32) < 0
    lib.md_bgzf_index_free(h)


def test_new_kernels_use_no_scratch(tmp_path):
    build.build()
    kernels = _all_kernel_metadata(_lib.SO, tmp_path)
    mine = {k: v for k, v in kernels.items() if "2md3bgr" in k}  # namespace md::bgr
    for want in KERNELS:
        assert any(want in k for k in mine), (want, sorted(mine))
    assert len(mine) == len(KERNELS), sorted(mine)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["group_segment_fixed_size"] == 0, (name, k)
