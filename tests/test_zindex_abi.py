"""CPU-side checks of the inflate index (md_inflate_index_*; csrc/zindex.hpp, capi_zindex.cpp, zindex_kernels.hip): declared,
exported and bound; a blob written with struct.pack from the header's description loads, answers with its fields and is
saved back byte for byte; each rule of the layout broken alone; truncations; misuse refused without a device; the new
kernels use no scratch."""
import ctypes
import os
import re
import struct

from decompress_amd import _lib, build
from tests import zindex_blob as zb
from tests.test_inf_batch_abi import _all_kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["md_inflate_index_build", "md_inflate_index_get", "md_inflate_index_points", "md_inflate_index_save_size",
         "md_inflate_index_save", "md_inflate_index_load", "md_inflate_index_free", "md_inflate_index_read", "md_inflate_index_last"]
KERNELS = ["windows_take_kernel", "plan_kernel", "windows_put_kernel", "verdict_kernel", "gather_kernel"]
BAD = 21  # MD_INVALID_INDEX


def test_declared_exported_bound():
    build.build()
    for f in ("zindex_kernels.hip", "capi_zindex.cpp"):
        assert f in build.SOURCES and os.path.exists(os.path.join(build.CSRC, f))
    hdr = open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    so = ctypes.CDLL(_lib.SO)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert hasattr(so, f), f
        assert f in bound, f
    for s in ("md_inflate_index_info", "md_inflate_index_stats", "index_read_workspace", "MD_INVALID_INDEX = 21"):
        assert s in hdr
    assert ctypes.sizeof(_lib.InflateIndexInfo) == 4 + 4 + 6 * 8
    assert ctypes.sizeof(_lib.InflateIndexStats) == 5 * 8
    lib = _lib.load()
    assert lib.md_version() == 0x000300
    assert lib.md_status_string(21) == b"Invalid index"
    from decompress_amd import engine
    assert engine.STATUS_NAMES[21] == "Invalid index"
    # zindex.hpp is the host's alone
    txt = open(os.path.join(build.CSRC, "zindex.hpp")).read()
    assert "hip" not in re.sub(r"//.*", "", txt).lower()


def _load(blob):
    """(status, handle)"""
    lib = _lib.load()
    h = ctypes.c_void_p()
    st = lib.md_inflate_index_load(bytes(blob), len(blob), ctypes.byref(h))
    assert (st == 0) == bool(h.value)
    return st, h


def _status(blob):
    st, h = _load(blob)
    _lib.load().md_inflate_index_free(h)
    return st


def test_hand_written_blob_loads_and_is_saved_back():
    lib = _lib.load()
    points = ((16, 0), (9000, 4096), (20001, 12300), (39000, 60000))
    for kw in (dict(), dict(fmt=0, header_len=0, points=((0, 0),), size=0), dict(fmt=2, header_len=18, points=((144, 0), (900, 5000))),
               dict(points=points, size=60000), dict(points=points, size=60001, consumed=5000, src_len=1 << 40)):
        blob = zb.blob(**kw)
        st, h = _load(blob)
        assert st == 0, kw
        info = _lib.InflateIndexInfo()
        assert lib.md_inflate_index_get(h, ctypes.byref(info)) == 0
        want = dict(fmt=1, src_len=5000, header_len=2, consumed=4990, size=20000, span=4096, checksum=0x1234abcd,
                    points=((16, 0), (9000, 4096), (20001, 12300)))
        want.update(kw)
        assert (info.format, info.src_len, info.header_len, info.consumed, info.size, info.span, info.checksum, info.points) == \
               (want["fmt"], want["src_len"], want["header_len"], want["consumed"], want["size"], want["span"], want["checksum"], len(want["points"]))
        n = len(want["points"])
        bit, out = (ctypes.c_uint64 * (n + 1))(), (ctypes.c_uint64 * (n + 1))()
        assert lib.md_inflate_index_points(h, bit, out, n + 1) == 0
        assert list(zip(bit, out))[:n] == [tuple(p) for p in want["points"]] and (bit[n], out[n]) == (0, 0)
        assert lib.md_inflate_index_points(h, bit, out, 1) == 0 and lib.md_inflate_index_points(h, None, None, 0) == 0
        assert lib.md_inflate_index_save_size(h) == len(blob)
        buf, got = ctypes.create_string_buffer(b"\xa5" * (len(blob) + 1), len(blob) + 1), ctypes.c_size_t()
        assert lib.md_inflate_index_save(h, buf, len(blob), ctypes.byref(got)) == 0 and got.value == len(blob)
        assert buf.raw == blob + b"\xa5"
        assert lib.md_inflate_index_save(h, buf, len(blob) - 1, ctypes.byref(got)) == 2 and got.value == len(blob)
        lib.md_inflate_index_free(h)


def test_each_rule_broken_alone():
    assert _status(zb.blob()) == 0
    pts = [(16, 0), (9000, 4096), (20001, 12300)]
    cases = {
        "magic": b"MDZINDEY" + zb.blob()[8:],
        "version": zb.blob(version=2),
        "the zero word of the head": zb.blob(zero=1),
        "the zero word of a point": zb.blob(point_zero=1),
        "format": zb.blob(fmt=3),
        "a raw stream with a header": zb.blob(fmt=0),
        "a ZLIB header of 3 bytes": zb.blob(header_len=3, points=[(24, 0)] + pts[1:]),
        "a GZip header of 9 bytes": zb.blob(fmt=2, header_len=9, points=[(72, 0)] + pts[1:]),
        "consumed beyond src": zb.blob(consumed=5001),
        "no room for the trailer": zb.blob(consumed=5, points=[(16, 0)], size=1),
        "src_len of 2^60": zb.blob(src_len=1 << 60),
        "span below 4096": zb.blob(span=4095),
        "no points": zb.blob(points=[]),
        "point 0 is not the first block": zb.blob(points=[(17, 0)] + pts[1:]),
        "point 0 has output in front": zb.blob(points=[(16, 1)] + pts[1:]),
        "bits do not increase": zb.blob(points=[pts[0], (9000, 4096), (9000, 12300)]),
        "outs do not increase": zb.blob(points=[pts[0], (9000, 4096), (20001, 4096)]),
        "a window shorter than min(32768, out)": zb.blob(win_lens=[0, 4095, 12300]),
        "a window longer than min(32768, out)": zb.blob(win_lens=[0, 4097, 12300]),
        "a window of 32769": zb.blob(points=pts + [(30000, 50000)], size=60000, win_lens=[0, 4096, 12300, 32769]),
        "a bit in the trailer": zb.blob(points=pts[:2] + [(8 * 4986, 12300)]),
        "a bit behind the stream": zb.blob(points=pts[:2] + [(8 * 4990, 12300)]),
        "out beyond size": zb.blob(size=12299),
        "out == size in the middle": zb.blob(size=4096, points=pts[:2] + [(20001, 4097)]),
        "a trailing byte": zb.blob() + b"\0",
        "a byte short": zb.blob()[:-1],
        "one point more than the table holds": zb.blob(npoints=4),
        "one point fewer": zb.blob(npoints=2),
        "a count that would need 2^64 bytes": zb.blob(npoints=(1 << 64) // 24 + 1),
    }
    assert _status(zb.blob(size=12300)) == 0  # (the last point may be an empty block at the very end)
    assert _status(zb.blob(points=pts[:2] + [(8 * 4986 - 1, 12300)])) == 0  # (the last bit of the body)
    for label, bad in cases.items():
        assert _status(bad) == BAD, label


def test_truncation_at_every_length():
    blob = zb.blob()
    assert all(_status(blob[:n]) == BAD for n in range(len(blob)))
    assert _status(b"") == BAD


def test_misuse_refused_without_device():
    lib = _lib.load()
    blob = zb.blob()
    st, h = _load(blob)
    info, stats, got = _lib.InflateIndexInfo(), _lib.InflateIndexStats(), ctypes.c_size_t()
    x = ctypes.c_void_p()
    assert lib.md_inflate_index_load(None, 5, ctypes.byref(x)) == -1 and lib.md_inflate_index_load(blob, len(blob), None) == -1
    assert lib.md_inflate_index_load(None, 0, ctypes.byref(x)) == BAD  # (an empty blob is only invalid)
    assert lib.md_inflate_index_get(None, ctypes.byref(info)) == -1 and lib.md_inflate_index_get(h, None) == -1
    assert lib.md_inflate_index_points(None, None, None, 0) == -1 and lib.md_inflate_index_points(h, None, None, 1) == -1
    assert lib.md_inflate_index_save_size(None) == 0
    buf = ctypes.create_string_buffer(len(blob))
    assert lib.md_inflate_index_save(None, buf, len(blob), ctypes.byref(got)) == -1
    assert lib.md_inflate_index_save(h, buf, len(blob), None) == -1 and lib.md_inflate_index_save(h, None, len(blob), ctypes.byref(got)) == -1
    assert lib.md_inflate_index_last(None, ctypes.byref(stats)) == -1
    lib.md_inflate_index_free(None)
    # build and read need a context: a call-level error, and no index comes back
    x = ctypes.c_void_p(1)
    assert lib.md_inflate_index_build(None, 1, b"x", 1, 0, None, 0, ctypes.byref(x), ctypes.byref(info)) < 0 and not x.value
    assert lib.md_inflate_index_build(None, 1, b"x", 1, 0, None, 0, None, None) < 0
    off, ln, st32 = (ctypes.c_uint64 * 1)(0), (ctypes.c_uint64 * 1)(1), (ctypes.c_int32 * 1)()
    assert lib.md_inflate_index_read(None, h, b"x" * 5000, 5000, 1, off, ln, buf, off, st32) < 0
    lib.md_inflate_index_free(h)


def test_new_kernels_use_no_scratch(tmp_path):
    build.build()
    kernels = _all_kernel_metadata(_lib.SO, tmp_path)
    mine = {k: v for k, v in kernels.items() if "2md3zix" in k}  # namespace md::zix
    for want in KERNELS:
        assert any(want in k for k in mine), (want, sorted(mine))
    assert len(mine) == len(KERNELS), sorted(mine)
    for name, k in mine.items():
        assert k["private_segment_fixed_size"] == 0, (name, k)
