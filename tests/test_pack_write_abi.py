"""CPU-side checks of the pack writer's entry points (md_pack_delta_batch_*, md_pack_write_bound, md_pack_write,
md_pack_write_last): declared, exported and bound; the structs have the sizes the header declares; the header's
constants are pack_write.hpp's and the model's; md_pack_write_bound - host arithmetic - matches the model; misuse is refused
without a device."""
import ctypes
import os
import re

from decompress_amd import _lib, build
from decompress_amd import pack as mp
from tests import pack_delta_model as dm
from tests import pack_write_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["md_pack_delta_batch_device", "md_pack_delta_batch_host", "md_pack_write_bound", "md_pack_write", "md_pack_write_last"]


def test_declared_exported_bound():
    build.build()
    for f in ("pack_write_kernels.hip", "capi_pack_write.cpp"):
        assert f in build.SOURCES and os.path.exists(os.path.join(build.CSRC, f)), f
    hdr = open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    so = ctypes.CDLL(_lib.SO)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert hasattr(so, f), f
        assert f in bound, f
    assert re.search(r"#define\s+MD_PACK_WRITE_NO_DELTA\s+1u", hdr) and mp.WRITE_NO_DELTA == 1
    for name, cls, size in (("md_pack_delta_pair", _lib.PackDeltaPair, 48), ("md_pack_source", _lib.PackSource, 32),
                            ("md_pack_write_result", _lib.PackWriteResult, 24), ("md_pack_write_stats", _lib.PackWriteStats, 64)):
        assert "} %s;" % name in hdr and ctypes.sizeof(cls) == size, name
    assert "Out of scope: writing packs" not in hdr
    # pack_write.hpp is plain C++ with no HIP in it, and its constants are the header's and the model's
    text = open(os.path.join(build.CSRC, "pack_write.hpp")).read()
    assert "#include <hip" not in text and "__device__" not in text
    assert "kBlock = %d, kHashMul = 0x%Xu, kMinBits = %d" % (dm.BLOCK, dm.MUL, dm.MIN_BITS) in text
    assert "kMaxInsert = %d, kMaxCopy = 0x%x" % (dm.MAX_INSERT, dm.MAX_COPY) in text
    assert "kDeltaMinTarget = %d, kDeltaSlack = %d" % (dm.DELTA_MIN_TARGET, dm.DELTA_SLACK) in text and "kHeaderMax = %d" % dm.HEADER_MAX in text
    assert "0x9E3779B1" in hdr and "len / 2 - 20" in hdr


def _sources(lens):
    src = (_lib.PackSource * max(len(lens), 1))()
    for s, n in zip(src, lens):
        s.off, s.len, s.base, s.type = 0, n, mp.NO_BASE, 3
    return src


def test_bound_matches_the_model():
    lib = _lib.load()
    for lens in ([], [0], [1], [7, 8, 9], [63, 64, 65, 1 << 20], [0xFFFFFFF0], [0xFFFFFFF0] * 5):
        assert lib.md_pack_write_bound(len(lens), _sources(lens)) == dm.write_bound(lens), lens
    assert lib.md_pack_write_bound(0, None) == 32
    assert lib.md_pack_write_bound(1, None) == 0
    assert lib.md_pack_write_bound(2, _sources([5, 0xFFFFFFF1])) == 0
    for c in wc.pack_cases():  # the bound holds for every pack of the model, at every level the tests write
        lens = [len(d) for _, d in c["objects"]]
        for r in wc.pack_model(c["name"], 6):
            assert len(r["pack"]) <= dm.write_bound(lens), c["name"]


def test_misuse_refused_without_device():
    lib = _lib.load()
    pair, src = (_lib.PackDeltaPair * 1)(), _sources([1])
    one64, one32, need = (ctypes.c_uint64 * 1)(), (ctypes.c_int32 * 1)(), ctypes.c_size_t(7)
    ents, res, stats = (_lib.PackIndexEntry * 1)(), _lib.PackWriteResult(), _lib.PackWriteStats()
    out = ctypes.create_string_buffer(64)
    assert lib.md_pack_delta_batch_host(None, 1, pair, b"x", 1, out, 64, one64, one32) == -1
    assert lib.md_pack_delta_batch_host(None, 0, None, None, 0, None, 0, None, None) == -1
    assert lib.md_pack_delta_batch_device(None, 1, pair, None, None, None, None) == -1
    assert lib.md_pack_write(None, 6, 0, 50, 1, src, b"x", 1, out, 64, ctypes.byref(need), ents, ctypes.byref(res)) == -1
    assert lib.md_pack_write(None, 6, 0, 50, 0, None, None, 0, out, 64, ctypes.byref(need), None, ctypes.byref(res)) == -1
    assert need.value == 7
    assert lib.md_pack_write_last(None, ctypes.byref(stats)) == -1
