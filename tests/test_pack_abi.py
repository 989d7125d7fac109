"""CPU-side checks of the packfile entry points (md_pack_*): declared, exported and bound; the five statuses and
their strings; md_pack_index over the index family against the model of tests/pack_model.py, field by field; misuse refused
without a device."""
import ctypes
import os
import re

import pytest

from decompress_amd import _lib, build, engine
from decompress_amd import pack as mp
from tests import pack_cases as pc
from tests import pack_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ["md_pack_index", "md_pack_open", "md_pack_get", "md_pack_objects", "md_pack_find", "md_pack_free", "md_pack_read", "md_pack_last"]
STRINGS = {22: "Invalid pack", 23: "Invalid delta", 24: "Invalid delta base", 25: "Missing delta base", 26: "Unsupported pack"}


def test_declared_exported_bound():
    build.build()
    assert "pack_kernels.hip" in build.SOURCES and "capi_pack.cpp" in build.SOURCES
    for f in ("pack_kernels.hip", "capi_pack.cpp", "pack_index.hpp"):
        assert os.path.exists(os.path.join(build.CSRC, f)), f
    hdr = open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    so = ctypes.CDLL(_lib.SO)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert hasattr(so, f), f
        assert f in bound, f
    for s in ("md_pack_index_entry", "md_pack_index_info", "md_pack_info", "md_pack_object", "md_pack_result", "md_pack_stats", "MD_PACK_VERIFY_CRC",
              "pack_workspace", "MD_INVALID_PACK = 22", "MD_INVALID_DELTA = 23", "MD_INVALID_PACK_BASE = 24", "MD_PACK_MISSING_BASE = 25",
              "MD_PACK_UNSUPPORTED = 26"):
        assert s in hdr, s
    assert ctypes.sizeof(_lib.PackIndexEntry) == 32 and ctypes.sizeof(_lib.PackIndexInfo) == 32
    assert ctypes.sizeof(_lib.PackObject) == 64 and ctypes.sizeof(_lib.PackInfo) == 40 and ctypes.sizeof(_lib.PackStats) == 48
    assert ctypes.sizeof(_lib.PackResult) == 2 * ctypes.sizeof(ctypes.c_size_t) + 8
    lib = _lib.load()
    for k, s in STRINGS.items():
        assert lib.md_status_string(k) == s.encode() and engine.STATUS_NAMES[k] == s and engine.STATUS_CODES[s] == k
    assert lib.md_status_string(27) == b"Unknown status"
    assert (pm.INVALID_PACK, pm.INVALID_DELTA, pm.INVALID_PACK_BASE, pm.MISSING_BASE, pm.UNSUPPORTED) == tuple(STRINGS)


def test_index_family_equals_the_model():
    lib = _lib.load()
    cases, pack, layout = pc.index_cases()
    for label, blob, want in cases:
        info = _lib.PackIndexInfo()
        assert lib.md_pack_index(blob, len(blob), ctypes.byref(info), None, 0) == want == pm.read_idx(blob)[0], label
        if want != 0:
            with pytest.raises(engine.Error, match=engine.STATUS_NAMES[want]):
                mp.index(blob)
            continue
        ents, got = mp.index(blob)
        _, went, winfo = pm.read_idx(blob)
        assert got == {"n": winfo["n"], "has_64bit_table": winfo["has64"], "pack_checksum": winfo["pack_checksum"]}, label
        assert [(e["name"], e["offset"], e["crc32"]) for e in ents] == went, label
        assert got["pack_checksum"] == pack[-20:] and sorted(e["offset"] for e in ents) == [x["offset"] for x in layout]


def test_every_truncation_is_refused():
    lib = _lib.load()
    good = pc.index_cases()[0][0][1]
    info = _lib.PackIndexInfo()
    for n in range(len(good)):
        assert lib.md_pack_index(good[:n], n, ctypes.byref(info), None, 0) == pm.INVALID_INDEX, n


def test_misuse_refused_without_device():
    lib = _lib.load()
    good = pc.index_cases()[0][0][1]
    info = _lib.PackIndexInfo()
    ents = (_lib.PackIndexEntry * 40)()
    assert lib.md_pack_index(None, 0, ctypes.byref(info), None, 0) == -1
    assert lib.md_pack_index(good, len(good), None, None, 0) == -1
    assert lib.md_pack_index(good, len(good), ctypes.byref(info), None, 3) == -1
    ents[2].offset = 77
    assert lib.md_pack_index(good, len(good), ctypes.byref(info), ents, 2) == 0 and info.n == 40  # (cap below the count)
    assert ents[1].offset >= 12 and ents[2].offset == 77
    h = ctypes.c_void_p()
    assert lib.md_pack_open(None, b"PACK", 4, good, len(good), ctypes.byref(h)) < 0 and not h.value
    pinfo, stats, res = _lib.PackInfo(), _lib.PackStats(), _lib.PackResult()
    assert lib.md_pack_get(None, ctypes.byref(pinfo)) == -1 and lib.md_pack_objects(None, None, 0) == -1
    assert lib.md_pack_find(None, bytes(20)) == -1
    assert lib.md_pack_last(None, ctypes.byref(stats)) == -1
    off, st = (ctypes.c_uint64 * 2)(), (ctypes.c_int32 * 1)()
    assert lib.md_pack_read(None, None, b"x", 1, None, 0, 0, None, 0, off, st, ctypes.byref(res)) < 0
    lib.md_pack_free(None)
