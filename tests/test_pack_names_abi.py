"""CPU-side checks of the names entry points (md_sha1_batch_*, md_sha1_last, md_pack_verify, md_pack_check_trailers; DESIGN
4j): declared, exported and bound; MD_PACK_VERIFY_NAME is 2 and no status was added; misuse refused without a device; and
md_pack_check_trailers - which runs on the host - over the pack git wrote and the writer's packs, against hashlib."""
import ctypes
import hashlib
import os
import re

import pytest

from decompress_amd import _lib, build, engine
from decompress_amd import pack as mp
from tests import pack_cases as pc
from tests import pack_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "git_pack")
FUNCS = ["md_sha1_batch_device", "md_sha1_batch_host", "md_sha1_last", "md_pack_verify", "md_pack_check_trailers"]
STRINGS = {22: "Invalid pack", 23: "Invalid delta", 24: "Invalid delta base", 25: "Missing delta base", 26: "Unsupported pack", 27: "Unknown status"}


def _golden():
    with open(os.path.join(GOLDEN, "git.pack"), "rb") as f:
        pack = f.read()
    with open(os.path.join(GOLDEN, "git.idx"), "rb") as f:
        return pack, f.read()


def test_declared_exported_bound():
    build.build()
    assert "sha1_kernels.hip" in build.SOURCES and "capi_sha1.cpp" in build.SOURCES
    for f in ("sha1_kernels.hip", "capi_sha1.cpp", "sha1_host.hpp"):
        assert os.path.exists(os.path.join(build.CSRC, f)), f
    hdr = open(os.path.join(ROOT, "include", "mdeflate.h")).read()
    so = ctypes.CDLL(_lib.SO)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, hdr), f
        assert hasattr(so, f), f
        assert f in bound, f
    assert re.search(r"#define\s+MD_PACK_VERIFY_NAME\s+2u", hdr) and re.search(r"#define\s+MD_PACK_VERIFY_CRC\s+1u", hdr)
    assert mp.VERIFY_NAMES == 2 and mp.VERIFY_CRC == 1
    assert "md_sha1_stats" in hdr and ctypes.sizeof(_lib.Sha1Stats) == 32 and ctypes.sizeof(_lib.PackStats) == 48
    assert "Out of scope: hashing" not in hdr
    # the option's default, said once in each place
    assert '"sha1_launch_blocks"         1 .. 2^24 (default %d)' % engine.SHA1_LAUNCH_BLOCKS in hdr
    internal = open(os.path.join(build.CSRC, "internal.hpp")).read()
    assert "kLaunchBlocksDefault = %d" % engine.SHA1_LAUNCH_BLOCKS in internal
    # the header's formatter is plain C++ with no HIP in it
    text = open(os.path.join(build.CSRC, "sha1_host.hpp")).read()
    assert "#include <hip" not in text and "__host__ __device__" in text


def test_no_new_status():
    lib = _lib.load()
    for k, s in STRINGS.items():
        assert lib.md_status_string(k) == s.encode(), k
    assert 27 not in engine.STATUS_NAMES and max(engine.STATUS_NAMES) == 26


def test_misuse_refused_without_device():
    lib = _lib.load()
    one, digest, stats, res = (ctypes.c_uint64 * 1)(0), (ctypes.c_uint8 * 20)(), _lib.Sha1Stats(), _lib.PackResult()
    five = (ctypes.c_uint8 * 1)(5)
    assert lib.md_sha1_batch_host(None, 1, b"x", 1, one, one, None, digest) == -1
    assert lib.md_sha1_batch_host(None, 1, b"x", 1, one, one, five, digest) == -1
    assert lib.md_sha1_batch_host(None, 0, None, 0, None, None, None, None) == -1
    assert lib.md_sha1_batch_device(None, 1, None, None, None, None, 0, None) == -1
    assert lib.md_sha1_last(None, ctypes.byref(stats)) == -1
    st = (ctypes.c_int32 * 1)()
    assert lib.md_pack_verify(None, None, b"x", 1, None, 0, 2, st, ctypes.byref(res)) == -1
    pack, idx = _golden()
    ok = ctypes.c_int(7)
    assert lib.md_pack_check_trailers(None, len(pack), idx, len(idx), ctypes.byref(ok), ctypes.byref(ok)) == -1
    assert lib.md_pack_check_trailers(pack, len(pack), None, len(idx), ctypes.byref(ok), ctypes.byref(ok)) == -1
    assert lib.md_pack_check_trailers(pack, len(pack), idx, len(idx), None, ctypes.byref(ok)) == -1
    assert lib.md_pack_check_trailers(pack, len(pack), idx, len(idx), ctypes.byref(ok), None) == -1
    assert ok.value == 7


def _flip(b, at):
    return b[:at] + bytes([b[at] ^ 0x40]) + b[at + 1:]


def test_check_trailers():
    pack, idx = _golden()
    assert hashlib.sha1(pack[:-20]).digest() == pack[-20:] and hashlib.sha1(idx[:-20]).digest() == idx[-20:]
    assert mp.check_trailers(pack, idx) == (True, True)
    assert mp.check_trailers(_flip(pack, len(pack) // 2), idx) == (False, True)
    assert mp.check_trailers(pack, _flip(idx, 1032 + 7)) == (True, False)
    assert mp.check_trailers(_flip(pack, len(pack) - 1), _flip(idx, len(idx) - 20)) == (False, False)  # the trailers themselves
    assert mp.check_trailers(_flip(pack, 0), _flip(idx, 0)) == (False, False)  # (no word on what the files are: the bytes alone)
    for case in pc.cases():
        c = pc.build(case)
        want = (hashlib.sha1(c["pack"][:-20]).digest() == c["pack"][-20:], hashlib.sha1(c["idx"][:-20]).digest() == c["idx"][-20:])
        assert mp.check_trailers(c["pack"], c["idx"]) == want == (True, True), c["name"]
    empty = pc.build([c for c in pc.cases() if c["name"] == "an empty pack"][0])
    assert len(empty["pack"]) == 32 and len(empty["idx"]) == 8 + 1024 + 40
    lib = _lib.load()
    a, b = ctypes.c_int(7), ctypes.c_int(7)
    for cut in (0, 1, 31):
        assert lib.md_pack_check_trailers(empty["pack"][:cut], cut, empty["idx"], len(empty["idx"]), ctypes.byref(a), ctypes.byref(b)) == pm.INVALID_PACK
    for cut in (0, 8, 8 + 1024 + 39):
        assert lib.md_pack_check_trailers(empty["pack"], 32, empty["idx"][:cut], cut, ctypes.byref(a), ctypes.byref(b)) == pm.INVALID_INDEX
    assert lib.md_pack_check_trailers(empty["pack"][:31], 31, empty["idx"][:8], 8, ctypes.byref(a), ctypes.byref(b)) == pm.INVALID_INDEX
    assert (a.value, b.value) == (7, 7)
    with pytest.raises(engine.Error, match="Invalid pack"):
        mp.check_trailers(pack[:20], idx)
    with pytest.raises(engine.Error, match="Invalid index"):
        mp.check_trailers(pack, idx[:100])
