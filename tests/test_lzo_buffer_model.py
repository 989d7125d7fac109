"""tests/lzo_buffer_model.py - the size-only reading of Lzo.uncompress_with_buffer that the size query's GPU tests are held
to - against the CPU oracle's Lzo.uncompress (oracle/lzo.c) given room that cannot run out: 256 x len + 512 bytes (a zero
byte of a length adds 255 bytes and every other byte of a stream adds less).  Lzo.uncompress has one error where
uncompress_with_buffer has two (`Invalid_dictionary and "Malformed input" are both its "Input is malformed or output is
not large enough"): with 4 and 17 mapped to 16, status and length agree on every stream."""
import ctypes
import mmap
import time

from tests import lzo_batches
from tests import lzo_buffer_model as model
from tests.conftest import golden_bytes, load_golden

SEEN = set()


def _oracle(oracle, src):
    """(status, length) of orc_lzo_uncompress with room 256 x len + 512: anonymous pages, touched only where written"""
    fn = oracle.lib.orc_lzo_uncompress
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    cap = 256 * len(src) + 512
    w = ctypes.c_size_t()
    with mmap.mmap(-1, cap) as room:
        buf = (ctypes.c_char * cap).from_buffer(room)
        rc = fn(bytes(src), len(src), ctypes.addressof(buf), cap, ctypes.byref(w))
        del buf
    return rc, w.value


def _hold(oracle, name, src):
    st, n = model.size(src)
    assert st in model.STATUSES and (st == model.OK or n == 0), (name, st, n)
    assert (model.as_uncompress(st), n) == _oracle(oracle, src), (name, st, n)
    SEEN.add(st)


def test_families(oracle):
    seen = set()
    for fam in lzo_batches.FAMILIES.values():
        for c in fam():
            if (id(c.b), len(c.stream)) in seen:
                continue
            seen.add((id(c.b), len(c.stream)))
            _hold(oracle, c.name, c.stream)
            if not c.b.malformed and c.b.ended and len(c.stream) == len(c.b.stream):
                assert model.size(c.stream) == (model.OK, len(c.b.out)), c.name


def test_reference_vectors(oracle):
    cases = load_golden("lzo.json")
    assert len(cases) == 34
    for c in cases:
        src = golden_bytes(c["src"])
        t0 = time.perf_counter()
        st, n = model.size(src)
        assert time.perf_counter() - t0 < 1.0, c["name"]  # (the zero runs of 8 - 17 MB: a scan, not a loop)
        _hold(oracle, c["name"], src)
        if c["status"] == 0:
            assert (st, n) == (model.OK, len(golden_bytes(c["out"]))), c["name"]
        else:
            assert st != model.OK, c["name"]
    assert sum(1 for c in cases if len(golden_bytes(c["src"])) > 4_000_000) == 3


def test_random_streams(oracle):
    streams = model.random_streams()
    assert len(streams) == 3000 and all(1 <= len(s) <= 59 for s in streams)
    for k, s in enumerate(streams):
        _hold(oracle, "random %d" % k, s)


def test_cut_stream(oracle):
    cuts = model.cut_streams()
    assert len(cuts) > 1000
    for k, s in enumerate(cuts):
        _hold(oracle, "cut at %d" % k, s)
    assert model.size(cuts[-1])[0] == model.OK and model.size(b"") == (model.END_OF_INPUT, 0)


def test_every_status_met(oracle):
    """over the four tests above (run here again when this test runs alone)"""
    if not SEEN:
        test_families(oracle), test_reference_vectors(oracle), test_random_streams(oracle), test_cut_stream(oracle)
    assert SEEN >= set(model.STATUSES), SEEN
