"""md_pack_index_write through ctypes (host arithmetic, no device): against pack_writer.write_idx - also with made-up
offsets at 0x7fffffff, 0x80000000 and 2^40, since no real pack reaches the 64-bit table in a test's time -, the round trip
through md_pack_index, equal names, a capacity one short, and no entries at all."""
import ctypes
import hashlib

from decompress_amd import _lib, build
from tests import pack_cases as pc
from tests import pack_model as pm
from tests import pack_writer as pw

END_OF_OUTPUT = 2


def _lib_():
    build.build()
    return _lib.load()


def _write(lib, entries, checksum, cap=None):
    """entries [(name, offset, crc)] -> (status, idx bytes, idx_len)"""
    n = len(entries)
    ents = (_lib.PackIndexEntry * max(n, 1))()
    for e, (name, off, crc) in zip(ents, entries):
        e.offset, e.crc32 = off, crc
        e.name[:] = name
    need = ctypes.c_size_t(0)
    if cap is None:
        assert lib.md_pack_index_write(ents, n, checksum, None, 0, ctypes.byref(need)) == END_OF_OUTPUT
        cap = need.value
    buf = ctypes.create_string_buffer(b"\xaa" * max(cap, 1), max(cap, 1))
    st = lib.md_pack_index_write(ents, n, checksum, buf, cap, ctypes.byref(need))
    return st, buf.raw[:cap], need.value


def _layout(offsets):
    return [{"name": hashlib.sha1(b"object %d" % k).digest(), "offset": off, "packed_len": 0} for k, off in enumerate(offsets)]


def test_against_the_writer_of_the_tests():
    lib = _lib_()
    checksum = hashlib.sha1(b"a pack").digest()
    for offsets in ([12], [12, 500, 90], list(range(12, 12 + 700 * 37, 37)), [12, 0x7fffffff, 0x80000000, 1 << 40, 77, (1 << 40) + 5, 0x7ffffffe]):
        layout = _layout(offsets)
        want = pw.write_idx(b"" * 20 + checksum, layout)  # (packed_len 0: every CRC is that of no bytes, 0)
        for order in (list(range(len(layout))), list(reversed(range(len(layout))))):
            st, got, need = _write(lib, [(layout[k]["name"], layout[k]["offset"], 0) for k in order], checksum)
            assert st == 0 and got == want and need == len(want), offsets[:4]
        m = sum(o > 0x7fffffff for o in offsets)
        assert len(want) == 8 + 1024 + 28 * len(offsets) + 8 * m + 40
        assert pm.read_idx(want)[2]["has64"] == int(m != 0)


def test_round_trip_through_the_reader():
    lib = _lib_()
    family, _, _ = pc.index_cases()
    for label, idx, st in family:
        if st != pm.OK:
            continue
        info = _lib.PackIndexInfo()
        assert lib.md_pack_index(idx, len(idx), ctypes.byref(info), None, 0) == 0
        ents = (_lib.PackIndexEntry * max(info.n, 1))()
        assert lib.md_pack_index(idx, len(idx), ctypes.byref(info), ents, info.n) == 0
        entries = [(bytes(e.name), e.offset, e.crc32) for e in ents[:info.n]]
        st, got, _ = _write(lib, entries, bytes(info.pack_checksum))
        # (an idx whose every offset goes through the 64-bit table is valid, but not what a writer makes of small offsets)
        want = idx if not info.has_64bit_table else pw.write_idx(b"", [{"name": n, "offset": o, "packed_len": 0} for n, o, _ in entries],
                                                                 idx_crc={k: c for k, (_, _, c) in enumerate(entries)}, pack_checksum=bytes(info.pack_checksum))
        assert st == 0 and got == want, label
    from decompress_amd import pack as mp
    ents, info = mp.index(family[0][1])
    assert mp.write_index(ents, info["pack_checksum"]) == family[0][1]


def test_refusals():
    lib = _lib_()
    checksum = bytes(20)
    a, b = hashlib.sha1(b"a").digest(), hashlib.sha1(b"b").digest()
    st, got, _ = _write(lib, [(a, 12, 1), (b, 40, 2), (a, 90, 3)], checksum, cap=4096)
    assert st == pm.INVALID_INDEX and got == b"\xaa" * 4096
    good = [(a, 12, 1), (b, 40, 2)]
    st, want, need = _write(lib, good, checksum)
    assert st == 0 and need == 8 + 1024 + 56 + 40
    st, got, short = _write(lib, good, checksum, cap=need - 1)
    assert st == END_OF_OUTPUT and short == need and got == b"\xaa" * (need - 1)
    st, got, need = _write(lib, [], checksum)
    assert st == 0 and need == 1072 and got == pw.write_idx(checksum, [])
    n = ctypes.c_size_t(0)
    assert lib.md_pack_index_write(None, 1, checksum, None, 0, ctypes.byref(n)) == -1
    assert lib.md_pack_index_write(None, 0, None, None, 0, ctypes.byref(n)) == -1
    assert lib.md_pack_index_write(None, 0, checksum, None, 0, None) == -1
