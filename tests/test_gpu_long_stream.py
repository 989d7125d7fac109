"""The long-stream inflate path (csrc/inflate_chunked.hip, par_decode in csrc/capi_long_stream.cpp) on the hand-built
streams of tests/long_stream_cases.py.  Needs an MI355X: `pytest -m gpu`.

The path hides its own failures: a flag from the device, a checksum that does not match or a piece status it does not
expect sends the stream to the serial decoder, which produces the right bytes a hundred times slower.  So every valid stream
here must come back THROUGH the pieces (`inflate_parallel_last` says how many, and in how many decode rounds), in exactly the
pieces tests/test_long_stream_cases.py predicted on the CPU wherever every candidate is a block start - and most go through
md_de_higher_uncompress, the raw frame, where no checksum stands behind a wrong byte of resolve_kernel.  An invalid
stream (a match that reaches in front of the stream's start) must be REFUSED by the path: the serial decoder's status and
bytes, and no pieces."""
import contextlib
import ctypes
import zlib

import pytest

from tests import deflate_writer as dw
from tests import long_stream_cases as lc

pytestmark = pytest.mark.gpu

ALL = [(f, i) for f in lc.FAMILIES for i in range(lc.COUNTS[f])]
UNEXPECTED_END_OF_INPUT = 1


@pytest.fixture(scope="module")
def eng():
    import decompress_amd
    return decompress_amd.Engine(0)


@contextlib.contextmanager
def _path(eng, parallel=True):
    """the long-stream decoder in pieces of 4 KiB, for pieces of the protocol from 16 KiB on - or never"""
    eng.set_option("inflate_parallel_chunk", 4)
    eng.set_option("inflate_parallel_min", 16 if parallel else 0)
    try:
        yield
    finally:
        eng.set_option("inflate_parallel_chunk", 64)
        eng.set_option("inflate_parallel_min", 96)


def _par_last(eng):
    v = eng.lib.md_set_option(eng.ctx, b"inflate_parallel_last", 0)
    return v & 0xffffff, v >> 24  # pieces (0: the serial path took the stream), decode rounds


def _higher(eng, fmt, z, cap):
    """-> (status, bytes of input used where the call says so, output)"""
    dst = ctypes.create_string_buffer(max(cap, 1))
    used, wrote = ctypes.c_size_t(), ctypes.c_size_t()
    if fmt == "zl":
        st = eng.lib.md_zl_higher_uncompress(eng.ctx, z, len(z), dst, cap, ctypes.byref(wrote))
    elif fmt == "de":
        st = eng.lib.md_de_higher_uncompress(eng.ctx, z, len(z), dst, cap, ctypes.byref(wrote))
    else:
        st = eng.lib.md_gz_higher_uncompress(eng.ctx, z, len(z), dst, cap, ctypes.byref(used), ctypes.byref(wrote), None)
    return st, used.value if fmt == "gz" else None, dst.raw[:wrote.value]


def _continue(eng, src, hist, cap):
    """md_de_inf_continue_host on one piece of the protocol, Adler-32 from 1 and the CRC-32 of the new output
    -> (status, output position, new bytes, the resume record's fields)"""
    from decompress_amd import _lib
    dst = ctypes.create_string_buffer(bytes(hist), max(1, cap))
    n, st, rs = ctypes.c_size_t(), ctypes.c_int(), _lib.InfResume()
    eng._check(eng.lib.md_de_inf_continue_host(eng.ctx, bytes(src), len(src), 0, dst, len(hist), cap, 1, 1, ctypes.byref(n), ctypes.byref(st),
                                               ctypes.byref(rs)))
    return st.value, n.value, dst.raw[len(hist):n.value], {f: getattr(rs, f) for f, _ in rs._fields_}


def _check_counts(case, fmt, pieces, rounds):
    want = case.pieces[fmt]
    print("long stream: %-44s %s predicted %s pieces, %s; observed %d pieces in %d round(s)"
          % (case.name, fmt, want, "more than one round" if case.rounds2 else "one round", pieces, rounds))
    assert pieces > 0, "the serial path took the stream"
    if want is not None:
        assert pieces == want
    assert rounds >= 2 if case.rounds2 else rounds == 1
    assert pieces < lc.JUMP_FROM if case.variant == "chain" else pieces >= lc.JUMP_FROM


@pytest.mark.parametrize("fam,i", [p for p in ALL if p[0] != "H"], ids=lambda v: str(v))
def test_streams_through_the_pieces(eng, fam, i):
    case = lc.family(fam)[i]
    if case.status != dw.OK:
        cap = case.meta["total"]
        with _path(eng):
            got = _higher(eng, "de", case.raw, cap)
            pieces, rounds = _par_last(eng)
        with _path(eng, parallel=False):
            want = _higher(eng, "de", case.raw, cap)
        print("long stream: %-44s refused: status %d behind %d bytes, %d pieces" % (case.name, got[0], len(got[2]), pieces))
        assert (got[0], got[2]) == (case.status, case.plain)
        assert got == want and pieces == 0
        return
    for fmt in case.pieces:
        src = lc.frame(case.raw, case.plain, fmt)
        with _path(eng):
            st, used, out = _higher(eng, fmt, src, len(case.plain))
            pieces, rounds = _par_last(eng)
        assert st == 0 and len(out) == len(case.plain)
        assert out == case.plain, next(k for k in range(len(out)) if out[k] != case.plain[k])
        assert used in (None, len(src))
        _check_counts(case, fmt, pieces, rounds)


@pytest.mark.parametrize("i", range(lc.COUNTS["H"]))
def test_a_piece_of_the_protocol_with_history(eng, i):
    """md_de_inf_continue_host: the window the caller hands in lies in front of piece 0, and a match of a later piece may
    reach its first byte and not the byte in front of it"""
    case = lc.family("H")[i]
    hist, cut = case.meta["hist"], case.meta["cut"]
    src = case.raw if cut is None else case.raw[:cut]
    cap = len(hist) + case.meta["total"]
    with _path(eng):
        got = _continue(eng, src, hist, cap)
        pieces, rounds = _par_last(eng)
    with _path(eng, parallel=False):
        want = _continue(eng, src, hist, cap)
    st, at, new, rs = got
    if case.status != dw.OK:
        print("long stream: %-44s refused: status %d behind %d bytes, %d pieces" % (case.name, st, len(new), pieces))
        assert (st, new) == (case.status, case.plain) and got == want and pieces == 0
        return
    assert got == want
    if cut is None:
        assert st == 0 and new == case.plain and at == len(hist) + len(new)
        assert rs["consumed"] == len(src) and rs["last"] == 1
        assert rs["checksum"] == zlib.adler32(new) and rs["crc_end"] == zlib.crc32(new)
    else:  # the piece ends inside a block: its complete blocks by the pieces, what the block holds up to there by the serial path
        whole = max((b, o) for b, o in case.starts if b < 8 * cut)
        assert st == UNEXPECTED_END_OF_INPUT and case.plain.startswith(new) and len(new) >= whole[1]
        assert rs["bits"] == whole[0] and rs["out"] == len(hist) + whole[1] and rs["adler"] == zlib.adler32(new[:whole[1]])
    _check_counts(case, "de", pieces, rounds)
