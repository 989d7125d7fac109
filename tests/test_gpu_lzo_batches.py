"""The batched LZO1X decoder (csrc/lzo_kernels.hip) at the limits of its batches, on streams written instruction by
instruction (tests/lzo_writer.py, the families of tests/lzo_batches.py) instead of by a compressor: both states of the
decoder on the fast path (M1, opcodes below 16), the lengths and offsets where the fast path hands over to the
one-instruction interpreter, opcodes and literals over windows, input blocks and the ring's wrap, batches that are
exactly full, every alignment of a batch's start and end, match sources in front of, across and inside the batch, the
room's edges and failures at chosen lanes.  tests/test_lzo_writer.py asserts on the CPU that the streams are where
they claim to be.

Every launch goes through Engine.lzo_batch with the outputs at offsets of every residue mod 16 in a buffer filled with
a sentinel: status and bytes are the writer's expansion and the oracle's, and nothing outside a stream's output is
touched.  Of a stream that fails the decoder reports no output, but - like the reference, which decodes into the
caller's buffer - it has written what it decoded before the failure: for such a stream "outside" is outside its room
[out_off, out_off + cap); for a stream that succeeds it is outside [out_off, out_off + out_len).  All comparisons are
exact.  Needs an MI355X: `pytest -m gpu`."""
import ctypes

import numpy as np
import pytest

from tests.lzo_batches import FAMILIES, family_g

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
SEEN = {}  # family -> the statuses of its streams


@pytest.fixture(scope="module")
def eng():
    import decompress_amd
    return decompress_amd.Engine(0)


_ORACLE = {}


def _oracle(oracle, c):
    key = (id(c.b), len(c.stream), c.cap)
    if key not in _ORACLE:
        _ORACLE[key] = oracle.lzo_uncompress(c.stream, c.cap)
    return _ORACLE[key]


def _run(eng, oracle, cases, shift=0):
    """one launch: inputs back to back, outputs `cap` bytes each with 1..16 sentinel bytes between them so that stream
    i starts at residue (i + shift) mod 16"""
    import torch
    n = len(cases)
    in_len = np.array([len(c.stream) for c in cases], dtype=np.int64)
    in_off = np.zeros(n, dtype=np.int64)
    np.cumsum(in_len[:-1], out=in_off[1:])
    cap = np.array([c.cap for c in cases], dtype=np.int64)
    out_off = np.zeros(n, dtype=np.int64)
    at = 256
    for i in range(n):
        at += (i + shift - at) % 16 or 16
        out_off[i] = at
        at += int(cap[i])
    size = at + 256
    assert {int(o) % 16 for o in out_off} == set(range(16)) or n < 16
    dev = eng.device
    t = lambda a: torch.from_numpy(a).to(dev)
    d_in = t(np.frombuffer(b"".join(c.stream for c in cases) + bytes(64), dtype=np.uint8).copy())
    d_out = torch.full((size,), SENTINEL, dtype=torch.uint8, device=dev)
    out_len, status = eng.lzo_batch(False, d_in, t(in_off), t(in_len), d_out, t(out_off), t(cap))
    torch.cuda.synchronize(dev)
    out, out_len, status = d_out.cpu().numpy(), out_len.cpu().numpy(), status.cpu().numpy()
    may = np.zeros(size, dtype=bool)  # what a stream may have written
    seen = set()
    for i, c in enumerate(cases):
        st, ln, o = int(status[i]), int(out_len[i]), int(out_off[i])
        assert 0 <= ln <= c.cap, c.name
        got = out[o:o + ln].tobytes()
        ost, oout = _oracle(oracle, c)
        if c.out is not None:
            assert (ost, oout) == (0, c.out), c.name  # the writer's expansion is the oracle's
        else:
            assert ost != 0 and oout == b"", c.name
        assert st == ost, (c.name, st, ost)
        assert got == oout, (c.name, ln, len(oout), next((k for k, (a, b) in enumerate(zip(got, oout)) if a != b), None))
        may[o:o + (ln if st == 0 else c.cap)] = True
        seen.add(st)
    outside = np.nonzero(~may & (out != SENTINEL))[0]
    if outside.size:
        k = int(np.searchsorted(out_off, outside[0], side="right")) - 1
        raise AssertionError("written outside a stream's output: byte %d, %d bytes behind the start of %r (room %d, length %d)"
                             % (outside[0], outside[0] - out_off[k], cases[k].name, cases[k].cap, out_len[k]))
    return seen


@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_family(eng, oracle, fam):
    """the family's streams in one launch - twice over with the output offsets shifted, so that every stream of a family
    of fewer than 16 meets more than one alignment"""
    cases = FAMILIES[fam]()
    SEEN[fam] = _run(eng, oracle, cases) | _run(eng, oracle, cases, shift=5) | _run(eng, oracle, cases, shift=11)


def _resident_workgroups(eng):
    import torch
    slots = eng.lib.md_lzo_slots
    slots.restype, slots.argtypes = ctypes.c_uint32, [ctypes.c_int, ctypes.c_uint32]
    return slots(0, torch.cuda.get_device_properties(eng.device).multi_processor_count)


def test_many_at_once(eng, oracle):
    """G: all of A-F and the small ones again, 2 000 streams or more shuffled into one launch - a quarter more than the
    resident workgroups hold, so that the streams are handed out by the counter in another order"""
    resident = _resident_workgroups(eng)
    cases = family_g(max(2000, resident + resident // 4))
    assert len(cases) > resident > 0
    SEEN["G"] = _run(eng, oracle, cases)


def test_corpus_statuses(eng, oracle):
    """over all families: success, "unexpected end of input" and "out of bound" have all been met on the GPU"""
    seen = set().union(*(SEEN.get(f) or _run(eng, oracle, FAMILIES[f]()) for f in sorted(FAMILIES)))
    assert seen >= {0, 1, 16}, seen
