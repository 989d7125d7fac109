"""The LZO size query on the GPU (md_lzo_sizes_batch_*, md_lzo_uncompress_with_buffer; csrc/lzo_kernels.hip
lzo_count_kernel): every stream's uncompressed size without decoding it, with the statuses of
Lzo.uncompress_with_buffer.  The yardstick is tests/lzo_buffer_model.py (held to the CPU oracle by
tests/test_lzo_buffer_model.py), the writers' own byte-serial expansions and the fixtures - never the library's decoder,
except where a test says that the decode into planned room gives the originals back.  All comparisons are exact."""
import ctypes
import functools
import random

import numpy as np
import pytest

from tests import lzo_batches
from tests import lzo_buffer_model as model
from tests.conftest import golden_bytes, load_golden
from tests.lzo_writer import encode

pytestmark = pytest.mark.gpu

END = bytes([17, 0, 0])
MAX_STREAM = 0xfffffff0


@pytest.fixture(scope="module")
def eng():
    import decompress_amd
    return decompress_amd.Engine(0)


def _upload(eng, streams):
    import torch
    in_len = np.array([len(s) for s in streams], dtype=np.int64)
    in_off = np.zeros(len(streams), dtype=np.int64)
    np.cumsum(in_len[:-1], out=in_off[1:])
    blob = np.frombuffer(b"".join(bytes(s) for s in streams) + bytes(64), dtype=np.uint8).copy()
    t = lambda a: torch.from_numpy(a).to(eng.device)
    d = (t(blob), t(in_off), t(in_len))
    torch.cuda.synchronize(eng.device)
    return d


def _sizes(eng, streams):
    """[(status, out_len)] of the device form, one launch"""
    import torch
    out_len, status = eng.lzo_sizes(*_upload(eng, streams))
    eng.synchronize()
    torch.cuda.synchronize(eng.device)
    out_len, status = out_len.cpu().numpy(), status.cpu().numpy()
    return [(int(status[i]), int(out_len[i])) for i in range(len(streams))]


@functools.lru_cache(None)
def _model(stream):
    return model.size(stream)


def _distinct(cases):
    """a family lists a stream once per output cap: every distinct stream once"""
    seen, out = set(), []
    for c in cases:
        if c.stream not in seen:
            seen.add(c.stream)
            out.append(c)
    return out


def _whole(c):
    return not c.b.malformed and c.b.ended and len(c.stream) == len(c.b.stream)


@pytest.mark.parametrize("fam", sorted(lzo_batches.FAMILIES))
def test_family(eng, fam):
    """1. every distinct stream of a family, one launch: the model's status and size, the writer's size for valid streams;
    the same through the host-pointer form"""
    cases = _distinct(lzo_batches.FAMILIES[fam]())
    streams = [c.stream for c in cases]
    dev, host = _sizes(eng, streams), eng.lzo_sizes_host(streams)
    for c, got, hgot in zip(cases, dev, host):
        assert got == _model(c.stream), (c.name, got, _model(c.stream))
        assert hgot == got, (c.name, hgot, got)
        if _whole(c):
            assert got == (0, len(c.b.out)), (c.name, got, len(c.b.out))
    assert any(g[0] == 0 and g[1] > 0 for g in dev)


def test_many_at_once(eng):
    """2. more streams than the count kernel's resident workgroups: the counter hands them out in an order of its own"""
    import torch
    slots = eng.lib.md_lzo_slots
    slots.restype, slots.argtypes = ctypes.c_uint32, [ctypes.c_int, ctypes.c_uint32]
    cus = torch.cuda.get_device_properties(eng.device).multi_processor_count
    resident = slots(2, cus)
    assert resident > 0 and slots(0, cus) > 0 and slots(1, cus) > 0
    cases = lzo_batches.family_g(max(2000, resident + resident // 4))
    assert len(cases) > resident
    for k, (c, got) in enumerate(zip(cases, _sizes(eng, [c.stream for c in cases]))):
        assert got == _model(c.stream), (k, c.name, got, _model(c.stream))


def test_reference_vectors(eng):
    """3. the 34 decoder cases of test/test_lzo.ml, the zero runs of 4, 8 and 17 MB among them: sizes, and the bytes
    through lzo.uncompress_with_buffer"""
    from decompress_amd import engine, lzo
    cases = load_golden("lzo.json")
    assert len(cases) == 34
    srcs = [golden_bytes(c["src"]) for c in cases]
    for c, src, got in zip(cases, srcs, _sizes(eng, srcs)):
        want = model.size(src)
        assert got == want, (c["name"], got, want)
        res = lzo.uncompress_with_buffer(src)
        if c["status"] == 0:
            out = golden_bytes(c["out"])
            assert got == (0, len(out)), c["name"]
            assert res == ("Ok", out), c["name"]
            assert lzo.uncompressed_size(src) == ("Ok", len(out)), c["name"]
        else:
            assert got[0] != 0 and res == ("Error", engine.STATUS_NAMES[want[0]]), (c["name"], res)


def test_random_and_cut_streams(eng):
    """4. the short random streams and the cut stream of the CPU test, one batch"""
    streams = model.random_streams() + model.cut_streams()
    seen = set()
    for k, (s, got) in enumerate(zip(streams, _sizes(eng, streams))):
        assert got == model.size(s), (k, s[:64].hex(), got, model.size(s))
        seen.add(got[0])
    assert seen >= set(model.STATUSES), seen


def _edge(pos, lane, form, off, valid):
    """a match of `form` at offset `off` that is the instruction at lane `lane` of a window, with exactly `pos` bytes of
    output in front of it -> (stream, expected size or None)"""
    pre = 300
    for _ in range(3):  # (the bytes in front of the match: the leading literals make up for what the padding produces)
        b = lzo_batches.Build(random.Random(pos * 64 + lane), pre)
        b.place(0, lane)
        pre += pos - b.opos
    assert b.opos == pos and b.ipos == b.b0 + lane
    if valid:
        b.m(off, 5, 2, form)
        b.finish(tail=False)
        return bytes(b.stream), len(b.out)
    return bytes(b.stream) + encode(form, off, 5, 2) + bytes(400), None


def _edge_cases():
    cases = []
    for p in (1, 2, 3, 4):  # small positions: first-byte literals, then the match
        head = bytes([17 + p]) + bytes(range(1, p + 1))
        cases.append(("pos %d off %d" % (p, p), head + encode("M2", p, 3, 0) + END, p + 3))
        cases.append(("pos %d off %d" % (p, p + 1), head + encode("M2", p + 1, 3, 0) + END, None))
    spots = [(700, "M2", 700, True), (700, "M2", 701, False), (5000, "M3", 5000, True), (5000, "M3", 5001, False),
             (16384, "M3", 16384, True), (16383, "M3", 16384, False),  # (offset 16 384: the interpreter's)
             (16385, "M4", 16385, True), (16385, "M4", 16386, False),
             (49151, "M4", 49151, True), (49150, "M4", 49151, False),
             (49152, "M4", 49151, True), (49153, "M4", 49151, True), (49215, "M4", 49151, True)]
    for (pos, form, off, valid), lane in ((s, l) for s in spots for l in (0, 28, 63)):
        stream, size = _edge(pos, lane, form, off, valid)
        cases.append(("pos %d off %d lane %d" % (pos, off, lane), stream, size))
    return cases


def test_offset_edge(eng):
    """5. a match whose offset equals the bytes so far (valid) and exceeds them by one (`Invalid_dictionary): at small
    positions, below and at the last position an offset can exceed (49 150 / 49 151 with offset 49 151), just past
    49 152 where nothing is checked any more, as the first, a middle and the last instruction of a window"""
    cases = _edge_cases()
    seen = set()
    for (name, s, size), got in zip(cases, _sizes(eng, [c[1] for c in cases])):
        want = (0, size) if size is not None else (model.INVALID_DICTIONARY, 0)
        assert model.size(s) == want, (name, model.size(s), want)
        assert got == want, (name, got, want)
        seen.add(got[0])
    assert seen == {0, model.INVALID_DICTIONARY}


def test_beyond_4_gib(eng):
    """6. four literals, then three matches at offset 1 whose lengths go on over 5.62 million zero bytes each: the size is
    more than 32 bits hold, exact - and more than the decoder writes"""
    zeros, last = 5_620_000, 77
    match = bytes([32]) + bytes(zeros) + bytes([last, 0, 0])  # M3, offset 1, no literals
    stream = bytes([17 + 4]) + b"abcd" + match * 3 + END
    size = 4 + 3 * (31 + zeros * 255 + last + 2)
    assert size > 1 << 32 and size > MAX_STREAM and model.size(stream) == (0, size)
    assert _sizes(eng, [stream, END]) == [(0, size), (0, 0)]
    assert eng.lzo_sizes_host([stream]) == [(0, size)]
    dst, n = ctypes.c_void_p(), ctypes.c_size_t(5)
    rc = eng.lib.md_lzo_uncompress_with_buffer(eng.ctx, stream, len(stream), ctypes.byref(dst), ctypes.byref(n))
    assert rc == -1 and not dst.value and n.value == 0  # MD_E_INVALID_ARGUMENT


def _failing():
    """a stream of every failing status -> {status: stream}"""
    bad = {model.END_OF_INPUT: bytes([17 + 3]) + b"abc", model.INVALID_DICTIONARY: bytes([18, 65]) + encode("M2", 2, 3, 0) + END,
           model.INVALID_INPUT: bytes(3), model.NO_DICTIONARY: bytes([16, 1, 2, 3]), model.MALFORMED: bytes([17 + 5, 1, 2])}
    for st, s in bad.items():
        assert model.size(s) == (st, 0), (st, model.size(s))
    return bad


def test_lzo_many_without_caps(eng, oracle):
    """7. the corpus files compressed by the oracle, failing streams of every status among them, through
    Engine.lzo_many(False, streams, None): sizes, plan, decode.  The originals come back, the statuses are the model's,
    and the plan's offsets are 256-aligned and back to back."""
    import torch
    from decompress_amd import workloads
    files = list(workloads.corpus().values())
    zs = []
    for b in files:
        st, z = oracle.lzo_compress(b)
        assert st == 0
        zs.append(z)
    bad = list(_failing().items())
    streams, want = [], []
    for k, (b, z) in enumerate(zip(files, zs)):
        streams.append(z), want.append((0, b))
        st, s = bad[k % len(bad)]
        streams.append(s), want.append((st, b""))
        if k % 3 == 0:
            streams.append(z[:len(z) // 2]), want.append((model.size(z[:len(z) // 2])[0], b""))
    assert {w[0] for w in want} >= set(model.STATUSES)
    got = eng.lzo_many(False, streams, None)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g[0], w[0], len(g[1]), len(w[1]))
    # the plan behind it
    sizes, status = eng.lzo_sizes(*_upload(eng, streams))
    out_off, out_cap, total = eng.inflate_plan(sizes, 256)
    eng.synchronize()
    torch.cuda.synchronize(eng.device)
    sz, off, cap = sizes.cpu().numpy(), out_off.cpu().numpy(), out_cap.cpu().numpy()
    assert [int(x) for x in sz] == [len(w[1]) for w in want] and [int(x) for x in status.cpu().numpy()] == [w[0] for w in want]
    aligned = (sz + 255) // 256 * 256
    assert (cap == sz).all() and (off % 256 == 0).all()
    assert (off == np.cumsum(aligned) - aligned).all() and int(total.item()) == int(aligned.sum())


def test_uncompress_with_buffer_abi(eng, oracle):
    """8. md_lzo_uncompress_with_buffer through ctypes: a valid stream, an empty result, an empty input and every failing
    status; the block is the caller's, freed with md_host_free"""
    from decompress_amd import lzo, workloads
    lib = eng.lib

    def call(src):
        dst, n = ctypes.c_void_p(), ctypes.c_size_t(123)
        rc = lib.md_lzo_uncompress_with_buffer(eng.ctx, bytes(src), len(src), ctypes.byref(dst), ctypes.byref(n))
        if rc != 0:
            assert not dst.value and n.value == 0, rc
            return rc, None
        assert dst.value  # (an empty result is a block too)
        out = ctypes.string_at(dst.value, n.value)
        lib.md_host_free(eng.ctx, dst)
        return rc, out

    text = workloads.text(8, 300000)
    st, z = oracle.lzo_compress(text)
    assert st == 0
    assert call(z) == (0, text)
    assert call(END) == (0, b"")
    assert call(b"") == (model.END_OF_INPUT, None)
    for st, s in _failing().items():
        assert call(s) == (st, None), st
    assert call(z[:-1])[0] == model.size(z[:-1])[0] != 0
    assert lzo.uncompress_with_buffer(z, chunk=7) == ("Ok", text)
    assert lzo.uncompress_with_buffer(bytes([16])) == ("Error", "No dictionary at offset 0 available")
    assert lzo.uncompress_with_buffer(bytes([17 + 5, 1, 2])) == ("Error", "Malformed input")
    assert lzo.uncompressed_size(bytes([18, 65]) + encode("M2", 2, 3, 0) + END) == ("Error", "Invalid_dictionary")
