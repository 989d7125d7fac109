"""SHA-1 of many buffers on the GPU (md_sha1_batch_host, md_sha1_batch_device; csrc/sha1_kernels.hip).  Needs an
MI355X: `pytest -m gpu`.  Yardstick: hashlib over the same bytes, with Python's own "<type> <size>\\0" in front for the git
types - never the code under test."""
import ctypes
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TYPE_NAMES = {1: b"commit", 2: b"tree", 3: b"blob", 4: b"tag"}


@pytest.fixture(scope="module")
def eng():
    from decompress_amd import engine
    return engine.default_engine(0)


def _want(data, t):
    return hashlib.sha1((TYPE_NAMES[t] + b" %d\0" % len(data) if t else b"") + data).digest()


def _blocks(n, t):
    head = len(TYPE_NAMES[t]) + 1 + len(str(n)) + 1 if t else 0
    return (head + n + 9 + 63) // 64


def _bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _laid_out(msgs, aligns):
    """the messages in one blob, message i at an address that is aligns[i] mod 16, the gaps (never empty) filled with 0xff:
    a mask one byte too wide hashes an 0xff"""
    blob, off = bytearray(), []
    for m, a in zip(msgs, aligns):
        blob += b"\xff"
        blob += b"\xff" * ((a - len(blob)) % 16)
        off.append(len(blob))
        blob += m
    return bytes(blob), off


@pytest.fixture(scope="module")
def family():
    """lengths 0 .. 200 and 4 095 .. 4 097 at every alignment 0 .. 15, the types going round: (blob, off, len, type, want)"""
    msgs, aligns, types = [], [], []
    for n in list(range(201)) + [4095, 4096, 4097]:
        for a in range(16):
            msgs.append(_bytes(n, 16 * n + a))
            aligns.append(a)
            types.append((n + a) % 5)
    blob, off = _laid_out(msgs, aligns)
    assert {(o % 16, t) for o, t in zip(off, types)} == {(a, t) for a in range(16) for t in range(5)}
    return blob, off, [len(m) for m in msgs], types, [_want(m, t) for m, t in zip(msgs, types)]


def _host(eng, blob, off, lens, types):
    n = len(off)
    data = np.frombuffer(blob, dtype=np.uint8)
    o, ln = np.array(off or [0], dtype=np.uint64), np.array(lens or [0], dtype=np.uint64)
    t = None if types is None else np.array(types or [0], dtype=np.uint8)
    digest = np.zeros(20 * max(n, 1), dtype=np.uint8)
    rc = eng.lib.md_sha1_batch_host(eng.ctx, n, data.ctypes.data if data.size else None, data.size, o.ctypes.data, ln.ctypes.data,
                                    t.ctypes.data if t is not None else None, digest.ctypes.data)
    return rc, [digest[20 * i:20 * i + 20].tobytes() for i in range(n)]


def test_every_length_alignment_and_type_host_form(eng, family):
    blob, off, lens, types, want = family
    rc, got = _host(eng, blob, off, lens, types)
    assert rc == 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, lens[i], off[i] % 16, types[i])
    last = eng.sha1_last()
    assert last["messages"] == len(off) and last["blocks"] == sum(_blocks(n, t) for n, t in zip(lens, types))
    assert last["launches"] == 1 and last["device_ns"] > 0
    # without types: the bytes as they are
    rc, got = _host(eng, blob, off, lens, None)
    assert rc == 0 and got == [hashlib.sha1(blob[o:o + n]).digest() for o, n in zip(off, lens)]


def test_every_length_alignment_and_type_device_form(eng, family):
    import torch
    blob, off, lens, types, want = family
    dev = eng.device
    d_data = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(np.array(off, dtype=np.int64)).to(dev)
    d_len = torch.from_numpy(np.array(lens, dtype=np.int64)).to(dev)
    d_type = torch.from_numpy(np.array(types, dtype=np.uint8)).to(dev)
    torch.cuda.synchronize(dev)
    try:
        eng.set_option("sha1_launch_blocks", 16)  # 4 097 bytes are 65 blocks: the resume path of the unordered form
        digest = eng.sha1_batch_device(d_data, d_off, d_len, d_type, max(lens))
        eng.synchronize()
        got = digest.cpu().numpy().tobytes()
        assert [got[20 * i:20 * i + 20] for i in range(len(off))] == want
        last = eng.sha1_last()
        assert last["launches"] == -(-_blocks(max(lens), 1) // 16) == 5 and last["messages"] == len(off) and last["device_ns"] > 0
        digest = eng.sha1_batch_device(d_data, d_off, d_len, None, max(lens))
        eng.synchronize()
        got = digest.cpu().numpy().tobytes()
        assert [got[20 * i:20 * i + 20] for i in range(len(off))] == [hashlib.sha1(blob[o:o + n]).digest() for o, n in zip(off, lens)]
    finally:
        from decompress_amd import engine
        eng.set_option("sha1_launch_blocks", engine.SHA1_LAUNCH_BLOCKS)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_partial_wavefronts(eng, n):
    bufs = [_bytes(37 + 3 * i, 900 + i) for i in range(n)]
    types = [i % 5 for i in range(n)]
    assert eng.sha1_batch(bufs, types) == [_want(b, t) for b, t in zip(bufs, types)]
    assert eng.sha1_last()["messages"] == n


def test_lengths_0_and_70000_in_one_call(eng):
    bufs = [b"", _bytes(70000, 1), b"", _bytes(70000, 2), _bytes(1, 3)]
    types = [3, 3, 0, 0, 4]
    assert eng.sha1_batch(bufs, types) == [_want(b, t) for b, t in zip(bufs, types)]
    assert _want(b"", 3).hex() == "e69de29bb2d1d6434b8b29ae775ad8c2e48c5391"  # (git's empty blob)


@pytest.mark.parametrize("per_launch", [1, 2, 3])
def test_messages_resumed_across_launches(eng, per_launch):
    """messages of 1 .. 6 blocks (0 .. 5 full blocks of content and what the padding adds), several of each, advanced by
    1, 2 or 3 blocks a launch: the same digests, and as many launches as the longest needs"""
    from decompress_amd import engine
    lens = [0, 1, 55, 56, 63, 64, 119, 120, 128, 183, 184, 200, 247, 248, 256, 311, 312, 320]
    bufs = [_bytes(n, 70 + k) for k, n in enumerate(lens * 5)]
    types = [k % 5 for k in range(len(bufs))]
    longest = max(_blocks(len(b), t) for b, t in zip(bufs, types))
    assert sorted({_blocks(len(b), t) for b, t in zip(bufs, types)}) == [1, 2, 3, 4, 5, 6]
    try:
        eng.set_option("sha1_launch_blocks", per_launch)
        got = eng.sha1_batch(bufs, types)
        last = eng.sha1_last()
    finally:
        eng.set_option("sha1_launch_blocks", engine.SHA1_LAUNCH_BLOCKS)
    assert got == [_want(b, t) for b, t in zip(bufs, types)]
    assert last["launches"] == -(-longest // per_launch) and last["launches"] > 1
    assert last["blocks"] == sum(_blocks(len(b), t) for b, t in zip(bufs, types))


def test_nothing_and_misuse(eng):
    from decompress_amd import engine
    assert eng.sha1_batch([]) == []
    assert eng.sha1_last() == {"messages": 0, "blocks": 0, "launches": 0, "device_ns": 0}
    rc, _ = _host(eng, b"abcdef", [0], [6], [5])
    assert rc == -1
    rc, _ = _host(eng, b"abcdef", [2], [5], None)  # one byte beyond the data
    assert rc == -1
    rc, _ = _host(eng, b"abcdef", [7], [0], None)
    assert rc == -1
    rc, got = _host(eng, b"abcdef", [6, 0], [0, 6], None)  # an empty message at the very end
    assert rc == 0 and got == [hashlib.sha1(b"").digest(), hashlib.sha1(b"abcdef").digest()]
    digest = (ctypes.c_uint8 * 20)()
    one = (ctypes.c_uint64 * 1)(0)
    assert eng.lib.md_sha1_batch_host(eng.ctx, 1, b"x", 1, None, one, None, digest) == -1
    assert eng.lib.md_sha1_batch_host(eng.ctx, 1, b"x", 1, one, one, None, None) == -1
    for bad in (0, -1, (1 << 24) + 1):
        with pytest.raises(engine.Error):
            eng.set_option("sha1_launch_blocks", bad)
    eng.set_option("sha1_launch_blocks", 1 << 24)
    eng.set_option("sha1_launch_blocks", engine.SHA1_LAUNCH_BLOCKS)
    with pytest.raises(engine.Error):
        eng.sha1_batch([b"x"], [5])
