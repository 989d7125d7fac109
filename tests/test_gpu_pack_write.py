"""Writing git packs on the GPU (md_pack_delta_batch_*, md_pack_write; csrc/pack_write_kernels.hip).  Needs an
MI355X: `pytest -m gpu`.  Yardstick: tests/pack_delta_model.py - the header's definition in Python, checked on the CPU
against git itself (test_pack_write_model.py) - held to byte for byte; the payloads' streams are the oracle's."""
import ctypes

import numpy as np
import pytest

from tests import pack_delta_model as dm
from tests import pack_write_cases as wc

pytestmark = pytest.mark.gpu
LEVELS = (0, 1, 6, 9)


@pytest.fixture(scope="module")
def eng():
    from decompress_amd import engine
    return engine.default_engine(0)


@pytest.fixture(scope="module")
def family():
    """every pair of every delta case in one blob at every alignment: (blob, rows, [model delta])"""
    cases = wc.delta_cases()
    blob, rows, who = wc.laid_out(cases)
    models = [wc.delta_model(c)[1] for c in cases]
    return blob, rows, [models[ci][pi] for ci, pi in who], ["%s / %d" % (cases[ci]["name"], pi) for ci, pi in who]


def _check(got, want, caps, names):
    for (st, d), w, cap, name in zip(got, want, caps, names):
        if len(w) <= cap:
            assert st == dm.MD_OK and d == w, name
        else:
            assert (st, d) == (dm.MD_UNEXPECTED_END_OF_OUTPUT, b""), name


def test_every_case_in_one_batch_host_form(eng, family):
    blob, rows, want, names = family
    for caps in ([len(w) for w in want], [max(len(w) - 1, 0) for w in want], None):
        got = eng.pack_deltas(blob, rows, caps)
        _check(got, want, caps or [1 << 40] * len(want), names)
    last = eng.pack_write_last()
    assert last["pairs"] == len(rows) and last["launches"] == 2 and last["delta_ns"] > 0
    assert last["kept"] == last["dropped_size"] == last["payload_after"] == 0


def test_every_case_one_pair_at_a_time(eng):
    for c in wc.delta_cases():
        _, want = wc.delta_model(c)
        blob, rows, _ = wc.laid_out([c])
        for k, (row, w) in enumerate(zip(rows, want)):
            got = eng.pack_deltas(blob, [row], [len(w)])
            _check(got, [w], [len(w)], ["%s / %d" % (c["name"], k)])
            assert eng.pack_write_last()["launches"] == (2 if row[1] >= 16 else 1), c["name"]


def test_every_case_device_form(eng, family):
    import torch
    blob, rows, want, names = family
    dev = eng.device
    d_src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(dev)
    for short in (0, 1):
        caps = [max(len(w) - short, 0) for w in want]
        offs = np.concatenate([[0], np.cumsum([(c + 15) & ~15 for c in caps])]).astype(np.int64)
        d_out = torch.full((int(offs[-1]) + 16,), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        out_len, status = eng.pack_deltas_device([r + (int(o), c) for r, o, c in zip(rows, offs, caps)], d_src, d_out)
        eng.synchronize()
        raw, out_len, status = d_out.cpu().numpy().tobytes(), out_len.cpu().tolist(), status.cpu().tolist()
        got = [(st, raw[o:o + n]) for st, o, n in zip(status, offs, out_len)]
        _check(got, want, caps, names)
        last = eng.pack_write_last()
        assert last["pairs"] == len(rows) and last["delta_ns"] > 0
        # nothing is written outside a pair's room
        for o, c, nxt in zip(offs, caps, offs[1:]):
            assert raw[o + c:nxt] == b"\xee" * (int(nxt) - int(o) - c)


def test_one_plan_from_two_routes(eng):
    """md_pack_choose_bases lays the tables of its candidates out by rank; md_pack_delta_sizes_host finds the distinct bases of
    the same pairs by sorting them.  Both go through one builder: the sizes of the pairs the search scores for
    pack_search_cases.plan_objects() with window 1 - one base of three targets, equal bytes at two addresses as two bases -
    are the scores the search's model saw.  A search never scores a base shorter than its target, and no target has fewer
    than 64 bytes, so the base of 15 bytes (no table) and the one of exactly 16 (one block) come as two pairs more, without a
    bound, against the delta model."""
    from tests import pack_search_cases as sc
    case = sc.case("one base, three targets")
    trace = sc.search_model(case["name"])[0]
    datas = [case["objects"][i][1] for i in trace["order"]]  # by rank
    target = datas[3]
    blob, rows = sc.laid_out(datas + [target[:15], target[:16]])
    pairs = [rows[b] + rows[t] for t, b in trace["pairs"]] + [rows[7] + rows[3], rows[8] + rows[3]]
    caps = [dm.delta_cap(rows[t][1]) for t, _ in trace["pairs"]] + [1 << 40] * 2
    want = list(trace["scores"]) + [dm.delta_result(target[:k], target, 1 << 40)[:2] for k in (15, 16)]
    # the case on the CPU: five distinct bases, four with a table of 2^10 words, two of them of equal bytes
    bases = sorted({p[:2] for p in pairs})
    assert [n for _, n in bases] == [716, 716, 648, 15, 16] and datas[0] == datas[1] and rows[0][0] != rows[1][0]
    assert [dm.table_bits(n // dm.BLOCK) for _, n in bases if n >= dm.BLOCK] == [10] * 4
    assert sorted(p[:2] for p in pairs).count(rows[2]) == 3 and all(st == dm.MD_OK for st, _ in want)
    assert eng.pack_delta_sizes(blob, pairs, caps) == want
    last = eng.pack_write_last()
    assert last["pairs"] == 7 and last["launches"] == 2 and last["delta_ns"] > 0


def test_delta_batch_misuse(eng):
    from decompress_amd import _lib
    lib = eng.lib
    assert eng.pack_deltas(b"", []) == []
    assert eng.pack_write_last()["pairs"] == 0
    src, out = b"x" * 100, ctypes.create_string_buffer(64)
    n64, n32 = (ctypes.c_uint64 * 1)(), (ctypes.c_int32 * 1)()

    def call(fields, src_len=100, out_bytes=64):
        pair = (_lib.PackDeltaPair * 1)()
        pair[0].base_off, pair[0].base_len, pair[0].tgt_off, pair[0].tgt_len, pair[0].out_off, pair[0].out_cap = fields
        return lib.md_pack_delta_batch_host(eng.ctx, 1, pair, src, src_len, out, out_bytes, n64, n32)
    assert call((0, 50, 50, 50, 0, 64)) == 0
    assert call((0, 50, 51, 50, 0, 64)) == -1  # the target leaves src
    assert call((51, 50, 0, 50, 0, 64)) == -1  # the base leaves src
    assert call((0, 50, 50, 50, 1, 64)) == -1  # the room leaves out
    assert call((0, 0xFFFFFFF1, 50, 50, 0, 64)) == -1
    assert call(((1 << 64) - 1, 2, 50, 50, 0, 64)) == -1
    pair = (_lib.PackDeltaPair * 1)()
    assert lib.md_pack_delta_batch_host(eng.ctx, 1, None, src, 100, out, 64, n64, n32) == -1
    assert lib.md_pack_delta_batch_host(eng.ctx, 1, pair, src, 100, out, 64, None, n32) == -1
    assert lib.md_pack_delta_batch_host(eng.ctx, 1, pair, src, 100, out, 64, n64, None) == -1
    assert lib.md_pack_delta_batch_device(eng.ctx, 1, pair, None, None, None, None) == -1


def _runs(case):
    """[(kwargs of pack.write_raw, the model's result)] per level"""
    from decompress_amd import pack as mp
    out = []
    for level in ((case["level"],) if "level" in case else LEVELS):
        for run, r in zip(case["runs"], wc.pack_model(case["name"], level)):
            kw = {"level": level, "max_depth": run.get("max_depth", 50), "flags": 0 if run.get("deltas", True) else mp.WRITE_NO_DELTA}
            out.append((kw, r))
        if not any("deltas" in run for run in case["runs"]):  # NO_DELTA for every case
            r = dm.write_pack(case["objects"], case["bases"], level=level, deltas=False)
            out.append(({"level": level, "max_depth": 50, "flags": mp.WRITE_NO_DELTA}, r))
    return out


@pytest.mark.parametrize("name", [c["name"] for c in wc.pack_cases()])
def test_pack_write_gives_the_models_bytes(eng, name):
    from decompress_amd import pack as mp
    case = next(c for c in wc.pack_cases() if c["name"] == name)
    for kw, r in _runs(case):
        rc, pack, need, entries, res = mp.write_raw(case["objects"], case["bases"], **kw)
        assert rc == 0 and need == len(r["pack"]), (name, kw)
        assert pack == r["pack"], (name, kw)
        assert entries == r["entries"], (name, kw)
        assert res == {"n": len(case["objects"]), "deltas": sum(r["keep"]), "max_depth": max(r["depth"] or [0])}, (name, kw)
        last = mp.write_last()
        assert {k: last[k] for k in r["last"]} == r["last"], (name, kw)
        if case["objects"]:
            assert last["launches"] == 2 + (2 if r["last"]["pairs"] else 0) and (last["delta_ns"] > 0) == (r["last"]["pairs"] > 0), (name, kw)
        # round trip within the library
        if r["idx"] is None:
            with pytest.raises(Exception, match="Invalid index"):
                mp.write_index(entries, pack[-20:])
            continue
        idx = mp.write_index(entries, pack[-20:])
        assert idx == r["idx"], (name, kw)
        assert mp.build_index(pack) == idx, (name, kw)
        p = mp.Pack(pack, idx)
        got = p.read(verify_crc=True, verify_names=True)
        where = {e["name"]: i for i, e in enumerate(mp.index(idx)[0])}
        for (t, data), e in zip(case["objects"], entries):
            assert got[where[e["name"]]] == ("Ok", (t, data)), (name, kw)
        p.close()


def test_short_cap_returns_the_need(eng):
    from decompress_amd import pack as mp
    case = next(c for c in wc.pack_cases() if c["name"] == "a chain of 4")
    want = wc.pack_model(case["name"], 6)[3]["pack"]
    for cap in (0, 31, len(want) - 1):
        rc, pack, need, entries, _ = mp.write_raw(case["objects"], case["bases"], pack_cap=cap)
        assert (rc, need, pack, entries) == (2, len(want), b"", []), cap
    rc, pack, need, _, _ = mp.write_raw(case["objects"], case["bases"], pack_cap=len(want))
    assert rc == 0 and pack == want
    assert mp.write_raw([], [], pack_cap=31)[:3] == (2, b"", 32)
    assert mp.write_raw([], [], pack_cap=32)[1] == wc.pack_model("nothing", 6)[0]["pack"]


def test_invalid_arguments(eng):
    from decompress_amd import _lib
    from decompress_amd import pack as mp
    a, b = wc.rnd(200, 1), wc.rnd(200, 2)
    assert mp.write_raw([(3, a), (3, b)], [None, 1])[0] == -1  # base == i
    assert mp.write_raw([(3, a), (3, b)], [1, None])[0] == -1  # a later base
    assert mp.write_raw([(3, a), (2, b)], [None, 0])[0] == -1  # a base of another type
    assert mp.write_raw([(0, a)])[0] == -1 and mp.write_raw([(5, a)])[0] == -1 and mp.write_raw([(6, a)])[0] == -1
    assert mp.write_raw([(3, a)], flags=2)[0] == -1 and mp.write_raw([(3, a)], flags=3)[0] == -1
    assert mp.write_raw([(3, a)], level=10)[0] == -1 and mp.write_raw([(3, a)], level=-1)[0] == -1
    assert mp.write_raw([(3, a), (3, a[:100] + b)], [None, 0])[0] == 0
    lib = eng.lib
    src = (_lib.PackSource * 1)()
    src[0].off, src[0].len, src[0].base, src[0].type = 0, 0xFFFFFFF1, mp.NO_BASE, 3
    out, need, ents, res = ctypes.create_string_buffer(64), ctypes.c_size_t(0), (_lib.PackIndexEntry * 1)(), _lib.PackWriteResult()
    assert lib.md_pack_write(eng.ctx, 6, 0, 50, 1, src, a, len(a), out, 64, ctypes.byref(need), ents, ctypes.byref(res)) == -1
    src[0].off, src[0].len = 150, 51  # one byte beyond the source
    assert lib.md_pack_write(eng.ctx, 6, 0, 50, 1, src, a, len(a), out, 64, ctypes.byref(need), ents, ctypes.byref(res)) == -1
    src[0].len = 50
    assert lib.md_pack_write(eng.ctx, 6, 0, 50, 1, None, a, len(a), out, 64, ctypes.byref(need), ents, ctypes.byref(res)) == -1
    assert lib.md_pack_write(eng.ctx, 6, 0, 50, 1, src, a, len(a), out, 64, None, ents, ctypes.byref(res)) == -1
    assert lib.md_pack_write(eng.ctx, 6, 0, 50, 1, src, a, len(a), out, 64, ctypes.byref(need), None, ctypes.byref(res)) == -1
    assert lib.md_pack_write(eng.ctx, 6, 0, 50, 1, src, a, len(a), out, 64, ctypes.byref(need), ents, None) == -1


def test_python_write_and_make_deltas(eng):
    from decompress_amd import engine
    from decompress_amd import pack as mp
    case = next(c for c in wc.pack_cases() if c["name"] == "every type")
    want = wc.pack_model(case["name"], 6)[0]
    named = [(mp.TYPE_NAMES[t], d) for t, d in case["objects"]]
    assert mp.write(named, case["bases"]) == (want["pack"], want["idx"])
    assert mp.write_last()["kept"] == 4
    whole = dm.write_pack(case["objects"], case["bases"], deltas=False)
    assert mp.write(case["objects"], case["bases"], deltas=False) == (whole["pack"], whole["idx"])
    with pytest.raises(engine.Error, match="Invalid index"):  # two objects with one name
        mp.write([(3, b"same"), (3, b"same")])
    v = wc.delta_cases()[-1]["bufs"]
    pairs = [(v[0], v[1]), (v[1], v[2]), (v[0], v[3])]
    got = mp.make_deltas(pairs)
    assert got == [dm.make_delta(b, t)[0] for b, t in pairs]
    assert [dm.apply_delta(b, d) for (b, _), d in zip(pairs, got)] == [t for _, t in pairs]
