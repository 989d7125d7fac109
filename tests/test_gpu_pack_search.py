"""Choosing a pack's delta bases on the GPU (md_pack_sketch_*, md_pack_delta_sizes_*, md_pack_choose_bases;
csrc/pack_search_kernels.hip).  Needs an MI355X: `pytest -m gpu`.  Yardstick: tests/pack_search_model.py and
tests/pack_delta_model.py - the header's definitions in Python, checked on the CPU (test_pack_search_model.py) - held to
exactly: features, lengths, statuses, order, bases, counts and the written pack's bytes.  No tolerance anywhere."""
import ctypes
import faulthandler

import numpy as np
import pytest

from tests import pack_delta_model as dm
from tests import pack_search_cases as sc
from tests import pack_search_model as sm
from tests import pack_write_cases as wc

pytestmark = pytest.mark.gpu
LEVELS = (1, 6)
TIME_LIMIT = 120  # seconds a test may take before the process is ended (each takes a few)


@pytest.fixture(autouse=True)
def time_limit():
    faulthandler.dump_traceback_later(TIME_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def eng():
    from decompress_amd import engine
    return engine.default_engine(0)


@pytest.fixture(scope="module")
def sketches():
    """every sketch case in one blob at every alignment, the last ending on the blob's last byte: (blob, rows, features, names)"""
    cases = sc.sketch_cases()
    blob, rows = sc.laid_out([c["data"] for c in cases])
    return blob, rows, [f for f, _ in sc.sketch_model()], [c["name"] for c in cases]


def test_features_host_form(eng, sketches):
    blob, rows, want, names = sketches
    got = eng.pack_sketch(blob, rows)
    for g, w, name in zip(got, want, names):
        assert g == w, name
    for row, w, name in zip(rows, want, names):
        assert eng.pack_sketch(blob, [row]) == [w], name
    assert eng.pack_sketch(blob, []) == [] and eng.pack_sketch(b"", [(0, 0)]) == [sm.NONE]
    # the features do not depend on what stands around an object or on its address
    data = sc.sketch_cases()[-1]["data"]
    assert eng.pack_sketch(data, [(0, len(data))]) == [want[-1]]


def test_features_device_form(eng, sketches):
    import torch
    blob, rows, want, names = sketches
    d_src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(eng.device)
    got = eng.pack_sketch_device(rows, d_src)
    eng.synchronize()
    got = [int(v) & 0xFFFFFFFF for v in got.cpu().tolist()]
    for k, (w, name) in enumerate(zip(want, names)):
        assert tuple(got[4 * k:4 * k + 4]) == w, name
    for row, w, name in zip(rows, want, names):
        one = eng.pack_sketch_device([row], d_src)
        eng.synchronize()
        assert tuple(int(v) & 0xFFFFFFFF for v in one.cpu().tolist()) == w, name


@pytest.fixture(scope="module")
def family():
    """every pair of every delta case of the writer's tests in one blob: (blob, rows, [len(model delta)], names)"""
    cases = wc.delta_cases()
    blob, rows, who = wc.laid_out(cases)
    models = [wc.delta_model(c)[1] for c in cases]
    return blob, rows, [len(models[ci][pi]) for ci, pi in who], ["%s / %d" % (cases[ci]["name"], pi) for ci, pi in who]


def _want_sizes(lens, caps):
    return [(dm.MD_OK, n) if n <= cap else (dm.MD_UNEXPECTED_END_OF_OUTPUT, 0) for n, cap in zip(lens, caps)]


def test_delta_sizes_host_form(eng, family):
    blob, rows, lens, names = family
    for short in (0, 1):
        caps = [max(n - short, 0) for n in lens]
        got = eng.pack_delta_sizes(blob, rows, caps)
        for g, w, name in zip(got, _want_sizes(lens, caps), names):
            assert g == w, (name, short)
        last = eng.pack_write_last()
        assert last["pairs"] == len(rows) and last["launches"] == 2 and last["delta_ns"] > 0
        made = eng.pack_deltas(blob, rows, caps)  # md_pack_delta_batch_host on the same rows
        assert [(st, len(d)) for st, d in made] == got, short
    assert eng.pack_delta_sizes(blob, rows) == [(dm.MD_OK, n) for n in lens]
    assert eng.pack_delta_sizes(blob, []) == []
    for row, n, name in zip(rows, lens, names):  # one pair at a time
        assert eng.pack_delta_sizes(blob, [row], [n]) == [(dm.MD_OK, n)], name


def test_delta_sizes_device_form(eng, family):
    import torch
    blob, rows, lens, names = family
    d_src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(eng.device)
    for short in (0, 1):
        caps = [max(n - short, 0) for n in lens]
        out_len, status = eng.pack_delta_sizes_device([r + (c,) for r, c in zip(rows, caps)], d_src)
        eng.synchronize()
        got = list(zip(status.cpu().tolist(), out_len.cpu().tolist()))
        for g, w, name in zip(got, _want_sizes(lens, caps), names):
            assert g == w, (name, short)
        assert eng.pack_write_last()["delta_ns"] > 0


def test_a_sketch_leaves_the_writers_stats_alone(eng):
    """md_pack_write_last after a device-form delta batch and a stand-alone sketch behind it: the batch's counts, a time, and
    the same answer when asked again (the sketch records into no span of the batch's)"""
    import torch
    a = wc.rnd(600, 31)
    blob = a + a[:300] + a[100:500]
    d_src = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(eng.device)
    d_out = torch.zeros(512, dtype=torch.uint8, device=eng.device)
    _, status = eng.pack_deltas_device([(0, 600, 600, 300, 0, 256), (0, 600, 900, 400, 256, 256)], d_src, d_out)
    assert len(eng.pack_sketch(blob, [(0, 600), (600, 300), (900, 400)])) == 3
    last = eng.pack_write_last()
    assert last["pairs"] == 2 and last["launches"] == 2 and last["delta_ns"] > 0
    assert eng.pack_write_last() == last
    assert status.cpu().tolist() == [dm.MD_OK, dm.MD_OK]


def _written(mp, objects, bases, level, max_depth):
    rc, pack, need, entries, res = mp.write_raw(objects, bases, level=level, max_depth=max_depth)
    assert rc == 0 and need == len(pack)
    return pack, entries, res


@pytest.mark.parametrize("name", [c["name"] for c in sc.search_cases()])
def test_choose_bases_gives_the_models_choice(eng, name):
    from decompress_amd import pack as mp
    case = sc.case(name)
    for run, (trace, max_depth) in enumerate(zip(sc.search_model(name), case["runs"])):
        rc, order, bases = mp.choose_bases_raw(case["objects"], case["window"], max_depth)
        assert rc == 0, (name, max_depth)
        assert order == trace["order"] and bases == trace["bases"], (name, max_depth)
        last = mp.search_last()
        assert {k: last[k] for k in trace["last"]} == trace["last"], (name, max_depth)
        assert last["launches"] == sm.launches(trace), (name, max_depth)
        assert (last["sketch_ns"] > 0) == (trace["last"]["featured"] > 0) and (last["score_ns"] > 0) == (len(trace["pairs"]) > 0), (name, last)
        objects = [case["objects"][i] for i in order]
        for level in LEVELS:
            want = sc.pack_model(name, level)[run]
            pack, entries, res = _written(mp, objects, bases, level, max_depth)
            assert pack == want["pack"] and entries == want["entries"], (name, max_depth, level)
            assert res == {"n": len(objects), "deltas": trace["last"]["chosen"], "max_depth": max(trace["depth"] or [0])}, (name, max_depth, level)
            wl = mp.write_last()
            assert wl["dropped_size"] == wl["dropped_depth"] == 0 and wl["kept"] == trace["last"]["chosen"], (name, max_depth, level)
            if want["idx"] is None:  # two objects with one name
                continue
            idx = mp.write_index(entries, pack[-20:])
            assert idx == want["idx"] and mp.build_index(pack) == idx, (name, max_depth, level)
            p = mp.Pack(pack, idx)
            got = p.read(verify_crc=True, verify_names=True)
            where = {e["name"]: i for i, e in enumerate(mp.index(idx)[0])}
            for (t, data), e in zip(objects, entries):
                assert got[where[e["name"]]] == ("Ok", (t, data)), (name, max_depth, level)
            p.close()


def test_python_write_with_search(eng):
    from decompress_amd import pack as mp
    case = sc.case("a chain of five")
    trace, want = sc.search_model(case["name"])[2], sc.pack_model(case["name"], 6)[2]
    named = [(mp.TYPE_NAMES[t], d) for t, d in case["objects"]]
    assert mp.choose_bases(named, max_depth=0) == (trace["order"], trace["bases"])
    pack, idx = mp.write(named, bases="search", max_depth=0)
    assert (pack, idx) == (want["pack"], want["idx"])
    p = mp.Pack(pack, idx)
    got = p.read(verify_crc=True, verify_names=True)
    assert sorted(d for st, (_, d) in got if st == "Ok") == sorted(d for _, d in case["objects"]) and len(got) == 5
    assert [o["depth"] for o in sorted(p.objects, key=lambda o: o["offset"])] == trace["depth"]
    p.close()
    # every other value of bases behaves as before
    assert mp.write(case["objects"], None) == mp.write(case["objects"])
    with pytest.raises(ValueError):
        mp.write(case["objects"], bases="window")


def test_invalid_arguments(eng):
    from decompress_amd import _lib
    from decompress_amd import pack as mp
    a = wc.rnd(200, 1)
    objs = [(3, a), (3, a[:100])]
    assert mp.choose_bases_raw(objs, window=0)[0] == -1 and mp.choose_bases_raw(objs, window=65)[0] == -1
    assert mp.choose_bases_raw(objs, window=1)[0] == 0 and mp.choose_bases_raw(objs, window=64)[0] == 0
    assert mp.choose_bases_raw([(0, a)])[0] == -1 and mp.choose_bases_raw([(5, a)])[0] == -1
    assert mp.choose_bases_raw([]) == (0, [], []) and mp.search_last()["launches"] == 0
    lib = eng.lib
    src, out, order = (_lib.PackSource * 1)(), (_lib.PackSource * 1)(), (ctypes.c_uint64 * 1)()
    src[0].off, src[0].len, src[0].base, src[0].type = 150, 51, 77, 3  # one byte beyond the source
    assert lib.md_pack_choose_bases(eng.ctx, 4, 50, 1, src, a, len(a), out, order) == -1
    src[0].len = 50
    assert lib.md_pack_choose_bases(eng.ctx, 4, 50, 1, src, a, len(a), out, order) == 0  # (base is not looked at)
    assert lib.md_pack_choose_bases(eng.ctx, 4, 50, 1, None, a, len(a), out, order) == -1
    assert lib.md_pack_choose_bases(eng.ctx, 4, 50, 1, src, a, len(a), None, order) == -1
    assert lib.md_pack_choose_bases(eng.ctx, 4, 50, 1, src, a, len(a), out, None) == -1
    # n * 4 * window above 2^31 - 16 is refused before anything is read
    assert lib.md_pack_choose_bases(eng.ctx, 64, 50, (0x7FFFFFF0 // 256) + 1, src, a, len(a), out, order) == -1
    assert lib.md_pack_choose_bases(eng.ctx, 1, 50, (0x7FFFFFF0 // 4) + 1, src, a, len(a), out, order) == -1
    # the sketch and the sizes: ranges that leave the source
    one, two, feats = (ctypes.c_uint64 * 1)(150), (ctypes.c_uint64 * 1)(51), (ctypes.c_uint32 * 4)()
    assert lib.md_pack_sketch_host(eng.ctx, 1, one, two, a, len(a), feats) == -1
    two[0] = 50
    assert lib.md_pack_sketch_host(eng.ctx, 1, one, two, a, len(a), feats) == 0
    assert lib.md_pack_sketch_host(eng.ctx, 1, None, two, a, len(a), feats) == -1
    assert lib.md_pack_sketch_host(eng.ctx, 1, one, two, a, len(a), None) == -1
    pair, n64, n32 = (_lib.PackDeltaPair * 1)(), (ctypes.c_uint64 * 1)(), (ctypes.c_int32 * 1)()
    pair[0].base_off, pair[0].base_len, pair[0].tgt_off, pair[0].tgt_len, pair[0].out_off, pair[0].out_cap = 0, 100, 100, 101, (1 << 64) - 1, 64
    assert lib.md_pack_delta_sizes_host(eng.ctx, 1, pair, a, len(a), n64, n32) == -1  # the target leaves src
    pair[0].tgt_len = 100
    assert lib.md_pack_delta_sizes_host(eng.ctx, 1, pair, a, len(a), n64, n32) == 0  # (out_off is not looked at)
    assert lib.md_pack_delta_sizes_host(eng.ctx, 1, None, a, len(a), n64, n32) == -1
    assert lib.md_pack_delta_sizes_host(eng.ctx, 1, pair, a, len(a), None, n32) == -1
