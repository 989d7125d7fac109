"""A git packfile read on one GPU, host to host, for DESIGN 4i.  The pack is written by tests/pack_writer.py from the
corpus as version chains: `--objects` objects in chains of `--depth` deltas on a whole object, each version a small edit
(a copy, an insert, a copy) of the one before it and stored as an OFS_DELTA against it; `--mib` is the total of the
objects' sizes.

  open        md_pack_open: idx, headers, chains, the deltas' sizes (their payloads inflated once)
  read_all    md_pack_read of every object
  read_1pct   md_pack_read of 1 % of the objects, chosen at random (and the bases they hang off)
  payloads    md_inflate_batch_host over the same pack's zlib streams alone: what a caller could do before there was
              md_pack_read - it yields the whole objects and the deltas' PAYLOADS, not the objects
  git         `git cat-file --batch-all-objects --batch` over the same pack, one CPU process, if git is on the machine
With read_all the share of its time that the apply launches take on the device (md_pack_last's apply_ns over the median).

With --names, for DESIGN 4j, further legs on the same pack:
  read_names    md_pack_read of every object with MD_PACK_VERIFY_NAME (beside read_all, which is the same call without)
  verify        md_pack_verify of every object with MD_PACK_VERIFY_CRC | MD_PACK_VERIFY_NAME: nothing comes back but statuses
  hashlib       hashlib.sha1 over "<type> <size>\0" + content of the same objects, one CPU thread of this machine
  git verify-pack, git fsck   over the same pack, if git is on the machine
and with read_names and verify the device time of their hash passes (md_sha1_last's device_ns) and its counts.

With --build, for DESIGN 4k, the idx from the pack alone:
  build, build_no_trailer   md_pack_index_build with and without MD_PACK_BUILD_CHECK_TRAILER; the idx is compared with the writer's
  verify                    what it cannot beat: md_pack_verify with both flags, given the idx (beside open)
  count                     md_inflate_sizes_batch_host over the same candidates (found here with numpy): the count pass, with
                            its own copy of the pack to the device
  trailer_hash, idx_write   md_pack_check_trailers (the host's SHA-1 over the pack and the idx) and md_pack_index_write alone
  git index-pack            over the same pack, one CPU process, if git is on the machine
and md_pack_build_last's counts (candidates against n, generations).

With --write, for DESIGN 4l, instead of the read legs: the same objects written as a pack again, the chains as bases:
  write               md_pack_write (level 6, max_depth 50) with every version's predecessor as its base
  write_no_delta      the same with MD_PACK_WRITE_NO_DELTA
  deflate_batch_host  md_deflate_batch_host over the same objects: what a caller could do before - payloads, not a pack
  git pack-objects    --window=10 --depth=50 on this machine's CPU from a scratch repository filled by git unpack-objects, if git
                      is on the machine; a yardstick of another shape: it also searches the bases
and the three packs' sizes, md_pack_write_last's counts and the device time of the index and delta launches.  Both written
packs are read back by md_pack_index_build and md_pack_read with both checks and compared with the objects.

With --search, for DESIGN 4m, instead of the read legs: the same objects in SHUFFLED order, as a caller has them who knows no bases:
  choose              md_pack_choose_bases alone (window 4, max_depth 50)
  choose_write        md_pack_choose_bases, then md_pack_write (level 6) on what it returned
  write_true          md_pack_write with every version's true predecessor as its base, the objects in the chains' order
  write_no_delta      md_pack_write with MD_PACK_WRITE_NO_DELTA: what a caller without bases had before
  git pack-objects    as with --write
and the packs' sizes, how many chosen bases are the target's true predecessor or of its chain, and md_pack_search_last's split:
the sketch launch, the index and size launches, the host's grouping and choice.  The searched pack is read back by
md_pack_index_build and md_pack_read with both checks and compared with the objects.

    python tools/bench_pack.py [--objects 16384] [--depth 8] [--mib 64] [--reps 7] [--warmup 1] [--names] [--build] [--write] [--search]

The legs are alternated in one process; every leg reports the median and the spread (min .. max) of its repeats, host to
host (perf_counter around a call that ends in a synchronise).  read_all's bytes are compared with the writer's."""
import argparse
import ctypes
import hashlib
import json
import os
import random
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from decompress_amd import _lib, workloads  # noqa: E402
from decompress_amd import engine as _engine  # noqa: E402
from decompress_amd import pack as mp  # noqa: E402
from tests import pack_writer as pw  # noqa: E402


def stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "n": len(v)}


def version_chains(objects, depth, size):
    """entries for pack_writer: chains of a blob and `depth` deltas, each delta against the version before it"""
    entries = []
    chain = 0
    while len(entries) < objects:
        cur = workloads.corpus_slice(chain, size)
        entries.append({"type": 3, "data": cur + b"%d" % chain})  # (the number: no two chains with one name)
        cur = entries[-1]["data"]
        for k in range(1, depth + 1):
            if len(entries) == objects:
                break
            at = (37 * k + 101 * chain) % (len(cur) - 40) + 1
            ins = [("copy", 0, at), ("insert", b"<%d.%d>" % (chain, k)), ("copy", at + 3, len(cur) - at - 3)]
            entries.append({"delta": "ofs", "base": len(entries) - 1, "ins": ins})
            cur = pw._result(cur, ins)
        chain += 1
    return entries


def time_git(pack, idx, reps):
    git = shutil.which("git")
    if not git:
        return None
    env = dict(os.environ, GIT_CONFIG_GLOBAL="/dev/null", GIT_CONFIG_SYSTEM="/dev/null")
    with tempfile.TemporaryDirectory() as tmp:
        repo = os.path.join(tmp, "r.git")
        subprocess.run([git, "init", "-q", "--bare", repo], check=True, env=env, capture_output=True)
        stem = os.path.join(repo, "objects", "pack", "pack-" + pack[-20:].hex())
        for ext, data in ((".pack", pack), (".idx", idx)):
            with open(stem + ext, "wb") as f:
                f.write(data)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = subprocess.run([git, "-C", repo, "cat-file", "--batch-all-objects", "--batch"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            times.append((time.perf_counter() - t0) * 1e3)
            assert r.returncode == 0, r.stderr
        return times


def time_git_checks(pack, idx, reps):
    """git verify-pack and git fsck over the pack -> {name: times} or None"""
    git = shutil.which("git")
    if not git:
        return None
    env = dict(os.environ, GIT_CONFIG_GLOBAL="/dev/null", GIT_CONFIG_SYSTEM="/dev/null")
    with tempfile.TemporaryDirectory() as tmp:
        repo = os.path.join(tmp, "r.git")
        subprocess.run([git, "init", "-q", "--bare", repo], check=True, env=env, capture_output=True)
        stem = os.path.join(repo, "objects", "pack", "pack-" + pack[-20:].hex())
        for ext, data in ((".pack", pack), (".idx", idx)):
            with open(stem + ext, "wb") as f:
                f.write(data)
        out = {}
        for name, cmd in (("git_verify_pack", ["verify-pack", stem + ".idx"]), ("git_fsck", ["fsck", "--no-dangling", "--no-progress"])):
            out[name] = []
            for _ in range(reps):
                t0 = time.perf_counter()
                r = subprocess.run([git, "-C", repo] + cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
                out[name].append((time.perf_counter() - t0) * 1e3)
                assert r.returncode == 0, r.stderr
        return out


def time_git_index_pack(pack, reps):
    git = shutil.which("git")
    if not git:
        return None
    env = dict(os.environ, GIT_CONFIG_GLOBAL="/dev/null", GIT_CONFIG_SYSTEM="/dev/null")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "x.pack")
        with open(path, "wb") as f:
            f.write(pack)
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = subprocess.run([git, "index-pack", "-o", os.path.join(tmp, "x.idx"), path], env=env, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            times.append((time.perf_counter() - t0) * 1e3)
            assert r.returncode == 0, r.stderr
        with open(os.path.join(tmp, "x.idx"), "rb") as f:
            return times, f.read()


def time_git_pack_objects(pack, reps):
    """git pack-objects --window=10 --depth=50 over the objects of `pack`, from a scratch repository filled by git
    unpack-objects -> (times, the pack's length) or None"""
    git = shutil.which("git")
    if not git:
        return None
    env = dict(os.environ, GIT_CONFIG_GLOBAL="/dev/null", GIT_CONFIG_SYSTEM="/dev/null")
    with tempfile.TemporaryDirectory() as tmp:
        repo = os.path.join(tmp, "r.git")
        subprocess.run([git, "init", "-q", "--bare", repo], check=True, env=env, capture_output=True)
        subprocess.run([git, "-C", repo, "unpack-objects", "-q"], input=pack, check=True, env=env, capture_output=True)
        names = subprocess.run([git, "-C", repo, "cat-file", "--batch-all-objects", "--batch-check=%(objectname)"], check=True, env=env,
                               capture_output=True).stdout
        times, size = [], 0
        for _ in range(reps):
            t0 = time.perf_counter()
            r = subprocess.run([git, "-C", repo, "pack-objects", "--window=10", "--depth=50", "--stdout", "-q"], input=names, env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            times.append((time.perf_counter() - t0) * 1e3)
            assert r.returncode == 0, r.stderr
            size = len(r.stdout)
        return times, size


def write_mode(a, eng, entries, layout):
    """--write, for DESIGN 4l: the objects of the read benchmark's pack written again on the device, the chains as bases"""
    lib, n = eng.lib, len(layout)
    blob = np.frombuffer(b"".join(lay["data"] for lay in layout), dtype=np.uint8)
    lens = np.array([len(lay["data"]) for lay in layout], dtype=np.uint64)
    offs = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64)
    src = (_lib.PackSource * n)()
    for s, e, o, ln in zip(src, entries, offs, lens):
        s.off, s.len, s.type, s.base = int(o), int(ln), 3, mp.NO_BASE if e.get("base") is None else e["base"]
    bound = int(lib.md_pack_write_bound(n, src))
    out = np.empty(bound, dtype=np.uint8)
    ents, need, res = (_lib.PackIndexEntry * n)(), ctypes.c_size_t(0), _lib.PackWriteResult()
    made, last = {}, {}

    def write_with(name, flags):
        def run():
            eng._check(lib.md_pack_write(eng.ctx, 6, flags, 50, n, src, blob.ctypes.data, blob.size, out.ctypes.data, out.size, ctypes.byref(need), ents,
                                         ctypes.byref(res)))
            last[name] = mp.write_last()
            if name not in made:
                made[name] = (out[:need.value].tobytes(), [{"name": bytes(e.name), "offset": e.offset, "crc32": e.crc32} for e in ents], res.deltas)
        return run

    caps = np.array([int(lib.md_zl_def_ns_compress_bound(int(ln))) + 64 + int(ln) // 8 for ln in lens], dtype=np.uint64)
    z_off = np.concatenate(([0], np.cumsum(caps)[:-1])).astype(np.uint64)
    z_out = np.empty(int(caps.sum()) + 1, dtype=np.uint8)
    z = {}

    def payloads():
        z["len"], z["status"], _ = eng.deflate_batch_host(_engine.FORMAT_ZLIB, blob, offs, lens, z_out, z_off, caps, level=6)

    legs = {"write": write_with("write", 0), "write_no_delta": write_with("write_no_delta", mp.WRITE_NO_DELTA), "deflate_batch_host": payloads}
    times = {k: [] for k in legs}
    for r in range(a.warmup + a.reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            if r >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    assert not z["status"].any()
    sizes = {}
    for name, (pack, entries_out, deltas) in made.items():  # what was written is a pack: the library's own reader takes it back
        idx = mp.write_index(entries_out, pack[-20:])
        assert mp.build_index(pack) == idx
        p = mp.Pack(pack, idx)
        got = p.read(verify_crc=True, verify_names=True)
        where = {e["name"]: i for i, e in enumerate(mp.index(idx)[0])}
        assert all(got[where[lay["name"]]] == ("Ok", (3, lay["data"])) for lay in layout), name
        sizes[name] = {"pack_bytes": len(pack), "deltas": int(deltas), "max_depth": p.info["max_depth"]}
        p.close()
    out_res = {"mode": "write", "objects": n, "depth": a.depth, "object_bytes": int(lens[0]), "total_size": int(lens.sum()), "level": 6, "reps": a.reps,
               "warmup": a.warmup, "times": {k: stats(v) for k, v in times.items()}, "packs": sizes, "payloads_bytes": int(z["len"].sum()), "last": last,
               "delta_launches_device_ms": round(last["write"]["delta_ns"] / 1e6, 4)}
    git = time_git_pack_objects(made["write"][0], min(a.reps, 3))
    if git:
        out_res["git_pack_objects"] = dict(stats(git[0]), pack_bytes=git[1])
    else:
        out_res["git_pack_objects"] = "git is not on this machine: this leg was not run"
    print(json.dumps(out_res))


def search_mode(a, eng, entries, layout):
    """--search, for DESIGN 4m: the objects of the read benchmark's pack in shuffled order, the bases chosen on the device"""
    lib, n = eng.lib, len(layout)
    perm = list(range(n))
    random.Random(7).shuffle(perm)
    chain_of, c = [], -1
    for e in entries:
        c += e.get("base") is None
        chain_of.append(c)

    def sources(idx, with_bases):
        blob = np.frombuffer(b"".join(layout[i]["data"] for i in idx), dtype=np.uint8)
        src, at = (_lib.PackSource * n)(), 0
        for s, i in zip(src, idx):
            s.off, s.len, s.type = at, len(layout[i]["data"]), 3
            s.base = entries[i]["base"] if with_bases and entries[i].get("base") is not None else mp.NO_BASE
            at += s.len
        return blob, src

    sh_blob, sh_src = sources(perm, False)
    tr_blob, tr_src = sources(range(n), True)
    sorted_src, order = (_lib.PackSource * n)(), (ctypes.c_uint64 * n)()
    out = np.empty(int(lib.md_pack_write_bound(n, tr_src)), dtype=np.uint8)
    ents, need, res = (_lib.PackIndexEntry * n)(), ctypes.c_size_t(0), _lib.PackWriteResult()
    made, last = {}, {}

    def choose():
        eng._check(lib.md_pack_choose_bases(eng.ctx, a.window, 50, n, sh_src, sh_blob.ctypes.data, sh_blob.size, sorted_src, order))
        last["search"] = mp.search_last()

    def write(name, src, blob, flags):
        eng._check(lib.md_pack_write(eng.ctx, 6, flags, 50, n, src, blob.ctypes.data, blob.size, out.ctypes.data, out.size, ctypes.byref(need), ents,
                                     ctypes.byref(res)))
        last[name] = mp.write_last()
        if name not in made:
            made[name] = (out[:need.value].tobytes(), [{"name": bytes(e.name), "offset": e.offset, "crc32": e.crc32} for e in ents], int(res.deltas),
                          int(res.max_depth))

    def choose_write():
        choose()
        write("choose_write", sorted_src, sh_blob, 0)

    legs = {"choose": choose, "choose_write": choose_write, "write_true": lambda: write("write_true", tr_src, tr_blob, 0),
            "write_no_delta": lambda: write("write_no_delta", sh_src, sh_blob, mp.WRITE_NO_DELTA)}
    times = {k: [] for k in legs}
    for r in range(a.warmup + a.reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            if r >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    # what the search chose, against the chains the objects were made as
    ranks = [perm[int(i)] for i in order]  # rank -> the object's index in the chains' order
    chosen = [(ranks[r], ranks[int(s.base)]) for r, s in enumerate(sorted_src) if s.base != mp.NO_BASE]
    quality = {"chosen": len(chosen), "true_predecessor": sum(entries[t].get("base") == b for t, b in chosen),
               "true_successor": sum(entries[b].get("base") == t for t, b in chosen), "own_chain": sum(chain_of[t] == chain_of[b] for t, b in chosen),
               "possible": sum(e.get("base") is not None for e in entries)}
    pack, entries_out, deltas, depth = made["choose_write"]  # what was written is a pack: the library's own reader takes it back
    idx = mp.write_index(entries_out, pack[-20:])
    assert mp.build_index(pack) == idx and deltas == len(chosen) and last["choose_write"]["dropped_size"] == last["choose_write"]["dropped_depth"] == 0
    p = mp.Pack(pack, idx)
    got = p.read(verify_crc=True, verify_names=True)
    where = {e["name"]: i for i, e in enumerate(mp.index(idx)[0])}
    assert all(got[where[lay["name"]]] == ("Ok", (3, lay["data"])) for lay in layout)
    p.close()
    sizes = {k: {"pack_bytes": len(v[0]), "deltas": v[2], "max_depth": v[3]} for k, v in made.items()}
    med = {k: statistics.median(v) for k, v in times.items()}
    s = last["search"]
    out_res = {"mode": "search", "objects": n, "depth": a.depth, "object_bytes": len(layout[0]["data"]), "total_size": int(sh_blob.size), "window": a.window,
               "level": 6, "reps": a.reps, "warmup": a.warmup, "times": {k: stats(v) for k, v in times.items()}, "packs": sizes, "quality": quality, "last": last,
               "search_split_ms": {"sketch_device": round(s["sketch_ns"] / 1e6, 4), "index_and_sizes_device": round(s["score_ns"] / 1e6, 4),
                                   "host_grouping_and_choice": round(s["host_ns"] / 1e6, 4), "choose_median": round(med["choose"], 3)},
               "choose_write_over_write_true": round(med["choose_write"] / med["write_true"], 3),
               "write_no_delta_over_choose_write": round(med["write_no_delta"] / med["choose_write"], 3),
               "searched_pack_over_true_pack": round(sizes["choose_write"]["pack_bytes"] / sizes["write_true"]["pack_bytes"], 4)}
    git = time_git_pack_objects(made["write_true"][0], min(a.reps, 3))
    if git:
        out_res["git_pack_objects"] = dict(stats(git[0]), pack_bytes=git[1])
    else:
        out_res["git_pack_objects"] = "git is not on this machine: this leg was not run"
    print(json.dumps(out_res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=16384)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--names", action="store_true")
    ap.add_argument("--build", action="store_true")
    ap.add_argument("--write", action="store_true")
    ap.add_argument("--search", action="store_true")
    ap.add_argument("--window", type=int, default=4)
    a = ap.parse_args()
    eng = _engine.default_engine(0)
    lib = eng.lib
    size = max(64, (a.mib << 20) // a.objects)
    entries = version_chains(a.objects, a.depth, size)
    pack, idx, layout = pw.write_pack(entries)
    if a.write:
        return write_mode(a, eng, entries, layout)
    if a.search:
        return search_mode(a, eng, entries, layout)
    order = pw.idx_order(layout)
    p = mp.Pack(pack, idx)
    n = p.info["n"]
    assert n == a.objects and p.info["failed"] == 0 and p.info["max_depth"] == min(a.depth, n - 1)
    total = p.info["total_size"]

    def opened():
        h = ctypes.c_void_p()
        eng._check(lib.md_pack_open(eng.ctx, pack, len(pack), idx, len(idx), ctypes.byref(h)))
        lib.md_pack_free(h)

    rng = random.Random(3)
    some = sorted(rng.sample(range(n), max(1, n // 100)))
    last = {}
    calls = {}
    for name, sel in (("read_all", None), ("read_1pct", some)):
        k = n if sel is None else len(sel)
        sizes = [p.objects[i]["size"] for i in (range(n) if sel is None else sel)]
        dst = np.empty(max(sum(sizes), 1), dtype=np.uint8)  # (a buffer that exists: no first-touch page faults timed)
        arr = None if sel is None else np.array(sel, dtype=np.uint64)
        out_off, status, res = np.zeros(k + 1, dtype=np.uint64), np.zeros(k, dtype=np.int32), _lib.PackResult()

        def read(arr=arr, k=k, dst=dst, out_off=out_off, status=status, res=res, name=name):
            eng._check(lib.md_pack_read(eng.ctx, p._h, pack, len(pack), arr.ctypes.data if arr is not None else None, k, 0, dst.ctypes.data, dst.size,
                                        out_off.ctypes.data, status.ctypes.data, ctypes.byref(res)))
            last[name] = p.last()

        calls[name] = (read, dst, out_off, status)
    # the same streams through the batch decoder alone
    objs = p.objects
    in_off = np.array([o["offset"] + o["packed_len"] - len(_zlib_of(pack, o)) for o in objs], dtype=np.uint64)
    in_len = np.array([len(_zlib_of(pack, o)) for o in objs], dtype=np.uint64)
    caps = np.array([_header_size(pack, o) for o in objs], dtype=np.uint64)
    p_off = np.concatenate(([0], np.cumsum(caps)[:-1])).astype(np.uint64)
    h_in = np.frombuffer(pack, dtype=np.uint8)
    h_out = np.empty(int(caps.sum()) + 1, dtype=np.uint8)
    out_len, consumed, pst = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int32)

    def payloads():
        eng._check(lib.md_inflate_batch_host(eng.ctx, _engine.FORMAT_ZLIB, n, h_in.ctypes.data, h_in.size, in_off.ctypes.data, in_len.ctypes.data,
                                             h_out.ctypes.data, h_out.size, p_off.ctypes.data, caps.ctypes.data, out_len.ctypes.data,
                                             consumed.ctypes.data, pst.ctypes.data, None))

    legs = {"open": opened, "payloads": payloads}
    legs.update({k: v[0] for k, v in calls.items()})
    hashed = {}
    if a.names:
        _, dst_all, off_all, _ = calls["read_all"]
        st_names, st_verify, res_n, res_v = np.ones(n, dtype=np.int32), np.ones(n, dtype=np.int32), _lib.PackResult(), _lib.PackResult()

        def read_names():
            eng._check(lib.md_pack_read(eng.ctx, p._h, pack, len(pack), None, n, mp.VERIFY_NAMES, dst_all.ctypes.data, dst_all.size,
                                        off_all.ctypes.data, st_names.ctypes.data, ctypes.byref(res_n)))
            hashed["read_names"] = eng.sha1_last()

        def verify():
            eng._check(lib.md_pack_verify(eng.ctx, p._h, pack, len(pack), None, n, mp.VERIFY_CRC | mp.VERIFY_NAMES, st_verify.ctypes.data,
                                          ctypes.byref(res_v)))
            hashed["verify"] = eng.sha1_last()

        legs.update({"read_names": read_names, "verify": verify})
    built = {}
    if a.build:
        b = np.frombuffer(pack, dtype=np.uint8)
        hi = len(pack) - 20 - 6
        cmf, flg = b[12:hi + 1].astype(np.uint32), b[13:hi + 2].astype(np.uint32)
        cand = (np.nonzero(((cmf & 15) == 8) & (((cmf << 8) + flg) % 31 == 0))[0] + 12).astype(np.uint64)
        c_len = np.minimum(np.uint64(len(pack) - 20) - cand, np.uint64(0x1ffffff0)).astype(np.uint64)
        c_out, c_used, c_st = np.zeros(cand.size, dtype=np.uint64), np.zeros(cand.size, dtype=np.uint64), np.zeros(cand.size, dtype=np.int32)
        idx_buf = np.zeros(len(idx), dtype=np.uint8)
        b_off, b_st, b_res = np.zeros(n, dtype=np.uint64), np.ones(n, dtype=np.int32), _lib.PackBuildResult()

        def build_with(flags):
            def run():
                eng._check(lib.md_pack_index_build(eng.ctx, pack, len(pack), flags, idx_buf.ctypes.data, idx_buf.size, b_off.ctypes.data,
                                                   b_st.ctypes.data, n, ctypes.byref(b_res)))
                built["last"] = mp.build_last()
            return run

        def count():
            eng._check(lib.md_inflate_sizes_batch_host(eng.ctx, _engine.FORMAT_ZLIB, cand.size, h_in.ctypes.data, h_in.size, cand.ctypes.data,
                                                       c_len.ctypes.data, c_out.ctypes.data, c_used.ctypes.data, c_st.ctypes.data))

        ents, info = mp.index(idx)
        c_ents = (_lib.PackIndexEntry * max(n, 1))()
        for e, d in zip(c_ents, ents):
            e.offset, e.crc32 = d["offset"], d["crc32"]
            e.name[:] = d["name"]
        w_buf, w_len, ok = ctypes.create_string_buffer(len(idx)), ctypes.c_size_t(0), (ctypes.c_int(0), ctypes.c_int(0))

        def idx_write():
            assert lib.md_pack_index_write(c_ents, n, info["pack_checksum"], w_buf, len(idx), ctypes.byref(w_len)) == 0

        def trailer_hash():
            assert lib.md_pack_check_trailers(pack, len(pack), idx, len(idx), ctypes.byref(ok[0]), ctypes.byref(ok[1])) == 0

        legs.update({"build": build_with(mp.BUILD_CHECK_TRAILER), "build_no_trailer": build_with(0), "count": count, "idx_write": idx_write,
                     "trailer_hash": trailer_hash})
        if not a.names:
            st_v, res_b = np.ones(n, dtype=np.int32), _lib.PackResult()

            def verify_both():
                eng._check(lib.md_pack_verify(eng.ctx, p._h, pack, len(pack), None, n, mp.VERIFY_CRC | mp.VERIFY_NAMES, st_v.ctypes.data,
                                              ctypes.byref(res_b)))

            legs["verify"] = verify_both
    times = {k: [] for k in legs}
    for r in range(a.warmup + a.reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            if r >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    assert not pst.any() and np.array_equal(out_len, caps) and np.array_equal(consumed, in_len)
    _, dst, out_off, status = calls["read_all"]
    assert not status.any() and not calls["read_1pct"][3].any()
    raw = dst.tobytes()
    for k, lay in enumerate(layout):
        i = order[k]
        assert raw[int(out_off[i]):int(out_off[i + 1])] == lay["data"], k
    res = {"objects": n, "depth": a.depth, "object_bytes": size, "pack_bytes": len(pack), "total_size": total, "deltas": p.info["deltas"],
           "payload_bytes": int(caps.sum()), "reps": a.reps, "warmup": a.warmup, "times": {k: stats(v) for k, v in times.items()}, "last_stats": last}
    med = res["times"]["read_all"]["median_ms"]
    res["read_all_gib_s"] = round(total / 2**30 / (med / 1e3), 3)
    res["apply_share_of_read_all"] = round(last["read_all"]["apply_ns"] / 1e6 / med, 4)
    git = time_git(pack, idx, a.reps)
    res["git_cat_file"] = stats(git) if git else "git is not on this machine: no CPU figure"
    if a.names:
        assert not st_names.any() and not st_verify.any() and res_v.written == 0 and res_v.failed == 0
        heads = [pw.TYPE_NAMES[lay["type"]] + b" %d\0" % len(lay["data"]) for lay in layout]
        cpu = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            got = [hashlib.sha1(h + lay["data"]).digest() for h, lay in zip(heads, layout)]
            cpu.append((time.perf_counter() - t0) * 1e3)
        assert got == [lay["name"] for lay in layout]
        t = res["times"]
        res["names"] = {
            "hash_pass": hashed, "hashlib": stats(cpu),
            "read_names_over_read_all": round(t["read_names"]["median_ms"] / t["read_all"]["median_ms"], 3),
            "verify_over_read_all": round(t["verify"]["median_ms"] / t["read_all"]["median_ms"], 3),
            "hashlib_over_read_names_extra": round(statistics.median(cpu) / max(t["read_names"]["median_ms"] - t["read_all"]["median_ms"], 1e-3), 1),
            "hashlib_over_verify": round(statistics.median(cpu) / t["verify"]["median_ms"], 1)}
        checks = time_git_checks(pack, idx, min(a.reps, 3))
        res["names"]["git"] = {k: stats(v) for k, v in checks.items()} if checks else "git is not on this machine: no CPU figure"
    if a.build:
        assert idx_buf.tobytes() == idx == w_buf.raw and not b_st.any() and ok[0].value and ok[1].value
        assert c_used.size == cand.size and int((c_st == 0).sum()) >= n
        t = res["times"]
        res["build"] = {"last": built["last"], "candidates_over_objects": round(cand.size / n, 3),
                        "candidates_that_count_ok": int((c_st == 0).sum()),
                        "build_over_open_plus_verify": round(t["build"]["median_ms"] / (t["open"]["median_ms"] + t["verify"]["median_ms"]), 3)}
        git = time_git_index_pack(pack, min(a.reps, 3))
        if git:
            assert git[1] == idx
            res["build"]["git_index_pack"] = stats(git[0])
            res["build"]["git_index_pack_over_build"] = round(statistics.median(git[0]) / t["build"]["median_ms"], 1)
        else:
            res["build"]["git_index_pack"] = "git is not on this machine: no CPU figure"
    print(json.dumps(res))


def _header_size(pack, o):
    """the size the object's header states"""
    at = o["offset"]
    c = pack[at]
    size, shift = c & 15, 4
    while c & 0x80:
        at += 1
        c = pack[at]
        size |= (c & 0x7f) << shift
        shift += 7
    return size


def _zlib_of(pack, o):
    """the object's zlib stream: what follows its header and, for an OFS_DELTA, its distance (the pack holds no REF_DELTA)"""
    at = o["offset"]
    kind = (pack[at] >> 4) & 7
    while pack[at] & 0x80:
        at += 1
    at += 1
    if kind == 6:
        while pack[at] & 0x80:
            at += 1
        at += 1
    return memoryview(pack)[at:o["offset"] + o["packed_len"]]


if __name__ == "__main__":
    main()
