"""Random access to a blocked gzip (BGZF) file on one GPU, host to host, for DESIGN 4f.  The file is text written by
md_bgzf_compress (level 6, blocks of 0xff00), at the size tools/bench_gz_members.py uses:

  (a) md_gz_members_uncompress of the whole file - the only way to a byte range before there was an index;
  (b) md_bgzf_read of [0, size): the same decode plus the gather into the range;
  (c) `--ranges` random ranges of `--range-kib` KiB in one md_bgzf_read call;
  (d) one range of 4 KiB;
  and md_bgzf_index_build (the member scan and its table, nothing decoded).
With each read leg the md_bgzf_read_last of its last run: members decoded, launches, bytes of src copied to the device.

    python tools/bench_bgzf_read.py [--mib 64] [--reps 7] [--warmup 1] [--ranges 4096] [--range-kib 64]

The legs are alternated in one process; every leg reports the median and the spread (min .. max) of its repeats, host to host
(perf_counter around a call that ends in a synchronise).  Every leg's bytes are compared with the plaintext."""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from decompress_amd import _lib  # noqa: E402
from decompress_amd import engine as _engine  # noqa: E402
from decompress_amd import gz, workloads  # noqa: E402


def stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ranges", type=int, default=4096)
    ap.add_argument("--range-kib", type=int, default=64)
    a = ap.parse_args()
    eng = _engine.default_engine(0)
    lib = eng.lib
    n = a.mib << 20
    src = workloads.text(1, n)
    f = gz.Bgzf.compress(src, level=6)
    flat = np.frombuffer(src, dtype=np.uint8)
    idx = gz.BgzfIndex.build(f)
    info = idx.info()
    assert info["size"] == n

    whole = np.empty(n, dtype=np.uint8)  # (every leg writes into a buffer that exists: no first-touch page faults timed)
    minfo = _lib.GzMembersInfo()

    def members():
        assert lib.md_gz_members_uncompress(eng.ctx, f, len(f), whole.ctypes.data, n, ctypes.byref(minfo)) == 0

    def build():
        h = ctypes.c_void_p()
        assert lib.md_bgzf_index_build(eng.ctx, f, len(f), ctypes.byref(h)) == 0
        lib.md_bgzf_index_free(h)

    rng = random.Random(2)
    step = a.range_kib << 10
    sets = {"b_whole": [(0, n)], "c_random_ranges": [(rng.randrange(n - step), step) for _ in range(a.ranges)],
            "d_one_4k": [(rng.randrange(n - 4096), 4096)]}
    calls, last = {}, {}
    for name, ranges in sets.items():
        off = np.array([o for o, _ in ranges], dtype=np.uint64)
        ln = np.array([m for _, m in ranges], dtype=np.uint64)
        dst_off = np.concatenate(([0], np.cumsum(ln)[:-1])).astype(np.uint64)
        dst = np.empty(int(ln.sum()), dtype=np.uint8)
        status = np.zeros(len(ranges), dtype=np.int32)

        def read(off=off, ln=ln, dst_off=dst_off, dst=dst, status=status, name=name):
            eng._check(lib.md_bgzf_read(eng.ctx, idx._h, f, len(f), len(off), off.ctypes.data, ln.ctypes.data, dst.ctypes.data,
                                        dst_off.ctypes.data, status.ctypes.data))
            last[name] = idx.last_stats()

        calls[name] = (read, off, ln, dst_off, dst, status)
    legs = {"a_members_uncompress": members, "index_build": build}
    legs.update({k: v[0] for k, v in calls.items()})
    times = {k: [] for k in legs}
    for r in range(a.warmup + a.reps):
        for k, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            if r >= a.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    assert minfo.indexed == 1 and minfo.written == n and whole.tobytes() == src
    for name, (_, off, ln, dst_off, dst, status) in calls.items():
        assert not status.any(), name
        for o, m, d in zip(off, ln, dst_off):
            assert np.array_equal(dst[int(d):int(d + m)], flat[int(o):int(o + m)]), (name, int(o))
    res = {"mib": a.mib, "reps": a.reps, "warmup": a.warmup, "file_bytes": len(f), "members": info["members"], "ranges": a.ranges,
           "range_kib": a.range_kib, "times": {k: stats(v) for k, v in times.items()}, "last_stats": last}
    base = res["times"]["a_members_uncompress"]["median_ms"]
    res["ratio_to_a"] = {k: round(res["times"][k]["median_ms"] / base, 4) for k in calls}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
