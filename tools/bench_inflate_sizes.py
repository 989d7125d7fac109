"""The size query against the full decode on C2 (4 096 zlib streams of 256 KiB): md_inflate_sizes_batch_device and
md_inflate_batch_device alternated in one process, 2 warm-ups + 10 repeats each, timed with md_timing_begin / _end.
Prints both medians with min..max, and the count kernel's rounds, passes per round and share of rounds that needed the
checking walk (md_set_option "profile").

    python tools/bench_inflate_sizes.py [--n 4096] [--kib 256] [--unique 256] [--reps 10] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import decompress_amd  # noqa: E402
from decompress_amd import workloads  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--kib", type=int, default=256)
    ap.add_argument("--unique", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch

    eng = decompress_amd.Engine(0)
    dev = eng.device
    nbytes = a.kib * 1024
    streams = workloads.c2_streams(a.n, nbytes, unique=a.unique, workers=16)
    blob, offs, lens = workloads.pack(streams)
    t = lambda x: torch.from_numpy(x).to(dev)
    d_in, d_off, d_len = t(blob), t(offs), t(lens)
    torch.cuda.synchronize(dev)
    sizes, used, st = eng.inflate_sizes(decompress_amd.FORMAT_ZLIB, d_in, d_off, d_len)
    out_off, out_cap, total = eng.inflate_plan(sizes, 256)
    eng.synchronize()
    assert (st.cpu() == 0).all() and (sizes.cpu() == nbytes).all() and int(total.item()) == a.n * nbytes
    d_out = torch.empty(int(total.item()) + 16, dtype=torch.uint8, device=dev)
    res_s = (sizes, used, st)
    res_d = None
    times = {"sizes": [], "decode": []}
    for rep in range(a.warmup + a.reps):
        for what in ("sizes", "decode"):
            eng.timing_begin()
            if what == "sizes":
                eng.inflate_sizes(decompress_amd.FORMAT_ZLIB, d_in, d_off, d_len, res_s)
            else:
                res_d = eng.inflate_batch(decompress_amd.FORMAT_ZLIB, d_in, d_off, d_len, d_out, out_off, out_cap, res_d)
            ms = eng.timing_end()
            if rep >= a.warmup:
                times[what].append(ms)
    assert (res_d[2].cpu() == 0).all() and (res_d[0].cpu() == nbytes).all()
    eng.set_option("profile", 1)
    eng.inflate_sizes(decompress_amd.FORMAT_ZLIB, d_in, d_off, d_len, res_s)
    eng.synchronize()
    rounds, passes, checked = eng.get_profile_raw()[:3]
    eng.set_option("profile", 0)
    out = {"workload": "C2 %d x %d KiB zlib" % (a.n, a.kib)}
    for what, v in times.items():
        out[what + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    out["speedup"] = round(out["decode_ms"]["median"] / out["sizes_ms"]["median"], 3)
    out["count_rounds"] = rounds
    out["passes_per_round"] = round(passes / max(rounds, 1), 3)
    out["checked_share"] = round(checked / max(rounds, 1), 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
