"""The SHA-1 kernel alone on one GPU, everything resident, for DESIGN 4j (md_sha1_batch_device; times are md_sha1_last's:
two events around the launches).

  wave      one wavefront of 64 messages of --kib KiB each: microseconds per block of a wavefront that has its SIMD to itself
  chip      --waves wavefronts per SIMD on every SIMD of the device, messages of --kib KiB: the same at that occupancy, and
            the rate of the whole device.  Where the messages of all lanes do not fit --max-gib of memory they share regions
            (lane i reads region i mod R, at its own byte shift): the kernel is bound by its arithmetic, not by the reads
  launch    for "sha1_launch_blocks" = 1024 .. 65536: ONE launch in which every lane of `chip` advances a message by exactly
            that many blocks - the longest a launch can take on a full device.  The default is the largest under 50 ms

    python tools/bench_sha1.py [--kib 64] [--waves 5] [--reps 5] [--max-gib 4]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from decompress_amd import engine as _engine  # noqa: E402


def run(eng, n, length, regions, data, reps):
    """n messages of `length` bytes, message i at region i mod regions (regions of length + 64 bytes) shifted by i mod 4"""
    dev = eng.device
    i = torch.arange(n, dtype=torch.int64, device=dev)
    off = (i % regions) * (length + 64) + (i % 4)
    ln = torch.full((n,), length, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    times = []
    for _ in range(reps + 1):
        eng.sha1_batch_device(data, off, ln, None, length)
        eng.synchronize()
        times.append(eng.sha1_last()["device_ns"] / 1e6)
    return times[1:], eng.sha1_last()["launches"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kib", type=int, default=64)
    ap.add_argument("--waves", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-gib", type=int, default=4)
    a = ap.parse_args()
    eng = _engine.default_engine(0)
    dev = eng.device
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    budget = a.max_gib << 30
    data = torch.randint(0, 256, (budget + 4096,), dtype=torch.uint8, device=dev)
    res = {"cus": cus, "waves_per_simd": a.waves, "message_kib": a.kib, "reps": a.reps}
    length = (a.kib << 10) - 9  # with the padding: exactly kib * 16 blocks
    blocks = a.kib * 16
    try:
        eng.set_option("sha1_launch_blocks", 1 << 24)
        t, launches = run(eng, 64, length, 64, data, a.reps)
        med = statistics.median(t)
        res["wave"] = {"median_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "launches": launches,
                       "us_per_block": round(med * 1e3 / blocks, 4), "mb_s_per_message": round(length / med / 1e3, 2)}
        n = cus * 4 * a.waves * 64
        regions = min(n, budget // (length + 64))
        t, launches = run(eng, n, length, regions, data, a.reps)
        med = statistics.median(t)
        res["chip"] = {"messages": n, "regions": regions, "median_ms": round(med, 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4),
                       "launches": launches, "us_per_block_per_wavefront": round(med * 1e3 / blocks, 4),
                       "gib_s": round(n * length / 2**30 / (med / 1e3), 2), "ns_per_block_per_message_device_wide": round(med * 1e6 / blocks / n, 4)}
        res["launch"] = {}
        for per_launch in (1024, 2048, 4096, 8192, 16384, 32768, 65536):
            ln = per_launch * 64 - 9
            regions = max(1, min(n, budget // (ln + 64)))
            t, launches = run(eng, n, ln, regions, data, max(2, a.reps // 2))
            assert launches == 1
            res["launch"][str(per_launch)] = {"median_ms": round(statistics.median(t), 3), "max_ms": round(max(t), 3), "regions": regions}
    finally:
        eng.set_option("sha1_launch_blocks", _engine.SHA1_LAUNCH_BLOCKS)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
