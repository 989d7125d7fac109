"""The LZO size query against the decode it precedes, on C5 (tools/bench_lzo.py's batch: 8 192 x 128 KiB, half text, half
printable-ASCII noise) compressed by the library: md_lzo_sizes_batch_device and md_lzo_uncompress_batch_device
alternated in one process, warm-ups + repeats each, timed with md_timing_begin / _end.  Prints both medians with
min..max and, end to end, sizes -> plan -> 8 bytes read back -> decode against the decode with known caps (wall clock
around the calls, the context synchronised; the output buffer is allocated before the clock starts in both).

    python tools/bench_lzo_sizes.py [--streams 8192] [--stream-kib 128] [--unique 128] [--kind mix|text] [--reps 10] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import decompress_amd  # noqa: E402
from decompress_amd import lzo, workloads  # noqa: E402


def _stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--stream-kib", type=int, default=128)
    ap.add_argument("--unique", type=int, default=128)
    ap.add_argument("--kind", default="mix", help="mix (C5: half text, half ASCII noise) | text")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch

    eng = decompress_amd.Engine(0)
    dev = eng.device
    n, nb = a.streams, a.stream_kib * 1024
    uniq = [(workloads.text if a.kind == "text" or i % 2 == 0 else workloads.ascii_uniform)(0xC5 + i, nb) for i in range(min(a.unique, n))]
    blob, off, ln = workloads.pack([uniq[i % len(uniq)] for i in range(n)], align=32)
    cap = np.full(n, lzo.max_compressed_length(nb), dtype=np.int64)
    zoff = np.arange(n, dtype=np.int64) * ((int(cap[0]) + 255) // 256 * 256)
    t = lambda x: torch.from_numpy(x).to(dev)
    d_in, d_off, d_len = t(blob), t(off), t(ln)
    d_z = torch.empty(int(zoff[-1] + cap[-1]) + 64, dtype=torch.uint8, device=dev)
    d_zoff = t(zoff)
    z_len, z_st = eng.lzo_batch(True, d_in, d_off, d_len, d_z, d_zoff, t(cap))
    torch.cuda.synchronize(dev)
    assert (z_st.cpu() == 0).all()

    res_s = eng.lzo_sizes(d_z, d_zoff, z_len)
    out_off, out_cap, total = eng.inflate_plan(res_s[0], 256)
    eng.synchronize()
    assert (res_s[1].cpu() == 0).all() and (res_s[0].cpu() == nb).all() and int(total.item()) == n * nb
    d_out = torch.empty(int(total.item()) + 64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    res_d = None
    times = {"sizes": [], "decode": [], "sizes_plan_decode_wall": [], "decode_known_caps_wall": []}
    for rep in range(a.warmup + a.reps):
        for what in ("sizes", "decode"):
            eng.timing_begin()
            if what == "sizes":
                eng.lzo_sizes(d_z, d_zoff, z_len, res_s)
            else:
                res_d = eng.lzo_batch(False, d_z, d_zoff, z_len, d_out, out_off, out_cap, res_d)
            ms = eng.timing_end()
            if rep >= a.warmup:
                times[what].append(ms)
        for what in ("sizes_plan_decode_wall", "decode_known_caps_wall"):
            eng.synchronize()
            t0 = time.perf_counter()
            if what == "sizes_plan_decode_wall":
                eng.lzo_sizes(d_z, d_zoff, z_len, res_s)
                p_off, p_cap, p_total = eng.inflate_plan(res_s[0], 256)
                eng.synchronize()
                assert int(p_total.item()) + 64 <= d_out.numel()  # (the read-back that tells how much to allocate)
                eng.lzo_batch(False, d_z, d_zoff, z_len, d_out, p_off, p_cap, res_d)
            else:
                eng.lzo_batch(False, d_z, d_zoff, z_len, d_out, out_off, out_cap, res_d)
            eng.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if rep >= a.warmup:
                times[what].append(ms)
    torch.cuda.synchronize(dev)
    assert (res_d[1].cpu() == 0).all() and (res_d[0].cpu() == nb).all()
    back, o = d_out.cpu().numpy(), out_off.cpu().numpy()
    for k in range(0, n, max(1, n // 16)):
        assert back[o[k]:o[k] + nb].tobytes() == uniq[k % len(uniq)], k
    what = "C5 %d x %d KiB LZO1X (half text, half ASCII noise)" if a.kind == "mix" else "%d x %d KiB LZO1X (text)"
    out = {"workload": what % (n, a.stream_kib) + ", compressed by the library",
           "compressed_ratio": round(float(z_len.sum().item()) / float(ln.sum()), 4)}
    for what, v in times.items():
        out[what + "_ms"] = _stats(v)
    out["decode_over_sizes"] = round(out["decode_ms"]["median"] / out["sizes_ms"]["median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
