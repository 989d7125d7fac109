#!/usr/bin/env python3
"""ONE long stream, host to host, through Zl.Higher.compress's entry point (md_deflate_batch_host with n = 1):
the hash chains in segments on the whole chip ("deflate_link_segment_min" at its default) against the one-workgroup
link kernel ("deflate_link_segment_min" = 0), alternated in one process; the two outputs are compared after the timed region.
    python tools/bench_deflate_long.py --mib 16 64 --kinds text random --levels 4 6 9 --reps 2
Prints one JSON line per (size, kind, level): best wall time of each mode in ms and the ratio."""
import argparse, json, os, sys, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--kinds", nargs="+", default=["text", "random"], choices=["text", "random"])
    ap.add_argument("--levels", type=int, nargs="+", default=[4, 6, 9])
    ap.add_argument("--reps", type=int, default=2)
    args = ap.parse_args()
    import decompress_amd
    from decompress_amd import workloads
    eng = decompress_amd.Engine(0)
    for mib in args.mib:
        for kind in args.kinds:
            data = workloads.text(0xE4, mib << 20) if kind == "text" else os.urandom(mib << 20)
            for level in args.levels:
                best = {"parallel": float("inf"), "serial": float("inf")}
                outs, segs = {}, 0
                eng.deflate_one(data[:1 << 20], decompress_amd.FORMAT_ZLIB, level=level)  # warm-up: workspaces, code objects
                for _ in range(args.reps):
                    for mode in ("parallel", "serial"):
                        eng.set_option("deflate_link_segment_min", 128 if mode == "parallel" else 0)
                        t0 = time.perf_counter()
                        st, out, _ = eng.deflate_one(data, decompress_amd.FORMAT_ZLIB, level=level)
                        dt = (time.perf_counter() - t0) * 1e3
                        if mode == "parallel":
                            segs = eng.link_segments()
                        best[mode] = min(best[mode], dt)
                        outs[mode] = (st, out)
                eng.set_option("deflate_link_segment_min", 128)
                same = outs["parallel"] == outs["serial"] and outs["parallel"][0] == 0
                ok = same and zlib.decompress(outs["parallel"][1]) == data
                print(json.dumps({"mib": mib, "kind": kind, "level": level, "segments": segs,
                                  "parallel_ms": round(best["parallel"], 1), "serial_ms": round(best["serial"], 1),
                                  "speedup": round(best["serial"] / best["parallel"], 3),
                                  "ratio": round(len(outs["parallel"][1]) / len(data), 4), "bytes_equal": ok}), flush=True)
                if not ok:
                    sys.exit(1)


if __name__ == "__main__":
    main()
