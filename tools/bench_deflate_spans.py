#!/usr/bin/env python3
"""ONE standard stream, host to host: the writer of joined spans (md_deflate_spans_host) over a list of span
sizes, against the single stream of Zl.Higher.compress's entry point (md_deflate_batch_host with n = 1) and against blocked
gzip (md_bgzf_compress) on the same input, all in one process.  Same text generator as tools/bench_deflate_long.py.
    python tools/bench_deflate_spans.py --mib 64 --kinds text random --level 6 --spans 64 128 256 512 1024
--prime adds primed rows ("deflate_span_prime") beside the unprimed ones, the variants of a span alternated run by run, and a
third row per span with the prefix chunks kept in the match kernel ("deflate_test_flags" bit 5: same bytes, for the time).
Prints one JSON line per (kind, writer): the median wall time of --reps runs in ms, the output size, and both relative to
the single stream; every output is inflated back by libz and compared with the input after the timed region.  The last
line per kind names the default the rule gives: the largest span whose time is within 10 % of the fastest."""
import argparse, json, os, statistics, sys, time, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    ts, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--kinds", nargs="+", default=["text", "random"], choices=["text", "random"])
    ap.add_argument("--level", type=int, default=6)
    ap.add_argument("--spans", type=int, nargs="+", default=[64, 128, 256, 512, 1024], help="KiB")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--prime", action="store_true", help="add primed rows beside the unprimed ones")
    ap.add_argument("--single-reps", type=int, default=3, help="runs of the single stream (seconds each)")
    args = ap.parse_args()
    import decompress_amd
    from decompress_amd import engine, gz, workloads
    eng = engine.default_engine(0)
    for kind in args.kinds:
        data = workloads.text(0xE4, args.mib << 20) if kind == "text" else os.urandom(args.mib << 20)
        ok = True

        def line(writer, ms, out, single=None, **more):
            nonlocal ok
            good = (b"".join(_members(out)) if writer == "bgzf" else zlib.decompress(out)) == data
            ok = ok and good
            d = {"mib": args.mib, "kind": kind, "level": args.level, "writer": writer, "ms": round(ms, 1), "bytes": len(out),
                 "ratio": round(len(out) / len(data), 4), "inflates_back": good}
            if single:
                d["time_vs_single"] = round(ms / single[0], 4)
                d["size_vs_single"] = round(len(out) / single[1], 4)
            d.update(more)
            print(json.dumps(d), flush=True)

        # warm-up: workspaces, code objects
        eng.deflate_one(data[:1 << 20], decompress_amd.FORMAT_ZLIB, level=args.level)
        eng.deflate_spans(data[:4 << 20], decompress_amd.FORMAT_ZLIB, span=64 << 10, level=args.level)
        gz.Bgzf.compress(data[:1 << 20], level=args.level)
        ms, (st, out, _) = timed(lambda: eng.deflate_one(data, decompress_amd.FORMAT_ZLIB, level=args.level), args.single_reps)
        assert st == 0
        single = (ms, len(out))
        line("single", ms, out)
        ms, out = timed(lambda: gz.Bgzf.compress(data, level=args.level), args.reps)
        line("bgzf", ms, out, single)
        rows, primed_rows = [], []
        variants = [("spans", False, 0)] + ([("spans-primed", True, 0), ("spans-primed-all-chunks", True, 32)] if args.prime else [])
        for kib in args.spans:
            def run(prime, flags):
                eng.set_option("deflate_test_flags", flags)
                try:
                    return eng.deflate_spans(data, decompress_amd.FORMAT_ZLIB, span=kib << 10, level=args.level, prime=prime)
                finally:
                    eng.set_option("deflate_test_flags", 0)
            ts, outs, last = {w: [] for w, _, _ in variants}, {}, {}
            for w, prime, flags in variants:
                run(prime, flags)  # (slots and workspace grow here, not in the timing)
            for _ in range(args.reps):
                for w, prime, flags in variants:
                    t0 = time.perf_counter()
                    st, outs[w], _ = run(prime, flags)
                    ts[w].append((time.perf_counter() - t0) * 1e3)
                    assert st == 0
                    last[w] = eng.deflate_spans_last()
            for w, _, _ in variants:
                ms = statistics.median(ts[w])
                line(w, ms, outs[w], single, span_kib=kib, min_ms=round(min(ts[w]), 1), max_ms=round(max(ts[w]), 1), **last[w])
                (rows if w == "spans" else primed_rows if w == "spans-primed" else []).append((kib, ms))
        if primed_rows:
            fastest = min(ms for _, ms in primed_rows)
            print(json.dumps({"kind": kind, "primed": True, "fastest_ms": round(fastest, 1),
                              "default_by_rule_kib": max(kib for kib, ms in primed_rows if ms <= 1.1 * fastest)}), flush=True)
        fastest = min(ms for _, ms in rows)
        print(json.dumps({"kind": kind, "fastest_ms": round(fastest, 1),
                          "default_by_rule_kib": max(kib for kib, ms in rows if ms <= 1.1 * fastest)}), flush=True)
        if not ok:
            sys.exit(1)


def _members(f):
    """the members of a gzip file, as libz reads them"""
    while f:
        d = zlib.decompressobj(31)
        yield d.decompress(f)
        f = d.unused_data


if __name__ == "__main__":
    main()
