"""Many streaming decoders fed in pieces: md_inf_batch_* (one inflate launch per round of pieces) against md_inf_* (one
decoder at a time, a piece per md_inf_chunk_bytes(65536) step), on N streams of word text cut into R rounds of 64 KiB of
compressed input, in ZLIB and GZIP.  Prints one line per format and mode, and whether every output is byte-equal.
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_inf_batch.py ...`.

    python tools/bench_inf_batch.py [--n 1024] [--rounds 8] [--piece 65536] [--sample 8]
"""
import argparse
import ctypes
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import decompress_amd  # noqa: E402
from decompress_amd import workloads  # noqa: E402


def _compress(fmt, data):
    c = zlib.compressobj(6, zlib.DEFLATED, 15 if fmt == decompress_amd.FORMAT_ZLIB else 31)
    return c.compress(data) + c.flush()


def batch(eng, fmt, srcs, piece):
    lib = eng.lib
    n = len(srcs)
    b = lib.md_inf_batch_open(eng.ctx, fmt, n)
    buf = ctypes.create_string_buffer(8 << 20)
    outs = [bytearray() for _ in range(n)]
    pos = [0] * n
    t_dec, rounds = 0.0, 0
    t0 = time.perf_counter()
    while True:
        live = [i for i in range(n) if lib.md_inf_batch_status(b, i) == 0]
        if not live:
            break
        for i in live:
            c = srcs[i][pos[i]:pos[i] + piece]
            pos[i] += len(c)
            lib.md_inf_batch_src(b, i, c if c else None, len(c))
        t1 = time.perf_counter()
        assert lib.md_inf_batch_decode(b) == 0
        t_dec += time.perf_counter() - t1
        rounds += 1
        for i in range(n):
            while lib.md_inf_batch_pending(b, i):
                k = lib.md_inf_batch_out(b, i, buf, len(buf))
                outs[i] += buf.raw[:k]
    dt = time.perf_counter() - t0
    ok = all(lib.md_inf_batch_status(b, i) == 2 for i in range(n))
    launches = lib.md_i_inf_batch_launches(b)
    lib.md_inf_batch_close(b)
    return dt, t_dec, rounds, launches, outs, ok


def single(eng, fmt, src, piece):
    lib = eng.lib
    o = ctypes.create_string_buffer(1 << 20)
    d = lib.md_inf_decoder(eng.ctx, fmt, o, len(o))
    lib.md_inf_chunk_bytes(d, piece)
    out, p = bytearray(), 0
    while True:
        sig = lib.md_inf_decode(d)
        if sig == 0:
            c = src[p:p + piece]
            p += len(c)
            lib.md_inf_src(d, c, 0, len(c))
            continue
        out += o.raw[:len(o) - lib.md_inf_dst_rem(d)]
        lib.md_inf_flush(d)
        if sig in (2, 3):
            st = lib.md_inf_status(d)
            lib.md_inf_free(d)
            return out, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--piece", type=int, default=65536)
    ap.add_argument("--sample", type=int, default=8, help="md_inf_* decoders timed (the rest extrapolated)")
    a = ap.parse_args()
    eng = decompress_amd.Engine(0)
    # word text, about R pieces of compressed input per stream (text compresses ~2.7x at level 6)
    texts = [workloads.text(500 + k, int(a.piece * a.rounds * 2.7)) for k in range(min(64, a.n))]
    plains = [texts[i % len(texts)] for i in range(a.n)]
    for fmt, name in ((decompress_amd.FORMAT_ZLIB, "zlib"), (decompress_amd.FORMAT_GZIP, "gzip")):
        zs = [_compress(fmt, t) for t in texts]
        srcs = [zs[i % len(zs)] for i in range(a.n)]
        comp = sum(len(s) for s in srcs)
        plain_bytes = sum(len(p) for p in plains)
        batch(eng, fmt, srcs[:min(64, a.n)], a.piece)  # warm-up (allocations, code objects)
        dt, t_dec, rounds, launches, outs, ok = batch(eng, fmt, srcs, a.piece)
        equal = ok and all(bytes(o) == p for o, p in zip(outs, plains))
        print("%s batch: %d decoders, %.1f MiB in, %.1f MiB out, %d rounds, %d launches: %.1f ms in all, %.2f ms per "
              "md_inf_batch_decode = %.0f MiB/s out end to end; byte-equal=%s"
              % (name, a.n, comp / 2**20, plain_bytes / 2**20, rounds, launches, dt * 1e3, t_dec * 1e3 / rounds,
                 plain_bytes / 2**20 / dt, equal), flush=True)
        m = min(a.sample, a.n)
        single(eng, fmt, srcs[0], a.piece)  # warm-up
        t0 = time.perf_counter()
        eq1 = True
        for i in range(m):
            out, st = single(eng, fmt, srcs[i], a.piece)
            eq1 = eq1 and st == 0 and bytes(out) == plains[i]
        per = (time.perf_counter() - t0) / m
        print("%s single: md_inf_* with md_inf_chunk_bytes(%d), %d of %d decoders timed: %.1f ms per decoder; all %d one "
              "after the other (extrapolated): %.0f ms = %.0f MiB/s out; batch is %.0fx faster; byte-equal=%s"
              % (name, a.piece, m, a.n, per * 1e3, a.n, per * a.n * 1e3, plain_bytes / 2**20 / (per * a.n), per * a.n / dt, eq1),
              flush=True)


if __name__ == "__main__":
    main()
