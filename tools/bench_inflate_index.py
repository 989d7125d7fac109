"""The index of one long stream against the plain one-stream call: ONE text stream at zlib level 6, everything
in one process, host buffers (pageable numpy arrays) in and out, every call synchronous, wall-clock per call
(time.perf_counter around the C call: copies in, kernels, copies out and the call's own synchronisation included),
`--warmup` calls first, then the median (min..max) of `--reps`.

  (a) md_zl_higher_uncompress           the yardstick: the whole stream by the long-stream decoder
  (b) md_inflate_index_build, no output
  (c) md_inflate_index_build with output
  (d) md_inflate_index_read of [0, size)
  (e) md_inflate_index_read of `--ranges` random ranges of `--range-kib` KiB in one call

With each: bytes copied to the device and pieces, where the call says so.  --fixed-mib: the same for a Z_FIXED stream,
which the block finder cannot cut: its build is the serial path.  --plain-only: (a) alone (for a build of the
parent commit through MD_LIBMDEFLATE).

    python tools/bench_inflate_index.py [--mib 64] [--span-kib 1024,128] [--reps 7] [--warmup 2] [--ranges 4096] [--range-kib 64]
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import decompress_amd  # noqa: E402
from decompress_amd import _lib, workloads  # noqa: E402


def _timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--span-kib", default="1024", help="one span, or several separated by commas: (b) .. (e) for each")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ranges", type=int, default=4096)
    ap.add_argument("--range-kib", type=int, default=64)
    ap.add_argument("--fixed-mib", type=int, default=8, help="also: a Z_FIXED stream of this many MiB at span 1 MiB, 1 + 3 calls (0 = skip)")
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    eng = decompress_amd.Engine(0)
    lib, ctx = eng.lib, eng.ctx
    plain = b"".join(workloads.text(1 + k, 4 << 20) for k in range(a.mib // 4)) if a.mib >= 4 else workloads.text(1, a.mib << 20)
    src_b = zlib.compress(plain, 6)
    size = len(plain)
    src = np.frombuffer(src_b, dtype=np.uint8)
    dst = np.zeros(size + 64, dtype=np.uint8)
    want = np.frombuffer(plain, dtype=np.uint8)
    top = {"workload": "text %d MiB, zlib -6, %d bytes compressed" % (a.mib, len(src_b))}
    out = top
    got = ctypes.c_size_t()

    def plain_call():
        assert lib.md_zl_higher_uncompress(ctx, src.ctypes.data, src.nbytes, dst.ctypes.data, size, ctypes.byref(got)) == 0

    out["a_uncompress"] = _timed(plain_call, a.warmup, a.reps)
    out["a_uncompress"]["bytes_in"] = src.nbytes
    out["a_uncompress"]["pieces | rounds << 24"] = lib.md_set_option(ctx, b"inflate_parallel_last", 0)
    assert got.value == size and np.array_equal(dst[:size], want)
    if not a.plain_only:
        for kib in a.span_kib.split(","):
            top["span_%s_kib" % kib] = _span(a, lib, ctx, src, size, want, int(kib) << 10)
        if a.fixed_mib:  # a stream the block finder has no candidates in: the build goes piece by piece through one pair of wavefronts
            c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
            fplain = plain[:a.fixed_mib << 20]
            fsrc = np.frombuffer(c.compress(fplain) + c.flush(), dtype=np.uint8)
            fwant = np.frombuffer(fplain, dtype=np.uint8)
            fdst = np.zeros(len(fplain) + 64, dtype=np.uint8)

            def fixed_plain():
                assert lib.md_zl_higher_uncompress(ctx, fsrc.ctypes.data, fsrc.nbytes, fdst.ctypes.data, len(fplain), ctypes.byref(got)) == 0

            top["fixed_%d_mib" % a.fixed_mib] = {"compressed": int(fsrc.nbytes), "uncompress": _timed(fixed_plain, 1, 3)}
            a.ranges, a.warmup, a.reps = min(a.ranges, 256), 1, 3
            top["fixed_%d_mib" % a.fixed_mib].update(_span(a, lib, ctx, fsrc, len(fplain), fwant, 1 << 20))
    print(json.dumps(top))


def _span(a, lib, ctx, src, size, want, span):
    """(b) .. (e) at one span"""
    out = {}
    dst = np.zeros(size + 64, dtype=np.uint8)
    handles = []

    def build(with_output):
        h, info = ctypes.c_void_p(), _lib.InflateIndexInfo()
        st = lib.md_inflate_index_build(ctx, 1, src.ctypes.data, src.nbytes, span, dst.ctypes.data if with_output else None,
                                        size if with_output else 0, ctypes.byref(h), ctypes.byref(info))
        assert st == 0 and info.size == size, st
        handles.append((h, info.points))

    for key, with_output in (("b_build", False), ("c_build_with_output", True)):
        dst[:] = 0
        out[key] = _timed(lambda: build(with_output), a.warmup, a.reps)
        out[key]["bytes_in"] = src.nbytes
        out[key]["points"] = handles[-1][1]
        out[key]["index_bytes"] = lib.md_inflate_index_save_size(handles[-1][0])
        out[key]["pieces | rounds << 24"] = lib.md_set_option(ctx, b"inflate_parallel_last", 0)
        if with_output:
            assert np.array_equal(dst[:size], want)
        for h, _ in handles[:-1]:
            lib.md_inflate_index_free(h)
        del handles[:-1]
    idx = handles[-1][0]
    stats = _lib.InflateIndexStats()

    def read(off, ln, dst_off, status):
        n = len(off)
        assert lib.md_inflate_index_read(ctx, idx, src.ctypes.data, src.nbytes, n, off.ctypes.data, ln.ctypes.data, dst.ctypes.data,
                                         dst_off.ctypes.data, status.ctypes.data) == 0
        assert not status.any()

    def counts(key):
        assert lib.md_inflate_index_last(ctx, ctypes.byref(stats)) == 0
        out[key].update(pieces=stats.pieces, launches=stats.launches, bytes_in=stats.bytes_in, bytes_windows=stats.bytes_windows,
                        bytes_scratch=stats.bytes_scratch)

    u64 = lambda v: np.array(v, dtype=np.uint64)
    dst[:] = 0
    whole = (u64([0]), u64([size]), u64([0]), np.zeros(1, dtype=np.int32))
    out["d_read_all"] = _timed(lambda: read(*whole), a.warmup, a.reps)
    counts("d_read_all")
    assert np.array_equal(dst[:size], want)
    rng = random.Random(1)
    rlen = min(a.range_kib << 10, size)
    nr = a.ranges
    dst = np.zeros(nr * rlen + 64, dtype=np.uint8)  # (the ranges' bytes are packed back to back)
    offs = [rng.randrange(size - rlen + 1) for _ in range(nr)]
    many = (u64(offs), u64([rlen] * nr), u64([k * rlen for k in range(nr)]), np.zeros(nr, dtype=np.int32))
    key = "e_read_%d_ranges_of_%d_kib" % (nr, a.range_kib)
    out[key] = _timed(lambda: read(*many), a.warmup, a.reps)
    counts(key)
    for k in (0, nr // 2, nr - 1):
        assert np.array_equal(dst[k * rlen:(k + 1) * rlen], want[offs[k]:offs[k] + rlen])
    lib.md_inflate_index_free(idx)
    return out


if __name__ == "__main__":
    main()
