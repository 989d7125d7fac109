"""Blocked gzip (BGZF) on one GPU, host to host and device time, for DESIGN 4f:

  (a) gz.Bgzf.compress, level 6, against gz.Higher.compress of the same buffer (one stream: DESIGN 4e's shape);
  (b) gz.Members.uncompress of (a)'s output against md_inflate_batch_host(MD_FORMAT_GZIP) over the same members handed in
      as a ready-made batch: descriptors built on the host, headers rewritten to the 10-byte form Gz.Inf reads - the gap
      is what the member scan, the chain and the descriptors cost;
  (c) the scan alone (md_gz_members_scan: copy-in, mark, chain, descriptors; no decode);
  (d) files WITHOUT size fields (--plain; written here with Python's zlib, as tests/gz_members_util.member does), each with
      md_set_option "gz_members_speculate" 1 and 0 - 0 is the host loop, member by member, the only path such a file had
      before the speculative one: (i) the word text as members of 0xff00 bytes ((b)'s file minus the BC field, so (b)'s
      indexed figure is the yardstick beside it), (ii) as 65 536 members of 1 KiB, (iii) file (i) with one member of
      16 MiB in the middle.  With each file the md_gz_members_last of its speculative run.
(b) calls the C entry point with a destination that exists, as the batch leg does; "members_uncompress_python" is the same
through gz.Members.uncompress, which allocates and slices a bytes object per call.

    python tools/bench_gz_members.py [--mib 64] [--reps 5] [--warmup 1] [--skip-single] [--plain | --plain-only]

The legs of a group are alternated in one process; every leg reports the median and the spread (min .. max) of its
repeats, host to host (perf_counter around the call) and on the device (md_timing_begin / md_timing_end)."""
import argparse
import ctypes
import json
import os
import random
import statistics
import struct
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from decompress_amd import _lib  # noqa: E402
from decompress_amd import engine as _engine  # noqa: E402
from decompress_amd import gz, workloads  # noqa: E402


def timed(eng, fn):
    ms = ctypes.c_float()
    eng.lib.md_timing_begin(eng.ctx)
    t0 = time.perf_counter()
    r = fn()
    host = (time.perf_counter() - t0) * 1e3
    eng.lib.md_timing_end(eng.ctx, ctypes.byref(ms))
    return r, host, ms.value


def stats(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "n": len(v)}


def alternate(eng, legs, reps, warmup):
    """legs: {name: fn}; one round runs every leg once, in order -> ({name: {host, device}}, the legs' last results)"""
    host = {k: [] for k in legs}
    dev = {k: [] for k in legs}
    last = {}
    for r in range(warmup + reps):
        for k, fn in legs.items():
            out, h, d = timed(eng, fn)
            last[k] = out
            if r >= warmup:
                host[k].append(h)
                dev[k].append(d)
    return {k: {"host": stats(host[k]), "device": stats(dev[k])} for k in legs}, last


def ready_made_batch(f):
    """the members of a file gz.Bgzf.compress wrote, as a batch for MD_FORMAT_GZIP: the 18-byte headers cut to the 10 bytes
    without FEXTRA -> (blob, in_off, in_len, out_cap)"""
    parts, caps, pos = [], [], 0
    while pos < len(f):
        size = struct.unpack_from("<H", f, pos + 16)[0] + 1
        parts.append(f[pos:pos + 3] + b"\0" + f[pos + 4:pos + 10] + f[pos + 18:pos + size])
        caps.append(struct.unpack_from("<I", f, pos + size - 4)[0])
        pos += size
    in_len = np.array([len(p) for p in parts], dtype=np.uint64)
    in_off = np.concatenate(([0], np.cumsum(in_len)[:-1])).astype(np.uint64)
    return np.frombuffer(b"".join(parts), dtype=np.uint8), in_off, in_len, np.array(caps, dtype=np.uint64)


def plain_member(data, level=6):
    """one RFC 1952 member without any optional field (tests/gz_members_util.member)"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return (struct.pack("<BBBBIBB", 0x1f, 0x8b, 8, 0, 0, 0, 255) + c.compress(data) + c.flush()
            + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff))


def plain_files(src):
    """name -> (file, members) for leg (d)"""
    n = len(src)
    cut = lambda a, b, step: [plain_member(src[k:min(k + step, b)]) for k in range(a, b, step)]
    i = cut(0, n, 0xff00)
    ii = cut(0, n, n // 65536 if n >= 65536 else 1)
    mid, big = (n // 2) // 0xff00 * 0xff00, min(16 << 20, n // 4)
    iii = cut(0, mid, 0xff00) + [plain_member(src[mid:mid + big])] + cut(mid + big, n, 0xff00)
    return {"i_members_of_ff00": (b"".join(i), len(i)), "ii_members_of_1k": (b"".join(ii), len(ii)),
            "iii_one_16mib_member": (b"".join(iii), len(iii))}


def plain_leg(eng, src, reps, warmup):
    n = len(src)
    dst = np.empty(n, dtype=np.uint8)
    info = _lib.GzMembersInfo()
    res = {}
    for name, (f, members) in plain_files(src).items():
        seen = {}

        def run(spec):
            eng.set_option("gz_members_speculate", spec)
            assert eng.lib.md_gz_members_uncompress(eng.ctx, f, len(f), dst.ctypes.data, n, ctypes.byref(info)) == 0
            seen[spec] = (info.members, info.written, info.indexed, gz.Members.last_stats())

        try:
            t, _ = alternate(eng, {"speculate_1": lambda: run(1), "speculate_0": lambda: run(0)}, reps, warmup)
        finally:
            eng.set_option("gz_members_speculate", 1)
        for spec in (0, 1):
            assert seen[spec][:3] == (members, n, 0), (name, seen[spec])
        assert seen[0][3]["path"] == 0 and seen[1][3]["path"] == 2 and dst.tobytes() == src, name
        res[name] = {"file_bytes": len(f), "members": members, "times": t, "last_stats": seen[1][3]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-single", action="store_true", help="leave gz.Higher.compress (seconds per call) out of (a)")
    ap.add_argument("--plain", action="store_true", help="add leg (d): files without size fields, speculative path against the host loop")
    ap.add_argument("--plain-only", action="store_true", help="leg (d) alone")
    a = ap.parse_args()
    eng = _engine.default_engine(0)
    n = a.mib << 20
    res = {"mib": a.mib, "reps": a.reps, "warmup": a.warmup}
    if a.plain or a.plain_only:
        res["d_plain_text"] = plain_leg(eng, workloads.text(1, n), a.reps, a.warmup)
    inputs = {} if a.plain_only else {"text": workloads.text(1, n), "random": random.Random(1).randbytes(n)}
    for name, src in inputs.items():
        legs = {"bgzf_compress": lambda: gz.Bgzf.compress(src, level=6)}
        if not a.skip_single:
            legs["higher_compress"] = lambda: gz.Higher.compress(src, level=6)
        t, last = alternate(eng, legs, a.reps, a.warmup)
        f = last["bgzf_compress"]
        row = {"a_compress": t, "file_bytes": len(f)}
        if "higher_compress" in last:
            row["single_stream_bytes"] = len(last["higher_compress"])
        blob, in_off, in_len, caps = ready_made_batch(f)
        m = len(caps)
        out_off = np.concatenate(([0], np.cumsum(caps)[:-1])).astype(np.uint64)
        out = np.empty(max(int(caps.sum()), 1), dtype=np.uint8)
        out_len, used = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64)
        status = np.zeros(m, dtype=np.int32)

        def batch():
            eng._check(eng.lib.md_inflate_batch_host(eng.ctx, _engine.FORMAT_GZIP, m, blob.ctypes.data, blob.size, in_off.ctypes.data,
                                                      in_len.ctypes.data, out.ctypes.data, out.size, out_off.ctypes.data, caps.ctypes.data,
                                                      out_len.ctypes.data, used.ctypes.data, status.ctypes.data, None))

        def scan():  # (one call: gz.Members.scan makes a second one for the offsets)
            info = _lib.GzMembersInfo()
            eng._check(eng.lib.md_gz_members_scan(eng.ctx, f, len(f), ctypes.byref(info), None, None, 0))
            assert info.indexed == 1 and info.written == n

        dst = np.empty(n, dtype=np.uint8)  # (both decoders write into buffers that exist: no first-touch page faults timed)
        info = _lib.GzMembersInfo()

        def members():
            assert eng.lib.md_gz_members_uncompress(eng.ctx, f, len(f), dst.ctypes.data, n, ctypes.byref(info)) == 0

        t, last = alternate(eng, {"members_uncompress": members, "ready_made_batch": batch, "members_scan": scan,
                                  "members_uncompress_python": lambda: gz.Members.uncompress(f, n)}, a.reps, a.warmup)
        assert info.indexed == 1 and info.written == n and dst.tobytes() == src, name
        assert last["members_uncompress_python"][2] == src, name
        assert not status.any() and out[:n].tobytes() == src, name
        row["b_c_uncompress"] = t
        row["members"] = info.members
        res[name] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
