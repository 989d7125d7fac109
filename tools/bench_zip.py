"""ZIP archives on one GPU, host to host and device time, for DESIGN 4g:

  (a) md_zip_uncompress of the corpus files cycled to --mib of plaintext, written by Python's zipfile at level 6, against
      today's way on the same bodies: md_inflate_batch_host(MD_FORMAT_DEFLATE) with descriptors taken from zipfile, the
      plaintext sent to the device again and md_crc32_batch_device over it, the checksums read back and compared.  The gap
      is what the container costs;
  (b) the same archive plus ONE stored entry of --big-mib (default 1 024), and that entry alone, for md_set_option
      "zip_crc_segment" = 64 .. 1 024 KiB; beside them md_crc32_batch_device on that one buffer, resident on the device
      (one wavefront).  This sweep picks the option's default;
  (c) md_zip_compress at level 6 against md_deflate_batch_host (raw DEFLATE, the same parameters) of the same files.

    python tools/bench_zip.py [--mib 512] [--big-mib 1024] [--reps 5] [--warmup 1] [--skip a,b,c]

The legs of a group are alternated in one process; every leg reports the median and the spread (min .. max) of its
repeats, host to host (perf_counter around the call) and on the device (md_timing_begin / md_timing_end)."""
import argparse
import ctypes
import io
import json
import os
import sys
import zipfile
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from decompress_amd import _lib  # noqa: E402
from decompress_amd import engine as _engine  # noqa: E402
from decompress_amd import workloads, zp  # noqa: E402
from tools.bench_gz_members import alternate  # noqa: E402

SEGMENTS_KIB = (64, 128, 256, 512, 1024)


def corpus_files(nbytes):
    """the corpus files, cycled until they hold nbytes -> [(name, bytes)]"""
    files, total, k = [], 0, 0
    items = list(workloads.corpus().items())
    while total < nbytes:
        name, data = items[k % len(items)]
        files.append(("%05d/%s" % (k, name), data))
        total += len(data)
        k += 1
    return files


def write_zip(files, big=None):
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED, compresslevel=6) as z:
        for n, d in files:
            z.writestr(n, d)
        if big is not None:
            z.writestr(zipfile.ZipInfo("big.bin"), big, compress_type=zipfile.ZIP_STORED)
    return buf.getvalue()


class Reader:
    """md_zip_uncompress into buffers that exist (no first-touch page faults timed)"""

    def __init__(self, eng, blob):
        self.eng, self.blob = eng, blob
        ents, info = zp.directory(blob)
        self.k, self.need = len(ents), info["total_usize"]
        self.dst = np.empty(max(self.need, 1), dtype=np.uint8)
        self.off, self.st, self.res = (ctypes.c_uint64 * (self.k + 1))(), (ctypes.c_int32 * max(self.k, 1))(), _lib.ZipResult()

    def __call__(self):
        rc = self.eng.lib.md_zip_uncompress(self.eng.ctx, self.blob, len(self.blob), None, 0, self.dst.ctypes.data, self.need, self.off, self.st,
                                            ctypes.byref(self.res))
        assert rc == 0 and self.res.failed == 0 and self.res.written == self.need, (rc, self.res.failed)


def by_hand(eng, blob):
    """today's way -> (the leg, its output array)"""
    torch = eng.torch
    with zipfile.ZipFile(io.BytesIO(blob)) as z:
        infos = z.infolist()
    assert all(i.compress_type == 8 for i in infos)
    body = lambda i: i.header_offset + 30 + int.from_bytes(blob[i.header_offset + 26:i.header_offset + 28], "little") + \
        int.from_bytes(blob[i.header_offset + 28:i.header_offset + 30], "little")
    m = len(infos)
    src = np.frombuffer(blob, dtype=np.uint8)
    in_off = np.array([body(i) for i in infos], dtype=np.uint64)
    in_len = np.array([i.compress_size for i in infos], dtype=np.uint64)
    caps = np.array([i.file_size for i in infos], dtype=np.uint64)
    want = np.array([i.CRC for i in infos], dtype=np.uint32)
    out_off = np.concatenate(([0], np.cumsum(caps)[:-1])).astype(np.uint64)
    out = np.empty(max(int(caps.sum()), 1), dtype=np.uint8)
    out_len, used, status = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.int32)
    d_off = torch.from_numpy(out_off.astype(np.int64)).to(eng.device)
    d_len = torch.from_numpy(caps.astype(np.int64)).to(eng.device)

    def leg():
        eng._check(eng.lib.md_inflate_batch_host(eng.ctx, _engine.FORMAT_DEFLATE, m, src.ctypes.data, src.size, in_off.ctypes.data, in_len.ctypes.data,
                                                  out.ctypes.data, out.size, out_off.ctypes.data, caps.ctypes.data, out_len.ctypes.data,
                                                  used.ctypes.data, status.ctypes.data, None))
        crc = eng.crc32_batch(torch.from_numpy(out).to(eng.device), d_off, d_len).cpu().numpy().view(np.uint32)
        assert not status.any() and (used == in_len).all() and (out_len == caps).all() and (crc == want).all()

    return leg, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=512)
    ap.add_argument("--big-mib", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip", default="", help="legs to leave out, e.g. b,c")
    a = ap.parse_args()
    skip = set(a.skip.split(","))
    eng = _engine.default_engine(0)
    files = corpus_files(a.mib << 20)
    plain = b"".join(d for _, d in files)
    res = {"mib": a.mib, "big_mib": a.big_mib, "reps": a.reps, "warmup": a.warmup, "files": len(files), "plain_bytes": len(plain)}
    blob = write_zip(files)
    res["archive_bytes"] = len(blob)
    if "a" not in skip:
        reader = Reader(eng, blob)
        hand, hand_out = by_hand(eng, blob)
        t, _ = alternate(eng, {"zip_uncompress": reader, "inflate_batch_host_plus_crc32_batch": hand}, a.reps, a.warmup)
        assert reader.dst.tobytes() == plain and hand_out.tobytes() == plain
        res["a_uncompress"] = t
    if "b" not in skip:
        big = np.random.default_rng(1).integers(0, 256, a.big_mib << 20, dtype=np.uint8).tobytes()
        both, alone = Reader(eng, write_zip(files, big)), Reader(eng, write_zip([], big))
        d_big = eng.torch.from_numpy(np.frombuffer(big, dtype=np.uint8).copy()).to(eng.device)
        d_off = eng.torch.zeros(1, dtype=eng.torch.int64, device=eng.device)
        d_len = eng.torch.full((1,), len(big), dtype=eng.torch.int64, device=eng.device)
        want = zlib.crc32(big)

        def one_wave():
            assert int(eng.crc32_batch(d_big, d_off, d_len).cpu().numpy().view(np.uint32)[0]) == want

        def at(reader, kib):
            def leg():
                eng.set_option("zip_crc_segment", kib)
                reader()
            return leg

        legs = {"crc32_batch_device_one_buffer": one_wave}
        for kib in SEGMENTS_KIB:
            legs["archive_plus_big_%d_kib" % kib] = at(both, kib)
            legs["big_alone_%d_kib" % kib] = at(alone, kib)
        try:
            t, _ = alternate(eng, legs, a.reps, a.warmup)
        finally:
            eng.set_option("zip_crc_segment", 0)
        assert both.dst.tobytes() == plain + big and alone.dst.tobytes() == big
        res["b_one_stored_entry"] = t
        del both, alone, d_big, big
    if "c" not in skip:
        src = np.frombuffer(plain, dtype=np.uint8)
        in_len = np.array([len(d) for _, d in files], dtype=np.uint64)
        in_off = np.concatenate(([0], np.cumsum(in_len)[:-1])).astype(np.uint64)
        caps = in_len + np.uint64(64)  # (room for a file that does not compress)
        out_off = np.concatenate(([0], np.cumsum(caps)[:-1])).astype(np.uint64)
        out = np.empty(int(caps.sum()), dtype=np.uint8)
        out_len, status = np.zeros(len(files), dtype=np.uint64), np.zeros(len(files), dtype=np.int32)
        p = eng._params(6, 4096, _engine.DRIVER_ZL, True)

        def batch():
            eng._check(eng.lib.md_deflate_batch_host(eng.ctx, _engine.FORMAT_DEFLATE, ctypes.byref(p), len(files), src.ctypes.data, src.size,
                                                      in_off.ctypes.data, in_len.ctypes.data, out.ctypes.data, out.size, out_off.ctypes.data,
                                                      caps.ctypes.data, out_len.ctypes.data, status.ctypes.data, None))

        arr, packed = zp._sources(files)
        bound = eng.lib.md_zip_compress_bound(len(files), arr)
        dst = np.empty(bound, dtype=np.uint8)
        wrote = ctypes.c_size_t()

        def writer():
            assert eng.lib.md_zip_compress(eng.ctx, 6, len(files), arr, packed, len(packed), dst.ctypes.data, bound, ctypes.byref(wrote)) == 0

        t, _ = alternate(eng, {"zip_compress": writer, "deflate_batch_host": batch}, a.reps, a.warmup)
        with zipfile.ZipFile(io.BytesIO(dst[:wrote.value].tobytes())) as z:
            assert z.testzip() is None and len(z.infolist()) == len(files)
        assert not status.any()
        res["c_compress"] = t
        res["c_archive_bytes"] = wrote.value
        res["c_batch_bytes"] = int(out_len.sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
