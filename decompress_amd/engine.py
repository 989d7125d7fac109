"""Batch engine: device buffers in, device buffers out (torch is only the
allocator / stream provider here; the work is done by libmdeflate.so)."""
import contextlib
import ctypes

import numpy as _np

from . import _lib

FORMAT_DEFLATE = 0
FORMAT_ZLIB = 1
FORMAT_GZIP = 2
MATCHER_DE, MATCHER_LZ = 0, 1
DRIVER_ZL, DRIVER_HIGHER, DRIVER_CLI = 0, 1, 2
SHA1_LAUNCH_BLOCKS = 4096  # the default of set_option("sha1_launch_blocks") (mdeflate.h)

# variant names of De.Inf.Ns.error (lib/de.ml:1548-1555) + Zl.Inf.Ns.error (lib/zl.ml:383)
STATUS_NAMES = {
    0: "Ok", 1: "Unexpected_end_of_input", 2: "Unexpected_end_of_output",
    3: "Invalid_kind_of_block", 4: "Invalid_dictionary",
    5: "Invalid_complement_of_length", 6: "Invalid_distance",
    7: "Invalid_distance_code", 8: "Invalid_header", 9: "Invalid_checksum",
    10: "Invalid GZip header", 11: "Invalid GZip header checksum", 12: "Invalid input size",
    13: "Queue.Full", 14: "Invalid input", 15: "No dictionary at offset 0 available",
    16: "Input is malformed or output is not large enough", 17: "Malformed input",
    18: "Invalid ZIP directory", 19: "Invalid ZIP local header", 20: "Unsupported ZIP entry",
    21: "Invalid index", 22: "Invalid pack", 23: "Invalid delta", 24: "Invalid delta base", 25: "Missing delta base",
    26: "Unsupported pack",
}
STATUS_CODES = {v: k for k, v in STATUS_NAMES.items()}


class Error(RuntimeError):
    """Call-level failure (the reference raises Invalid_argument / Failure)."""


class _HostArray(_np.ndarray):
    """numpy view of a pinned block of md_host_alloc; carries the owner that frees it"""

    def __array_finalize__(self, obj):
        self._md_owner = getattr(obj, "_md_owner", None)


def _check_blob(a, name):
    """The host entry points take the blob's address and byte count: it has to be a C-contiguous uint8 array (a strided
    view or another dtype would hand the library a wrong extent)."""
    if not isinstance(a, _np.ndarray) or a.dtype != _np.uint8 or not a.flags["C_CONTIGUOUS"]:
        raise TypeError("%s must be a C-contiguous numpy uint8 array" % name)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


class Engine:
    """One engine per GPU (wraps md_ctx).  Kernels are enqueued on torch's current stream of `device` — the
    legacy default stream included (MD_STREAM_NULL), so batch calls are ordered with the torch kernels that
    produce their inputs and consume their results — unless own_stream=True (then the caller synchronises)."""

    def __init__(self, device=0, own_stream=False):
        import torch

        self.torch = torch
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise Error("decompress_amd needs a HIP device (no CPU fallback)")
        self.device = torch.device("cuda", device)
        self.own_stream = bool(own_stream)
        if own_stream:
            handle = None
        else:
            stream = torch.cuda.current_stream(self.device).cuda_stream
            handle = ctypes.c_void_p(stream) if stream else ctypes.c_void_p(_lib.MD_STREAM_NULL)
        self.ctx = self.lib.md_create(device, handle)
        if not self.ctx:
            raise Error(self.lib.md_last_error_string(None).decode())

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.md_destroy(self.ctx)
            self.ctx = None

    __del__ = close

    def _check(self, rc):
        if rc != 0:
            raise Error("%s: %s" % (self.lib.md_status_string(rc).decode(),
                                    self.lib.md_last_error_string(self.ctx).decode()))

    def lzo_batch(self, compress, d_in, in_off, in_len, d_out, out_off, out_cap, results=None):
        """Lzo.compress / Lzo.uncompress over n device-resident buffers -> (out_len, status) CUDA tensors (async)."""
        torch = self.torch
        n = in_off.numel()
        if results is None:
            results = (torch.empty(n, dtype=torch.int64, device=self.device),
                       torch.empty(n, dtype=torch.int32, device=self.device))
        fn = self.lib.md_lzo_compress_batch_device if compress else self.lib.md_lzo_uncompress_batch_device
        self._check(fn(self.ctx, n, _ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out), _ptr(out_off), _ptr(out_cap),
                       _ptr(results[0]), _ptr(results[1])))
        return results

    def lzo_sizes(self, d_in, in_off, in_len, results=None):
        """md_lzo_sizes_batch_device: every stream's uncompressed size without decoding it, with the statuses of
        Lzo.uncompress_with_buffer.  CUDA tensors as lzo_batch; returns (out_len, status) CUDA tensors (async)."""
        torch = self.torch
        n = in_off.numel()
        if results is None:
            results = (torch.empty(n, dtype=torch.int64, device=self.device),
                       torch.empty(n, dtype=torch.int32, device=self.device))
        self._check(self.lib.md_lzo_sizes_batch_device(self.ctx, n, _ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(results[0]),
                                                       _ptr(results[1])))
        return results

    def lzo_sizes_host(self, streams):
        """md_lzo_sizes_batch_host on a list of bytes: [(status, out_len)].  Synchronous."""
        import numpy as np

        n = len(streams)
        if n == 0:
            return []
        in_len = np.array([len(s) for s in streams], dtype=np.uint64)
        in_off = np.zeros(n, dtype=np.uint64)
        np.cumsum(in_len[:-1], out=in_off[1:])
        blob = np.frombuffer(b"".join(bytes(s) for s in streams) + bytes(16), dtype=np.uint8)
        out_len, status = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int32)
        self._check(self.lib.md_lzo_sizes_batch_host(self.ctx, n, blob.ctypes.data, blob.nbytes, in_off.ctypes.data,
                                                     in_len.ctypes.data, out_len.ctypes.data, status.ctypes.data))
        return [(int(status[i]), int(out_len[i])) for i in range(n)]

    def lzo_many(self, compress, bufs, caps):
        """Convenience for tests: list of bytes -> list of (status, bytes).  Uncompress with caps=None: the room comes
        from the streams themselves (lzo_sizes, inflate_plan, one read-back, then the decode)."""
        import numpy as np

        torch = self.torch
        n = len(bufs)
        if n == 0:
            return []
        in_len = np.array([len(s) for s in bufs], dtype=np.int64)
        in_off = np.zeros(n, dtype=np.int64)
        np.cumsum(((in_len + 31) // 16 * 16)[:-1], out=in_off[1:])
        if caps is None:
            if compress:
                raise Error("Invalid argument: Lzo.compress needs the caller's room")
            return self._lzo_many_sized(bufs, in_off, in_len)[0]
        cap = np.array(caps, dtype=np.int64)
        out_off = np.zeros(n, dtype=np.int64)
        np.cumsum(((cap + 255) // 256 * 256)[:-1], out=out_off[1:])
        blob = np.zeros(int(in_off[-1] + in_len[-1]) + 32, dtype=np.uint8)
        for s, o in zip(bufs, in_off):
            blob[o:o + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
        dev = self.device
        t = lambda a: torch.from_numpy(a).to(dev)
        d_out = torch.zeros(int(out_off[-1] + cap[-1]) + 32, dtype=torch.uint8, device=dev)
        out_len, status = self.lzo_batch(compress, t(blob), t(in_off), t(in_len), d_out, t(out_off), t(cap))
        torch.cuda.synchronize(dev)
        out = d_out.cpu().numpy()
        out_len, status = out_len.cpu().numpy(), status.cpu().numpy()
        return [(int(status[i]), out[out_off[i]:out_off[i] + out_len[i]].tobytes()) for i in range(n)]

    def _lzo_many_sized(self, bufs, in_off, in_len, align=256):
        """-> ([(status, bytes)], out_off, total): a stream's status is the size call's; the decode of a stream the size
        call called valid can only report Ok and the same length"""
        import numpy as np

        torch, dev = self.torch, self.device
        n = len(bufs)
        blob = np.zeros(int(in_off[-1] + in_len[-1]) + 32, dtype=np.uint8)
        for s, o in zip(bufs, in_off):
            blob[o:o + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
        d_in = torch.from_numpy(blob).to(dev)
        d_off, d_len = torch.from_numpy(in_off).to(dev), torch.from_numpy(in_len).to(dev)
        if self.own_stream:
            torch.cuda.synchronize(dev)
        sizes, s_status = self.lzo_sizes(d_in, d_off, d_len)
        out_off, out_cap, total = self.inflate_plan(sizes, align)
        self.synchronize()
        total = int(total.item())
        d_out = torch.zeros(total + 32, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        out_len, status = self.lzo_batch(False, d_in, d_off, d_len, d_out, out_off, out_cap)
        self.synchronize()
        torch.cuda.synchronize(dev)
        out, out_off = d_out.cpu().numpy(), out_off.cpu().numpy()
        sizes, s_status = sizes.cpu().numpy(), s_status.cpu().numpy()
        out_len, status = out_len.cpu().numpy(), status.cpu().numpy()
        ok = s_status == 0
        if not ((status[ok] == 0).all() and (out_len[ok] == sizes[ok]).all()):
            raise Error("lzo: the decode disagrees with the size call")
        res = [(int(s_status[i]), out[out_off[i]:out_off[i] + sizes[i]].tobytes() if ok[i] else b"") for i in range(n)]
        return res, out_off, total

    def set_matcher(self, matcher):
        """Default matcher of this Engine object's later deflate calls: 0 = De.Lz77, 1 = Lz (lib/lz.ml).  Kept on the
        Python side — the C ABI takes the matcher per call (md_deflate_params)."""
        if matcher not in (MATCHER_DE, MATCHER_LZ):
            raise Error("Invalid argument: unknown matcher")
        self._matcher = int(matcher)

    def gz_set_header(self, mtime=0, os=3, hcrc=False, ascii=False, filename=None, comment=None):
        """Default GZip header of this Engine object's later FORMAT_GZIP deflate calls (Gz.Def.encoder's fields,
        lib/gz.ml:859-918); passed per call through md_deflate_params.gz_header."""
        self._gz = dict(mtime=int(mtime) & 0xffffffff, os=int(os), hcrc=int(bool(hcrc)), ascii=int(bool(ascii)),
                        filename=filename, comment=comment)

    def _params(self, level, queue, driver, dynamic, matcher=None, header=None, total_in=0):
        h = header if header is not None else getattr(self, "_gz", None)
        gz = _lib.GzHeader(**h) if h else None
        p = _lib.DeflateParams(int(level), int(queue), int(driver), int(bool(dynamic)),
                               int(getattr(self, "_matcher", MATCHER_DE) if matcher is None else matcher),
                               ctypes.pointer(gz) if gz is not None else None, 0, int(total_in))
        p._keep = gz  # the struct must outlive the call
        return p

    def crc32_batch(self, d_data, d_off, d_len):
        """Checkseum.Crc32 of n device-resident buffers -> uint32 tensor (device)."""
        n = d_off.numel()
        crc = self.torch.empty(n, dtype=self.torch.int32, device=self.device)
        self._check(self.lib.md_crc32_batch_device(self.ctx, n, _ptr(d_data), _ptr(d_off), _ptr(d_len), _ptr(crc)))
        return crc

    def sha1_batch(self, bufs, types=None):
        """md_sha1_batch_host on a list of bytes -> [20-byte digest]: SHA-1 of each buffer as it is, or with types[i] in
        1 .. 4 its name as a git commit / tree / blob / tag.  Synchronous."""
        n = len(bufs)
        if types is not None and len(types) != n:
            raise Error("Invalid argument: one type per buffer")
        in_len = _np.array([len(b) for b in bufs], dtype=_np.uint64)
        in_off = _np.zeros(max(n, 1), dtype=_np.uint64)
        if n > 1:
            _np.cumsum(in_len[:-1], out=in_off[1:])
        blob = _np.frombuffer(b"".join(bytes(b) for b in bufs), dtype=_np.uint8)
        if types is not None and any(not 0 <= int(t) <= 255 for t in types):
            raise Error("Invalid argument: a type is 0 .. 4")
        typ = None if types is None else _np.array([int(t) for t in types] or [0], dtype=_np.uint8)
        digest = _np.zeros(20 * max(n, 1), dtype=_np.uint8)
        self._check(self.lib.md_sha1_batch_host(self.ctx, n, blob.ctypes.data if blob.size else None, blob.size, in_off.ctypes.data,
                                                in_len.ctypes.data if n else None, typ.ctypes.data if typ is not None else None,
                                                digest.ctypes.data))
        return [digest[20 * i:20 * i + 20].tobytes() for i in range(n)]

    def sha1_batch_device(self, d_data, d_off, d_len, d_type, max_len):
        """md_sha1_batch_device: n device-resident buffers -> uint8 tensor of 20 n bytes (device, async).  d_type may be None;
        max_len bounds every length (it sets the number of launches)."""
        n = d_off.numel()
        digest = self.torch.empty(20 * n, dtype=self.torch.uint8, device=self.device)
        self._check(self.lib.md_sha1_batch_device(self.ctx, n, _ptr(d_data), _ptr(d_off), _ptr(d_len), _ptr(d_type), int(max_len), _ptr(digest)))
        return digest

    def sha1_last(self):
        """md_sha1_last: messages, blocks, launches, device_ns of the last SHA-1 batch (a pack read's hash passes included)"""
        s = _lib.Sha1Stats()
        self._check(self.lib.md_sha1_last(self.ctx, ctypes.byref(s)))
        return {k: getattr(s, k) for k in ("messages", "blocks", "launches", "device_ns")}

    @staticmethod
    def _delta_rows(pairs, fields=(), caps=None):
        """md_pack_delta_pair rows: base_off, base_len, tgt_off, tgt_len and then `fields` from each of pairs, out_cap from caps"""
        rows = (_lib.PackDeltaPair * max(len(pairs), 1))()
        for i, (r, p) in enumerate(zip(rows, pairs)):
            for f, v in zip(("base_off", "base_len", "tgt_off", "tgt_len") + fields, p, strict=True):
                setattr(r, f, int(v))
            if caps is not None:
                r.out_cap = int(caps[i])
        return rows

    @staticmethod
    def _ranges(objects):
        """objects = [(off, len)] -> the offsets and the lengths as the sketch calls take them"""
        u64s = ctypes.c_uint64 * max(len(objects), 1)
        return u64s(*[int(o) for o, _ in objects]), u64s(*[int(k) for _, k in objects])

    def pack_deltas(self, src, pairs, caps=None):
        """md_pack_delta_batch_host: the deltas of pairs = [(base_off, base_len, tgt_off, tgt_len)] into the bytes `src` ->
        [(status, delta bytes)], status 0 = Ok, 2 = the delta passed its room (then no bytes).  caps[i]: the room of delta i;
        default tgt_len + tgt_len // 127 + 16, which always suffices (nothing but inserts).  Synchronous."""
        n = len(pairs)
        src = bytes(src)
        if caps is None:
            caps = [p[3] + p[3] // 127 + 16 for p in pairs]
        if len(caps) != n:
            raise Error("Invalid argument: one room per pair")
        rows, at = self._delta_rows(pairs, caps=caps), 0
        for r in rows[:n]:
            r.out_off = at
            at += (r.out_cap + 15) & ~15
        out = ctypes.create_string_buffer(max(at, 1))
        out_len, status = (ctypes.c_uint64 * max(n, 1))(), (ctypes.c_int32 * max(n, 1))()
        self._check(self.lib.md_pack_delta_batch_host(self.ctx, n, rows, src, len(src), out, at, out_len, status))
        raw = out.raw
        return [(status[i], raw[rows[i].out_off:rows[i].out_off + out_len[i]]) for i in range(n)]

    def pack_deltas_device(self, pairs, d_src, d_out):
        """md_pack_delta_batch_device: pairs = [(base_off, base_len, tgt_off, tgt_len, out_off, out_cap)] (host) into the device
        tensors d_src / d_out -> (out_len int64 tensor, status int32 tensor), device, async"""
        n = len(pairs)
        rows = self._delta_rows(pairs, ("out_off", "out_cap"))
        out_len = self.torch.zeros(max(n, 1), dtype=self.torch.int64, device=self.device)
        status = self.torch.zeros(max(n, 1), dtype=self.torch.int32, device=self.device)
        self._check(self.lib.md_pack_delta_batch_device(self.ctx, n, rows, _ptr(d_src), _ptr(d_out), _ptr(out_len), _ptr(status)))
        return out_len[:n], status[:n]

    def pack_write_last(self):
        """md_pack_write_last: pairs, kept, dropped_size, dropped_depth, payload_before, payload_after, launches, delta_ns of the
        last pack written or delta batch made"""
        s = _lib.PackWriteStats()
        self._check(self.lib.md_pack_write_last(self.ctx, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in _lib.PackWriteStats._fields_}

    def pack_sketch(self, src, objects):
        """md_pack_sketch_host: the four features of every object (off, len) of the bytes `src` -> [(F0, F1, F2, F3)]; an
        object shorter than 16 bytes has none, its words are all ones.  Synchronous."""
        n, src = len(objects), bytes(src)
        off, length = self._ranges(objects)
        feats = (ctypes.c_uint32 * (4 * max(n, 1)))()
        self._check(self.lib.md_pack_sketch_host(self.ctx, n, off, length, src, len(src), feats))
        return [tuple(feats[4 * i:4 * i + 4]) for i in range(n)]

    def pack_sketch_device(self, objects, d_src):
        """md_pack_sketch_device: objects = [(off, len)] (host) in the device tensor d_src -> int32 tensor of 4 n words (the
        features' bit patterns), device, async"""
        n = len(objects)
        off, length = self._ranges(objects)
        feats = self.torch.zeros(4 * max(n, 1), dtype=self.torch.int32, device=self.device)
        self._check(self.lib.md_pack_sketch_device(self.ctx, n, off, length, _ptr(d_src), _ptr(feats)))
        return feats[:4 * n]

    def pack_delta_sizes(self, src, pairs, caps=None):
        """md_pack_delta_sizes_host: what `pack_deltas` would report for pairs = [(base_off, base_len, tgt_off, tgt_len)] of the
        bytes `src`, without the deltas -> [(status, length)], status 2 and length 0 where the delta would pass caps[i]
        (default: no bound).  Synchronous."""
        n, src = len(pairs), bytes(src)
        if caps is None:
            caps = [(1 << 64) - 1] * n
        if len(caps) != n:
            raise Error("Invalid argument: one bound per pair")
        rows = self._delta_rows(pairs, caps=caps)
        out_len, status = (ctypes.c_uint64 * max(n, 1))(), (ctypes.c_int32 * max(n, 1))()
        self._check(self.lib.md_pack_delta_sizes_host(self.ctx, n, rows, src, len(src), out_len, status))
        return [(status[i], out_len[i]) for i in range(n)]

    def pack_delta_sizes_device(self, pairs, d_src):
        """md_pack_delta_sizes_device: pairs = [(base_off, base_len, tgt_off, tgt_len, out_cap)] (host) in the device tensor
        d_src -> (out_len int64 tensor, status int32 tensor), device, async"""
        n = len(pairs)
        rows = self._delta_rows(pairs, ("out_cap",))
        out_len = self.torch.zeros(max(n, 1), dtype=self.torch.int64, device=self.device)
        status = self.torch.zeros(max(n, 1), dtype=self.torch.int32, device=self.device)
        self._check(self.lib.md_pack_delta_sizes_device(self.ctx, n, rows, _ptr(d_src), _ptr(out_len), _ptr(status)))
        return out_len[:n], status[:n]

    def pack_search_last(self):
        """md_pack_search_last: featured, pairs, fitted, chosen, launches, sketch_ns, score_ns, host_ns of the last
        `pack.choose_bases`"""
        s = _lib.PackSearchStats()
        self._check(self.lib.md_pack_search_last(self.ctx, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in _lib.PackSearchStats._fields_}

    def set_option(self, key, value):
        self._check(self.lib.md_set_option(self.ctx, key.encode(), int(value)))
        if key == "deflate_span_prime":  # (the library has no query: `deflate_spans(prime=)` puts this back)
            self._span_prime = int(value)

    @contextlib.contextmanager
    def _primed(self, prime):
        """`prime` of deflate_spans*: None leaves the option "deflate_span_prime" as it is, True / False sets it for the
        call and puts the old value back"""
        old = getattr(self, "_span_prime", 0)
        if prime is None or int(bool(prime)) == old:
            yield
            return
        self.set_option("deflate_span_prime", int(bool(prime)))
        try:
            yield
        finally:
            self.set_option("deflate_span_prime", old)

    PROFILE_FIELDS = ["cyc_ensure", "cyc_decode1", "cyc_decode2", "cyc_emit_a", "cyc_far", "cyc_near",
                      "cyc_adler", "cyc_header", "cyc_near_fast", "cyc_near_slow", "cyc_near_upd", "cyc_near_load", "cyc_hdr_lens", "cyc_hdr_lit", "cyc_far_rec", "cyc_far_load", "cyc_wait_dec", "cyc_wait_copy", "rounds", "passes", "lanes", "tokens", "slots",
                      "near_iters", "end_chain", "end_fit", "end_records", "end_stage", "end_eob", "long_near", "far_spill"]

    def get_profile(self):
        """In-kernel phase profile of stream 0 (enable with set_option('profile', 1))."""
        buf = (ctypes.c_uint64 * 32)()
        self._check(self.lib.md_get_profile(self.ctx, buf))
        return dict(zip(self.PROFILE_FIELDS, list(buf)))

    def get_profile_raw(self):
        """The 32 raw profile words (the deflate kernel's layout differs from the inflate one)."""
        buf = (ctypes.c_uint64 * 32)()
        self._check(self.lib.md_get_profile(self.ctx, buf))
        return list(buf)

    def synchronize(self):
        self._check(self.lib.md_synchronize(self.ctx))

    def timing_begin(self):
        self._check(self.lib.md_timing_begin(self.ctx))

    def timing_end(self):
        ms = ctypes.c_float()
        self._check(self.lib.md_timing_end(self.ctx, ctypes.byref(ms)))
        return ms.value

    # ------------------------------------------------------------------ inflate
    def inflate_batch(self, fmt, d_in, in_off, in_len, d_out, out_off, out_cap, results=None):
        """All arguments are CUDA tensors: d_in/d_out uint8, descriptors int64.
        Returns (out_len, consumed, status, checksum) CUDA tensors (async)."""
        torch = self.torch
        n = in_off.numel()
        if results is None:
            results = (torch.empty(n, dtype=torch.int64, device=self.device),
                       torch.empty(n, dtype=torch.int64, device=self.device),
                       torch.empty(n, dtype=torch.int32, device=self.device),
                       torch.empty(n, dtype=torch.int32, device=self.device))
        out_len, consumed, status, checksum = results
        self._check(self.lib.md_inflate_batch_device(
            self.ctx, fmt, n, _ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(d_out), _ptr(out_off),
            _ptr(out_cap), _ptr(out_len), _ptr(consumed), _ptr(status), _ptr(checksum)))
        return results

    # ------------------------------------------------------------------ host buffers (md_*_batch_host)
    def host_buffer(self, nbytes):
        """A pinned host buffer of nbytes (md_host_alloc) as a numpy uint8 array; the array owns it (freed with it)."""
        import numpy as np

        p = self.lib.md_host_alloc(self.ctx, nbytes)
        if not p:
            raise MemoryError("md_host_alloc(%d)" % nbytes)
        lib, ctx = self.lib, self.ctx

        class _Owner:
            def __init__(self):
                self.buf = (ctypes.c_uint8 * max(1, nbytes)).from_address(p)

            def __del__(self):
                lib.md_host_free(None, p)  # (the context may be gone by now: md_host_free does not use it)

        owner = _Owner()
        a = np.frombuffer(owner.buf, dtype=np.uint8, count=nbytes)
        a = a.view(_HostArray)
        a._md_owner = owner  # the array (and every view of it) keeps the pinned block alive; it goes when they do
        return a

    def inflate_batch_host(self, fmt, h_in, in_off, in_len, h_out, out_off, out_cap):
        """md_inflate_batch_host: numpy uint8 blobs (pinned ones overlap copies and kernels) and uint64 descriptor arrays.
        Returns (out_len, consumed, status, checksum) numpy arrays.  Synchronous."""
        import numpy as np

        n = len(in_off)
        _check_blob(h_in, "h_in"), _check_blob(h_out, "h_out")
        u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
        in_off, in_len, out_off, out_cap = u64(in_off), u64(in_len), u64(out_off), u64(out_cap)
        out_len, consumed = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        status, checksum = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint32)
        self._check(self.lib.md_inflate_batch_host(
            self.ctx, fmt, n, h_in.ctypes.data, h_in.nbytes, in_off.ctypes.data, in_len.ctypes.data, h_out.ctypes.data,
            h_out.nbytes, out_off.ctypes.data, out_cap.ctypes.data, out_len.ctypes.data, consumed.ctypes.data,
            status.ctypes.data, checksum.ctypes.data))
        return out_len, consumed, status, checksum

    def deflate_batch_host(self, fmt, h_in, in_off, in_len, h_out, out_off, out_cap, level=6, queue=4096, driver=DRIVER_ZL,
                           dynamic=True, matcher=None, header=None):
        """md_deflate_batch_host, as inflate_batch_host.  Returns (out_len, status, checksum of the input)."""
        import numpy as np

        n = len(in_off)
        _check_blob(h_in, "h_in"), _check_blob(h_out, "h_out")
        u64 = lambda a: np.ascontiguousarray(a, dtype=np.uint64)
        in_off, in_len, out_off, out_cap = u64(in_off), u64(in_len), u64(out_off), u64(out_cap)
        out_len = np.zeros(n, dtype=np.uint64)
        status, checksum = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint32)
        params = self._params(level, queue, driver, dynamic, matcher, header, 0)
        self._check(self.lib.md_deflate_batch_host(
            self.ctx, fmt, ctypes.byref(params), n, h_in.ctypes.data, h_in.nbytes, in_off.ctypes.data, in_len.ctypes.data,
            h_out.ctypes.data, h_out.nbytes, out_off.ctypes.data, out_cap.ctypes.data, out_len.ctypes.data,
            status.ctypes.data, checksum.ctypes.data))
        return out_len, status, checksum

    def inflate_sizes(self, fmt, d_in, in_off, in_len, results=None):
        """md_inflate_sizes_batch_device: every stream's inflated size without decoding it.  CUDA tensors as
        inflate_batch; returns (out_len, consumed, status) CUDA tensors (async)."""
        torch = self.torch
        n = in_off.numel()
        if results is None:
            results = (torch.empty(n, dtype=torch.int64, device=self.device),
                       torch.empty(n, dtype=torch.int64, device=self.device),
                       torch.empty(n, dtype=torch.int32, device=self.device))
        out_len, consumed, status = results
        self._check(self.lib.md_inflate_sizes_batch_device(
            self.ctx, fmt, n, _ptr(d_in), _ptr(in_off), _ptr(in_len), _ptr(out_len), _ptr(consumed), _ptr(status)))
        return results

    def inflate_plan(self, out_len, align=256):
        """md_inflate_plan_device: (out_off, out_cap, total) for inflate_batch from the sizes; `total` is a one-element
        CUDA tensor, the bytes to allocate (async)."""
        torch = self.torch
        n = out_len.numel()
        out_off = torch.empty(n, dtype=torch.int64, device=self.device)
        out_cap = torch.empty(n, dtype=torch.int64, device=self.device)
        total = torch.empty(1, dtype=torch.int64, device=self.device)
        self._check(self.lib.md_inflate_plan_device(self.ctx, n, _ptr(out_len), int(align), _ptr(out_off), _ptr(out_cap), _ptr(total)))
        return out_off, out_cap, total

    def inflate_sizes_host(self, fmt, streams):
        """md_inflate_sizes_batch_host on a list of bytes: [(status, consumed, out_len)].  Synchronous."""
        import numpy as np

        n = len(streams)
        if n == 0:
            return []
        in_len = np.array([len(s) for s in streams], dtype=np.uint64)
        in_off = np.zeros(n, dtype=np.uint64)
        np.cumsum(in_len[:-1], out=in_off[1:])
        blob = np.frombuffer(b"".join(bytes(s) for s in streams) + bytes(16), dtype=np.uint8)
        out_len, consumed, status = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int32)
        self._check(self.lib.md_inflate_sizes_batch_host(
            self.ctx, fmt, n, blob.ctypes.data, blob.nbytes, in_off.ctypes.data, in_len.ctypes.data, out_len.ctypes.data,
            consumed.ctypes.data, status.ctypes.data))
        return [(int(status[i]), int(consumed[i]), int(out_len[i])) for i in range(n)]

    def inflate_many(self, streams, caps=None, fmt=FORMAT_DEFLATE):
        """Convenience for tests: list of bytes -> list of (status, consumed, bytes, adler).  caps=None: the room comes
        from the streams themselves (inflate_sizes, inflate_plan, then the decode)."""
        import numpy as np

        torch = self.torch
        n = len(streams)
        if n == 0:
            return []
        in_len = np.array([len(s) for s in streams], dtype=np.int64)
        in_off = np.zeros(n, dtype=np.int64)
        np.cumsum(((in_len + 15) // 16 * 16)[:-1], out=in_off[1:])
        if caps is None:
            return self._inflate_many_sized(streams, in_off, in_len, fmt)
        cap = np.array(caps, dtype=np.int64)
        out_off = np.zeros(n, dtype=np.int64)
        np.cumsum(((cap + 255) // 256 * 256)[:-1], out=out_off[1:])
        blob = np.zeros(int(in_off[-1] + in_len[-1]) + 16, dtype=np.uint8)
        for s, o in zip(streams, in_off):
            blob[o:o + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
        dev = self.device
        d_in = torch.from_numpy(blob).to(dev)
        d_out = torch.zeros(int(out_off[-1] + cap[-1]) + 16, dtype=torch.uint8, device=dev)
        t = lambda a: torch.from_numpy(a).to(dev)
        args = (fmt, d_in, t(in_off), t(in_len), d_out, t(out_off), t(cap))
        if self.own_stream:  # torch's fills and copies above ran on ITS stream: they come first (the caller synchronises, i.e. we)
            torch.cuda.synchronize(dev)
        out_len, consumed, status, checksum = self.inflate_batch(*args)
        torch.cuda.synchronize(dev)
        out = d_out.cpu().numpy()
        out_len, consumed, status = out_len.cpu().numpy(), consumed.cpu().numpy(), status.cpu().numpy()
        checksum = checksum.cpu().numpy().view(np.uint32)
        return [(int(status[i]), int(consumed[i]),
                 out[out_off[i]:out_off[i] + out_len[i]].tobytes(), int(checksum[i]))
                for i in range(n)]

    def _inflate_many_sized(self, streams, in_off, in_len, fmt):
        import numpy as np

        torch, dev = self.torch, self.device
        n = len(streams)
        blob = np.zeros(int(in_off[-1] + in_len[-1]) + 16, dtype=np.uint8)
        for s, o in zip(streams, in_off):
            blob[o:o + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
        d_in = torch.from_numpy(blob).to(dev)
        d_off, d_len = torch.from_numpy(in_off).to(dev), torch.from_numpy(in_len).to(dev)
        if self.own_stream:
            torch.cuda.synchronize(dev)
        sizes, _, _ = self.inflate_sizes(fmt, d_in, d_off, d_len)
        out_off, out_cap, total = self.inflate_plan(sizes, 256)
        self.synchronize()
        d_out = torch.zeros(int(total.item()) + 16, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        out_len, consumed, status, checksum = self.inflate_batch(fmt, d_in, d_off, d_len, d_out, out_off, out_cap)
        self.synchronize()
        torch.cuda.synchronize(dev)
        out, out_off = d_out.cpu().numpy(), out_off.cpu().numpy()
        out_len, consumed, status = out_len.cpu().numpy(), consumed.cpu().numpy(), status.cpu().numpy()
        checksum = checksum.cpu().numpy().view(np.uint32)
        return [(int(status[i]), int(consumed[i]), out[out_off[i]:out_off[i] + out_len[i]].tobytes(), int(checksum[i]))
                for i in range(n)]

    # ------------------------------------------------------------------ deflate
    def deflate_batch(self, fmt, d_in, in_off, in_len, d_out, out_off, out_cap, level=6, queue=4096,
                      driver=DRIVER_ZL, dynamic=True, results=None, matcher=None, header=None, total_in=0):
        """All arguments are CUDA tensors (uint8 data, int64 descriptors).
        Returns (out_len, status, adler32_of_input) CUDA tensors (async).  total_in: an upper bound of in_len.sum()
        when the caller knows it (md_deflate_params.total_in_bytes); 0 makes the engine read the sum back first."""
        torch = self.torch
        n = in_off.numel()
        if results is None:
            results = (torch.empty(n, dtype=torch.int64, device=self.device),
                       torch.empty(n, dtype=torch.int32, device=self.device),
                       torch.empty(n, dtype=torch.int32, device=self.device))
        out_len, status, checksum = results
        params = self._params(level, queue, driver, dynamic, matcher, header, total_in)
        self._check(self.lib.md_deflate_batch_device(
            self.ctx, fmt, ctypes.byref(params), n, _ptr(d_in), _ptr(in_off), _ptr(in_len),
            _ptr(d_out), _ptr(out_off), _ptr(out_cap), _ptr(out_len), _ptr(status), _ptr(checksum)))
        return results

    def deflate_many(self, bufs, fmt=FORMAT_DEFLATE, level=6, queue=4096, driver=DRIVER_ZL, dynamic=True,
                     caps=None, matcher=None, header=None):
        """Convenience for tests: list of bytes -> list of (status, compressed bytes, adler32 of input)."""
        import numpy as np

        torch = self.torch
        n = len(bufs)
        if n == 0:
            return []
        in_len = np.array([len(s) for s in bufs], dtype=np.int64)
        in_off = np.zeros(n, dtype=np.int64)
        np.cumsum(((in_len + 15) // 16 * 16)[:-1], out=in_off[1:])
        if caps is None:
            caps = [2 * len(s) + 8192 for s in bufs]
        cap = np.array(caps, dtype=np.int64)
        out_off = np.zeros(n, dtype=np.int64)
        np.cumsum(((cap + 255) // 256 * 256)[:-1], out=out_off[1:])
        blob = np.zeros(int(in_off[-1] + in_len[-1]) + 16, dtype=np.uint8)
        for s, o in zip(bufs, in_off):
            blob[o:o + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
        dev = self.device
        d_in = torch.from_numpy(blob).to(dev)
        d_out = torch.zeros(int(out_off[-1] + cap[-1]) + 16, dtype=torch.uint8, device=dev)
        t = lambda a: torch.from_numpy(a).to(dev)
        d_off, d_len, d_ooff, d_cap = t(in_off), t(in_len), t(out_off), t(cap)
        if self.own_stream:
            torch.cuda.synchronize(dev)
        out_len, status, checksum = self.deflate_batch(fmt, d_in, d_off, d_len, d_out, d_ooff, d_cap,
                                                       level, queue, driver, dynamic, matcher=matcher, header=header,
                                                       total_in=max(1, int(in_len.sum())))
        torch.cuda.synchronize(dev)
        out = d_out.cpu().numpy()
        out_len, status = out_len.cpu().numpy(), status.cpu().numpy()
        checksum = checksum.cpu().numpy().view(np.uint32)
        return [(int(status[i]), out[out_off[i]:out_off[i] + out_len[i]].tobytes(), int(checksum[i]))
                for i in range(n)]

    def deflate_one(self, data, fmt=FORMAT_DEFLATE, level=6, queue=4096, driver=DRIVER_ZL, dynamic=True, cap=None,
                    matcher=None, header=None):
        """ONE stream through md_deflate_batch_host (host buffers: what md_*_higher_compress do; a long stream gets its hash
        chains from the whole chip) -> (status, compressed bytes, checksum of the input)."""
        import numpy as np

        n = len(data)
        src = np.frombuffer(bytes(data), dtype=np.uint8) if n else np.zeros(1, dtype=np.uint8)
        cap = 2 * n + 8192 if cap is None else int(cap)
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        out_len, status, checksum = self.deflate_batch_host(fmt, src, [0], [n], out, [0], [cap], level, queue, driver, dynamic,
                                                            matcher, header)
        return int(status[0]), out[:int(out_len[0])].tobytes(), int(checksum[0])

    def deflate_spans_bound(self, n, fmt=FORMAT_DEFLATE, span=None, header=None):
        """md_deflate_spans_bound: room that always suffices for `deflate_spans` of n bytes (host arithmetic)"""
        h = header if header is not None else getattr(self, "_gz", None)
        gz = _lib.GzHeader(**h) if h and fmt == FORMAT_GZIP else None
        return int(self.lib.md_deflate_spans_bound(fmt, n, int(span or 0), ctypes.byref(gz) if gz is not None else None))

    def deflate_spans(self, data, fmt=FORMAT_DEFLATE, span=None, level=6, queue=4096, driver=DRIVER_ZL, dynamic=True,
                      matcher=None, header=None, cap=None, prime=None):
        """ONE standard stream of `data` written as joined spans on the whole chip (md_deflate_spans_host):
        `span` bytes of text per span (None: the option "deflate_span_kib") -> (status, stream bytes, checksum of the
        input: Adler-32, CRC-32 for FORMAT_GZIP).  cap: room of the destination (default: the bound).  prime: every span's
        matcher starts from the 32 KiB of text in front of it (None: the option "deflate_span_prime"; True / False: for
        this call)."""
        data = data if isinstance(data, bytes) else bytes(data)
        params = self._params(level, queue, driver, dynamic, matcher, header)
        if cap is None:
            cap = self.deflate_spans_bound(len(data), fmt, span, header)
            if cap == 0:  # (bad arguments: the call says which)
                cap = 1
        dst = ctypes.create_string_buffer(max(int(cap), 1))
        wrote, sum_ = ctypes.c_size_t(), ctypes.c_uint32()
        with self._primed(prime):
            st = self.lib.md_deflate_spans_host(self.ctx, fmt, ctypes.byref(params), int(span or 0), data, len(data), dst, int(cap),
                                                ctypes.byref(wrote), ctypes.byref(sum_))
        if st < 0:
            self._check(st)
        return int(st), dst.raw[:wrote.value], int(sum_.value)

    def deflate_spans_device(self, d_src, n, d_dst, fmt=FORMAT_DEFLATE, span=None, level=6, queue=4096, driver=DRIVER_ZL,
                             dynamic=True, matcher=None, header=None, prime=None):
        """md_deflate_spans_device: the first n bytes of the CUDA uint8 tensor d_src into the CUDA uint8 tensor d_dst, nothing
        read back -> (written, status, checksum) CUDA tensors of one element (async on the engine's stream).  prime: as
        `deflate_spans`'s."""
        torch = self.torch
        written = torch.zeros(1, dtype=torch.int64, device=self.device)
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        checksum = torch.zeros(1, dtype=torch.int32, device=self.device)
        params = self._params(level, queue, driver, dynamic, matcher, header)
        with self._primed(prime):
            self._check(self.lib.md_deflate_spans_device(self.ctx, fmt, ctypes.byref(params), int(span or 0), _ptr(d_src), int(n),
                                                         _ptr(d_dst), d_dst.numel(), _ptr(written), _ptr(status), _ptr(checksum)))
        return written, status, checksum

    def deflate_spans_last(self):
        """md_deflate_spans_last -> dict: spans, stored_spans, span_bytes of the last deflate_spans* call"""
        info = _lib.DeflateSpansInfo()
        self._check(self.lib.md_deflate_spans_last(self.ctx, ctypes.byref(info)))
        return {k: int(getattr(info, k)) for k, _ in _lib.DeflateSpansInfo._fields_}

    def link_segments(self):
        """segments the last deflate batch call built its hash chains in; 0 = one workgroup per stream"""
        return int(self.lib.md_i_link_segments(self.ctx))

    # ------------------------------------------------------------------ De.Def.Ns
    def def_ns_many(self, bufs, level=4, fmt=FORMAT_DEFLATE, caps=None):
        """list of bytes -> list of (status, compressed bytes, adler32 of input) through md_def_ns_batch_device"""
        import numpy as np

        torch = self.torch
        n = len(bufs)
        if n == 0:
            return []
        in_len = np.array([len(s) for s in bufs], dtype=np.int64)
        in_off = np.zeros(n, dtype=np.int64)
        np.cumsum(((in_len + 15) // 16 * 16)[:-1], out=in_off[1:])
        if caps is None:
            caps = [int(self.lib.md_zl_def_ns_compress_bound(len(s))) for s in bufs]
        cap = np.array(caps, dtype=np.int64)
        out_off = np.zeros(n, dtype=np.int64)
        np.cumsum(((cap + 255) // 256 * 256)[:-1], out=out_off[1:])
        blob = np.zeros(int(in_off[-1] + in_len[-1]) + 16, dtype=np.uint8)
        for s, o in zip(bufs, in_off):
            blob[o:o + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8)
        dev = self.device
        d_in = torch.from_numpy(blob).to(dev)
        d_out = torch.zeros(int(out_off[-1] + cap[-1]) + 16, dtype=torch.uint8, device=dev)
        t = lambda a: torch.from_numpy(a).to(dev)
        out_len = torch.empty(n, dtype=torch.int64, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        checksum = torch.empty(n, dtype=torch.int32, device=dev)
        d_ioff, d_ilen, d_ooff, d_cap = t(in_off), t(in_len), t(out_off), t(cap)
        self._check(self.lib.md_def_ns_batch_device(self.ctx, fmt, int(level), max(1, int(in_len.sum())), n, _ptr(d_in), _ptr(d_ioff),
                                                    _ptr(d_ilen), _ptr(d_out), _ptr(d_ooff), _ptr(d_cap), _ptr(out_len),
                                                    _ptr(status), _ptr(checksum)))
        torch.cuda.synchronize(dev)
        out = d_out.cpu().numpy()
        out_len, status = out_len.cpu().numpy(), status.cpu().numpy()
        checksum = checksum.cpu().numpy().view(np.uint32)
        return [(int(status[i]), out[out_off[i]:out_off[i] + out_len[i]].tobytes(), int(checksum[i])) for i in range(n)]


_default = {}


def default_engine(device=0):
    if device not in _default:
        _default[device] = Engine(device)
    return _default[device]
