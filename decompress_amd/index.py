"""The index of ONE long DEFLATE / ZLIB / GZip stream (md_inflate_index_*, include/mdeflate.h): access points at block
starts, so that any byte range of the inflated output is read without decoding what lies in front of it.

    idx = Index.build(src, FORMAT_ZLIB, span=1 << 20)      # one decode of the whole stream
    blob = idx.dumps()                                     # keep it beside the file
    idx = Index.loads(blob)                                # no device needed
    idx.read(src, off, n)                                  # bytes, or ("Error", message)
    idx.read_many(src, [(off, n), ...])                    # [(status, bytes)], ONE batch
"""
import ctypes

import numpy as _np

from . import _lib
from . import engine as _engine


class Index:
    def __init__(self, handle, device=0):
        self._h = handle
        self._free = _lib.load().md_inflate_index_free  # (kept: the module may be gone when the last index goes)
        self.device = device

    def __del__(self):
        if getattr(self, "_h", None):
            self._free(self._h)
            self._h = None

    @staticmethod
    def build(src, fmt, span=1 << 20, want_output=False, dst_len=None, device=0):
        """md_inflate_index_build -> Index, or (Index, bytes) with want_output.  dst_len is the room for the output when the
        caller knows a bound of the inflated size: build then delivers the output itself, from its one decode.  Without it
        nobody knows the size in front of the decode, so the index is built without output and the output is read through
        it afterwards: every piece is decoded a second time (about twice the cost of the build)."""
        eng = _engine.default_engine(device)
        src = bytes(src)
        h, info = ctypes.c_void_p(), _lib.InflateIndexInfo()
        dst = ctypes.create_string_buffer(max(1, dst_len)) if want_output and dst_len is not None else None
        st = eng.lib.md_inflate_index_build(eng.ctx, int(fmt), src, len(src), int(span), dst, dst_len if dst is not None else 0,
                                            ctypes.byref(h), ctypes.byref(info))
        if st < 0:
            eng._check(st)
        if st != 0:
            raise _engine.Error(eng.lib.md_status_string(st).decode())
        idx = Index(h.value, device)
        if not want_output:
            return idx
        if dst is not None:
            return idx, dst.raw[:info.size]
        return idx, idx.read(src, 0, info.size)

    @property
    def info(self):
        f = _lib.InflateIndexInfo()
        assert _lib.load().md_inflate_index_get(self._h, ctypes.byref(f)) == 0
        return {k: int(getattr(f, k)) for k, _ in f._fields_}

    @property
    def points(self):
        n = self.info["points"]
        bit, out = _np.zeros(n, dtype=_np.uint64), _np.zeros(n, dtype=_np.uint64)
        assert _lib.load().md_inflate_index_points(self._h, bit.ctypes.data, out.ctypes.data, n) == 0
        return [(int(b), int(o)) for b, o in zip(bit, out)]

    def dumps(self):
        lib = _lib.load()
        n = lib.md_inflate_index_save_size(self._h)
        buf, got = ctypes.create_string_buffer(n), ctypes.c_size_t()
        assert lib.md_inflate_index_save(self._h, buf, n, ctypes.byref(got)) == 0 and got.value == n
        return buf.raw

    @staticmethod
    def loads(blob, device=0):
        blob = bytes(blob)
        h = ctypes.c_void_p()
        st = _lib.load().md_inflate_index_load(blob, len(blob), ctypes.byref(h))
        if st != 0:
            raise _engine.Error(_lib.load().md_status_string(st).decode())
        return Index(h.value, device)

    def read_many(self, src, ranges):
        """md_inflate_index_read: [(off, n), ...] -> [(status, bytes)]; the bytes of a range whose status is not 0 are b\"\"."""
        eng = _engine.default_engine(self.device)
        src = bytes(src)
        n = len(ranges)
        if any(int(o) < 0 or int(m) < 0 or int(o) >> 64 or int(m) >> 64 for o, m in ranges):
            raise _engine.Error("Invalid argument: a range's offset and length are 0 .. 2^64 - 1")
        off = _np.array([int(r[0]) for r in ranges], dtype=_np.uint64)
        ln = _np.array([int(r[1]) for r in ranges], dtype=_np.uint64)
        dst_off = _np.zeros(n, dtype=_np.uint64)
        if n > 1:
            _np.cumsum(ln[:-1], out=dst_off[1:])
        size = self.info["size"]
        inside = all(int(o) + int(m) <= size for o, m in ranges)  # (a range behind the end: the call refuses it, no room needed)
        dst = _np.zeros(max(1, sum(int(m) for _, m in ranges)) if inside else 1, dtype=_np.uint8)
        status = _np.zeros(max(1, n), dtype=_np.int32)
        eng._check(eng.lib.md_inflate_index_read(eng.ctx, self._h, src, len(src), n, off.ctypes.data, ln.ctypes.data, dst.ctypes.data,
                                                 dst_off.ctypes.data, status.ctypes.data))
        return [(int(status[i]), dst[int(dst_off[i]):int(dst_off[i] + ln[i])].tobytes() if status[i] == 0 else b"") for i in range(n)]

    def read(self, src, off, n):
        st, data = self.read_many(src, [(off, n)])[0]
        return data if st == 0 else ("Error", _lib.load().md_status_string(st).decode())

    def last_stats(self):
        """md_inflate_index_last of this index's device: the counts of the last read there"""
        eng = _engine.default_engine(self.device)
        s = _lib.InflateIndexStats()
        eng._check(eng.lib.md_inflate_index_last(eng.ctx, ctypes.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in s._fields_}
