"""Mirror of the reference's `Gz` module surface for the hot path (lib/gz.ml: `Gz.Inf`,
`Gz.Def`, `Gz.Higher`), executed on the GPU through the C ABI: header / trailer handling in
`csrc/gz_kernels.hip`, the DEFLATE body in the batched inflate / deflate kernels."""
import ctypes

import numpy as _np

from . import engine as _engine
from ._lib import BgzfIndexInfo, BgzfReadStats, GzMembersInfo, GzMembersStats, GzMeta
from ._lib import load as _load

# Gz.os, lib/gz.ml:158-246 (RFC1952 numbering)
OS = {"FAT": 0, "Amiga": 1, "VMS": 2, "Unix": 3, "VM": 4, "Atari": 5, "HPFS": 6, "Macintosh": 7, "Z": 8, "CPM": 9,
      "TOPS20": 10, "NTFS": 11, "QDOS": 12, "Acorn": 13, "Unknown": 255}


def extra(payload, key):
    """Gz.Inf.extra ~key (lib/gz.ml:617-633): 2-character subfield id, uint16_be length, value."""
    if len(key) != 2:
        raise ValueError("Subfield ID must be 2 characters.")
    idx = 0
    while payload is not None and idx + 4 <= len(payload):
        k, ln = payload[idx:idx + 2], int.from_bytes(payload[idx + 2:idx + 4], "big")
        if idx + 4 + ln > len(payload):
            break
        if k == key:
            return payload[idx + 4:idx + 4 + ln]
        idx += 4 + ln
    return None


class Higher:
    """Gz.Higher (lib/gz.ml:921-982)."""

    @staticmethod
    def compress(src, level=0, filename=None, comment=None, mtime=0, os="Unix", ascii=False, hcrc=False,
                 queue=4096, device=0):
        """`Gz.Higher.compress ?level ?filename ?comment ~w ~q ~refill ~flush time cfg i o`
        (`?level` defaults to 0 upstream, lib/gz.ml:928; `cfg` = ascii / hcrc / os / mtime)."""
        eng = _engine.default_engine(device)
        hdr = dict(mtime=int(mtime) & 0xffffffff, os=OS[os] if isinstance(os, str) else int(os), hcrc=int(bool(hcrc)),
                   ascii=int(bool(ascii)), filename=filename, comment=comment)
        st, out, _ = eng.deflate_one(src, _engine.FORMAT_GZIP, level=level, queue=queue, header=hdr)
        if st != 0:
            raise _engine.Error(_engine.STATUS_NAMES[st])
        return out

    @staticmethod
    def uncompress(src, dst_len, device=0):
        """`Gz.Higher.uncompress ~refill ~flush i o` -> ("Ok", metadata, bytes) | ("Error", msg)."""
        eng = _engine.default_engine(device)
        src = bytes(src)
        dst = ctypes.create_string_buffer(max(dst_len, 1))
        used, wrote, m = ctypes.c_size_t(), ctypes.c_size_t(), GzMeta()
        st = eng.lib.md_gz_higher_uncompress(eng.ctx, src, len(src), dst, dst_len, ctypes.byref(used),
                                             ctypes.byref(wrote), ctypes.byref(m))
        if st < 0:
            eng._check(st)
        if st != 0:
            return "Error", _engine.STATUS_NAMES[st]
        meta = {
            "filename": src[m.name_off:m.name_off + m.name_len] if m.has_name else None,
            "comment": src[m.comment_off:m.comment_off + m.comment_len] if m.has_comment else None,
            "os": m.os, "mtime": m.mtime,
            "extra": src[m.extra_off:m.extra_off + m.extra_len] if m.has_extra else None,
        }
        return "Ok", meta, dst.raw[:wrote.value]


class Inf:
    @staticmethod
    def inflate_batch(srcs, dst_lens, device=0):
        """n GZip members at once -> [(status, consumed, bytes, crc32)]"""
        return _engine.default_engine(device).inflate_many(srcs, dst_lens, _engine.FORMAT_GZIP)


class Def:
    @staticmethod
    def deflate_batch(bufs, level=4, queue=4096, device=0, **header):
        """n buffers at once -> [(status, gzip bytes, crc32 of the input)]"""
        hdr = dict(mtime=0, os=3, hcrc=0, ascii=0, filename=None, comment=None)
        hdr.update(header)
        hdr["os"] = OS[hdr["os"]] if isinstance(hdr["os"], str) else int(hdr["os"])
        return _engine.default_engine(device).deflate_many(bufs, _engine.FORMAT_GZIP, level=level, queue=queue, header=hdr)


def _raw(src):
    """bytes-like -> (object ctypes passes by address without a copy of bytes, length)"""
    src = src if isinstance(src, bytes) else bytes(src)
    return src, len(src)


class Members:
    """A GZip FILE of many members (RFC 1952 2.2: `cat a.gz b.gz`, bgzip / BGZF), read as libz reads it - not `Gz.Inf`'s
    reading, which `Higher.uncompress` keeps.  A file whose members all carry the BC size field is indexed: its members are
    found on the device and decoded by one inflate launch.  In any other file the device takes every position that looks
    like a member's start, decodes the spans between them as one batch and keeps those that end in a matching trailer
    where the next begins; the host walks the file over them and decodes the rest itself (`last_stats` says how it went)."""

    @staticmethod
    def scan(src, device=0):
        """-> None when the file is not indexed, else a dict: members, size (uncompressed), c_off / u_off (per member:
        its offset in src, the offset of its output) - the .gzi index, without decoding."""
        eng = _engine.default_engine(device)
        src, n = _raw(src)
        info = GzMembersInfo()
        eng._check(eng.lib.md_gz_members_scan(eng.ctx, src, n, ctypes.byref(info), None, None, 0))
        if not info.indexed:
            return None
        c_off, u_off = (ctypes.c_uint64 * info.members)(), (ctypes.c_uint64 * info.members)()
        eng._check(eng.lib.md_gz_members_scan(eng.ctx, src, n, ctypes.byref(info), c_off, u_off, info.members))
        return {"members": info.members, "size": info.written, "c_off": list(c_off), "u_off": list(u_off)}

    @staticmethod
    def uncompress(src, dst_len=None, device=0):
        """-> ("Ok", info, bytes) | ("Error", msg, info, bytes of the members in front of the failing one); info: members,
        consumed, written, indexed.  dst_len None: the size an indexed file states, else room that grows until it fits."""
        eng = _engine.default_engine(device)
        src, n = _raw(src)
        info = GzMembersInfo()
        grow = dst_len is None
        if grow:
            idx = Members.scan(src, device)
            dst_len = idx["size"] if idx else max(4 * n, 1 << 16)
        while True:
            dst = ctypes.create_string_buffer(max(dst_len, 1))
            st = eng.lib.md_gz_members_uncompress(eng.ctx, src, n, dst, dst_len, ctypes.byref(info))
            if st < 0:
                eng._check(st)
            if grow and st == _engine.STATUS_CODES["Unexpected_end_of_output"]:
                dst_len = max(2 * dst_len, info.written, 1 << 16)
                continue
            d = {"members": info.members, "consumed": info.consumed, "written": info.written, "indexed": info.indexed}
            if st != 0:
                # (an indexed file without room: `written` is the room it needs, not what dst holds)
                keep = 0 if st == _engine.STATUS_CODES["Unexpected_end_of_output"] and info.indexed else info.written
                return "Error", _engine.STATUS_NAMES[st], d, dst.raw[:keep]
            return "Ok", d, dst.raw[:info.written]

    @staticmethod
    def last_stats(device=0):
        """md_gz_members_last: which way the last `uncompress` of this device's engine went -> dict: path (0 general, 1
        indexed, 2 speculative), candidates, spans_decoded, members_device, members_host, spans_long, spans_no_room,
        spans_implausible."""
        eng = _engine.default_engine(device)
        s = GzMembersStats()
        eng._check(eng.lib.md_gz_members_last(eng.ctx, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in GzMembersStats._fields_}


class Bgzf:
    @staticmethod
    def compress_bound(n, block=0xff00):
        """room that always suffices for `compress` of n bytes (host arithmetic, no device needed)"""
        return _load().md_bgzf_compress_bound(n, block)

    @staticmethod
    def compress(src, level=4, block=0xff00, dst_len=None, device=0):
        """Blocked gzip as bgzip writes it: members of at most `block` input bytes, each with its BC size field, then the
        empty member that marks the end.  All blocks go through one deflate launch; the bytes depend on (src, level,
        block) alone.  Raises `Error` with the status' name (dst_len too small: "Unexpected_end_of_output")."""
        eng = _engine.default_engine(device)
        src, n = _raw(src)
        if dst_len is None:
            dst_len = eng.lib.md_bgzf_compress_bound(n, block)
        dst = ctypes.create_string_buffer(max(dst_len, 1))
        wrote = ctypes.c_size_t()
        st = eng.lib.md_bgzf_compress(eng.ctx, level, block, src, n, dst, dst_len, ctypes.byref(wrote))
        if st < 0:
            eng._check(st)
        if st != 0:
            raise _engine.Error(_engine.STATUS_NAMES[st])
        return dst.raw[:wrote.value]


class BgzfIndex:
    """Random access to a blocked GZip file (md_bgzf_index_*, md_bgzf_read*): where every member begins in the file and in
    its output, so that any set of byte ranges - or BGZF virtual offsets - is read as one batch, only the members they
    touch copied to the device and decoded, each checked against its CRC-32.  There is no CPU fallback.

        idx = BgzfIndex.build(src)                  # the member scan, nothing decoded
        idx = BgzfIndex.from_gzi(blob, src)         # a .gzi beside the file; no device needed
        idx.read(src, off, n)                       # bytes, or ("Error", name)
        idx.read_many(src, [(off, n), ...])         # [("Ok", bytes) | ("Error", name)], ONE batch
        idx.read_virtual_many(src, [(voff, n)])     # voff = member's offset in src << 16 | offset in its output
    """

    def __init__(self, handle, device=0):
        self._h = handle
        self._free = _load().md_bgzf_index_free  # (kept: the module may be gone when the last index goes)
        self.device = device

    def __del__(self):
        if getattr(self, "_h", None):
            self._free(self._h)
            self._h = None

    @staticmethod
    def build(src, device=0):
        eng = _engine.default_engine(device)
        src, n = _raw(src)
        h = ctypes.c_void_p()
        st = eng.lib.md_bgzf_index_build(eng.ctx, src, n, ctypes.byref(h))
        if st < 0:
            eng._check(st)
        if st != 0:
            raise _engine.Error(_engine.STATUS_NAMES[st])
        return BgzfIndex(h.value, device)

    @staticmethod
    def from_gzi(blob, src, device=0):
        blob, src = bytes(blob), _raw(src)[0]
        h = ctypes.c_void_p()
        st = _load().md_bgzf_index_from_gzi(blob, len(blob), src, len(src), ctypes.byref(h))
        if st != 0:
            raise _engine.Error(_load().md_status_string(st).decode())
        return BgzfIndex(h.value, device)

    def to_gzi(self):
        lib = _load()
        n = lib.md_bgzf_index_gzi_size(self._h)
        buf, got = ctypes.create_string_buffer(n), ctypes.c_size_t()
        assert lib.md_bgzf_index_to_gzi(self._h, buf, n, ctypes.byref(got)) == 0 and got.value == n
        return buf.raw

    def info(self):
        """-> dict: src_len, members, size (of the output)"""
        f = BgzfIndexInfo()
        assert _load().md_bgzf_index_get(self._h, ctypes.byref(f)) == 0
        return {k: int(getattr(f, k)) for k, _ in f._fields_}

    def entries(self):
        """-> the M + 1 pairs (c_off, u_off): every member's start, then the end of the last one"""
        n = self.info()["members"] + 1
        c_off, u_off = (ctypes.c_uint64 * n)(), (ctypes.c_uint64 * n)()
        assert _load().md_bgzf_index_entries(self._h, c_off, u_off, n) == 0
        return list(zip(c_off, u_off))

    def _read(self, fn, src, where, size_known):
        eng = _engine.default_engine(self.device)
        src, slen = _raw(src)
        n = len(where)
        if any(int(o) < 0 or int(m) < 0 or int(o) >> 64 or int(m) >> 64 for o, m in where):
            raise _engine.Error("Invalid argument: a range's offset and length are 0 .. 2^64 - 1")
        off = _np.array([int(r[0]) for r in where], dtype=_np.uint64)
        ln = _np.array([int(r[1]) for r in where], dtype=_np.uint64)
        dst_off = _np.zeros(n, dtype=_np.uint64)
        if n > 1:
            _np.cumsum(ln[:-1], out=dst_off[1:])
        size = self.info()["size"]
        # (a range behind the end: the call refuses it, no room needed)
        inside = all(int(m) <= size and (not size_known or int(o) + int(m) <= size) for o, m in where)
        dst = _np.zeros(max(1, sum(int(m) for _, m in where)) if inside else 1, dtype=_np.uint8)
        status = _np.zeros(max(1, n), dtype=_np.int32)
        eng._check(fn(eng.ctx, self._h, src, slen, n, off.ctypes.data, ln.ctypes.data, dst.ctypes.data, dst_off.ctypes.data,
                      status.ctypes.data))
        return [("Ok", dst[int(dst_off[i]):int(dst_off[i] + ln[i])].tobytes()) if status[i] == 0 else
                ("Error", _engine.STATUS_NAMES[int(status[i])]) for i in range(n)]

    def read_many(self, src, ranges):
        """md_bgzf_read: [(off, n), ...] -> [("Ok", bytes) | ("Error", name)]"""
        return self._read(_engine.default_engine(self.device).lib.md_bgzf_read, src, ranges, True)

    def read_virtual_many(self, src, ranges):
        """md_bgzf_read_virtual: [(voff, n), ...] -> [("Ok", bytes) | ("Error", name)]"""
        return self._read(_engine.default_engine(self.device).lib.md_bgzf_read_virtual, src, ranges, False)

    def read(self, src, off, n):
        st, data = self.read_many(src, [(off, n)])[0]
        return data if st == "Ok" else (st, data)

    def last_stats(self):
        """md_bgzf_read_last of this index's device: members decoded, inflate launches, bytes of src copied in, bytes of
        output slots - of the last read there"""
        eng = _engine.default_engine(self.device)
        s = BgzfReadStats()
        eng._check(eng.lib.md_bgzf_read_last(eng.ctx, ctypes.byref(s)))
        return {k: int(getattr(s, k)) for k, _ in s._fields_}


def inflated_size(src, device=0):
    """The inflated size of a GZip member (md_inflate_sizes_batch_host; ISIZE is checked, the CRC-32 is not):
    ("Ok", (consumed, size)) without decoding, or ("Error", name)."""
    st, used, size = _engine.default_engine(device).inflate_sizes_host(_engine.FORMAT_GZIP, [src])[0]
    if st == 0:
        return "Ok", (used, size)
    return "Error", _engine.STATUS_NAMES[st]


def index(src, span=1 << 20, device=0):
    """The index of a long GZip (its first member) stream (decompress_amd.index.Index.build): any byte range of its output as one batch."""
    from .index import Index
    return Index.build(src, _engine.FORMAT_GZIP, span=span, device=device)


def compress_spans(src, level=6, span=None, filename=None, comment=None, mtime=0, os="Unix", ascii=False, hcrc=False, queue=4096, device=0,
                   prime=None):
    """ONE GZip stream of src written as joined spans on the whole chip (md_deflate_spans_host): the text
    is cut into spans of `span` bytes (None: the option "deflate_span_kib"), the spans are compressed as one batch and
    joined into a stream that every inflater reads to its end.  Not the bytes of `Higher.compress`: a span cannot refer
    back across a joint, so the stream is a little longer - and takes milliseconds where the single stream takes seconds.  prime: every span's matcher starts from the 32 KiB
    of text in front of it, which buys nearly all of that back (None: the option "deflate_span_prime")."""
    eng = _engine.default_engine(device)
    hdr = dict(mtime=int(mtime) & 0xffffffff, os=OS[os] if isinstance(os, str) else int(os), hcrc=int(bool(hcrc)),
               ascii=int(bool(ascii)), filename=filename, comment=comment)
    st, out, _ = eng.deflate_spans(src, _engine.FORMAT_GZIP, span=span, level=level, queue=queue, header=hdr, prime=prime)
    if st != 0:
        raise _engine.Error(_engine.STATUS_NAMES[st])
    return out
