"""Mirror of the reference's `Lzo` module (decompress.lzo, lib/lzo.ml): `Lzo.compress` /
`Lzo.uncompress` / `Lzo.uncompress_with_buffer`, run on the GPU through the C ABI (csrc/lzo_kernels.hip)."""
import ctypes

from . import engine as _engine


def max_compressed_length(n):
    """room Lzo.compress never exceeds (liblzo's bound; the reference's tests use (len + 1) * 2)"""
    return n + n // 16 + 64 + 3


def compress(src, device=0):
    """`Lzo.compress in_data out_data wrkmem` (lib/lzo.ml:656-660) -> bytes"""
    st, out = _engine.default_engine(device).lzo_many(True, [src], [max_compressed_length(len(src))])[0]
    if st != 0:
        raise _engine.Error(_engine.STATUS_NAMES[st])
    return out


def uncompress(src, dst_len, device=0):
    """`Lzo.uncompress input output` (lib/lzo.ml:395-403) -> ("Ok", bytes) | ("Error", message)"""
    st, out = _engine.default_engine(device).lzo_many(False, [src], [dst_len])[0]
    return ("Ok", out) if st == 0 else ("Error", _engine.STATUS_NAMES[st])


def uncompressed_size(src, device=0):
    """The uncompressed size of an LZO1X stream without decoding it (md_lzo_sizes_batch_host): ("Ok", size) |
    ("Error", message), the errors being `Lzo.uncompress_with_buffer`'s"""
    st, size = _engine.default_engine(device).lzo_sizes_host([src])[0]
    return ("Ok", size) if st == 0 else ("Error", _engine.STATUS_NAMES[st])


def uncompress_with_buffer(src, chunk=0x1000, device=0):
    """`Lzo.uncompress_with_buffer ?chunk input` (lib/lzo.ml:405-414) -> ("Ok", bytes) | ("Error", message), through
    md_lzo_uncompress_with_buffer: the room comes from the stream.  `chunk` is the initial size of the reference's buffer
    and has no effect here."""
    eng = _engine.default_engine(device)
    src = bytes(src)
    dst, n = ctypes.c_void_p(), ctypes.c_size_t()
    st = eng.lib.md_lzo_uncompress_with_buffer(eng.ctx, src, len(src), ctypes.byref(dst), ctypes.byref(n))
    if st < 0:
        eng._check(st)
    if st != 0:
        return "Error", _engine.STATUS_NAMES[st]
    try:
        return "Ok", ctypes.string_at(dst.value, n.value)
    finally:
        eng.lib.md_host_free(eng.ctx, dst)
