"""Mirror of the reference's `Zl` module surface for the hot path
(lib/zl.ml:382-418 `Zl.Inf.Ns`), executed on the GPU through the C ABI."""
from . import engine as _engine


class Inf:
    class Ns:
        """Zl.Inf.Ns — zlib-framed whole-buffer inflate (lib/zl.ml:400-417)."""

        @staticmethod
        def inflate(src, dst_len, device=0):
            st, used, out, _ = _engine.default_engine(device).inflate_many(
                [src], [dst_len], _engine.FORMAT_ZLIB)[0]
            if st == 0:
                return "Ok", (used, len(out)), out
            return "Error", _engine.STATUS_NAMES[st]

        @staticmethod
        def inflate_batch(srcs, dst_lens, device=0):
            return _engine.default_engine(device).inflate_many(srcs, dst_lens, _engine.FORMAT_ZLIB)


class Def:
    class Ns:
        """Zl.Def.Ns (lib/zl.ml:596-629): De.Def.Ns inside a zlib frame"""

        @staticmethod
        def compress_bound(n, device=0):
            return _engine.default_engine(device).lib.md_zl_def_ns_compress_bound(n)

        @staticmethod
        def deflate(src, level=4, dst_len=None, device=0):
            from . import de
            return de.Def.Ns.deflate(src, level, dst_len, device, _zl=True)


class Higher:
    """Zl.Higher (lib/zl.ml:633-667)."""

    @staticmethod
    def compress(src, level=6, dynamic=True, queue=4096, device=0):
        """`Zl.Higher.compress ?level ?dynamic ~w ~q ~refill ~flush i o`: a zlib stream."""
        st, out, _ = _engine.default_engine(device).deflate_one(
            src, _engine.FORMAT_ZLIB, level=level, queue=queue, driver=_engine.DRIVER_ZL, dynamic=dynamic)
        if st != 0:
            raise _engine.Error(_engine.STATUS_NAMES[st])
        return out

    @staticmethod
    def uncompress(src, dst_len, device=0):
        """`Zl.Higher.uncompress ~allocate ~refill ~flush i o` (lib/zl.ml:650-666): bytes | ("Error", msg)."""
        import ctypes
        eng = _engine.default_engine(device)
        src = bytes(src)
        dst, n = ctypes.create_string_buffer(max(1, dst_len)), ctypes.c_size_t()
        st = eng.lib.md_zl_higher_uncompress(eng.ctx, src, len(src), dst, dst_len, ctypes.byref(n))
        if st < 0:
            eng._check(st)
        return dst.raw[:n.value] if st == 0 else ("Error", eng.lib.md_status_string(st).decode())


def inflated_size(src, device=0):
    """The inflated size of a ZLIB stream (md_inflate_sizes_batch_host; the Adler-32 is not checked):
    ("Ok", (consumed, size)) without decoding, or ("Error", name)."""
    st, used, size = _engine.default_engine(device).inflate_sizes_host(_engine.FORMAT_ZLIB, [src])[0]
    if st == 0:
        return "Ok", (used, size)
    return "Error", _engine.STATUS_NAMES[st]


def index(src, span=1 << 20, device=0):
    """The index of a long ZLIB stream (decompress_amd.index.Index.build): any byte range of its output as one batch."""
    from .index import Index
    return Index.build(src, _engine.FORMAT_ZLIB, span=span, device=device)


def compress_spans(src, level=6, span=None, queue=4096, dynamic=True, matcher=None, device=0, prime=None):
    """ONE ZLIB stream of src written as joined spans on the whole chip (md_deflate_spans_host): the text
    is cut into spans of `span` bytes (None: the option "deflate_span_kib"), the spans are compressed as one batch and
    joined into a stream that every inflater reads to its end.  Not the bytes of `Higher.compress`: a span cannot refer
    back across a joint, so the stream is a little longer - and takes milliseconds where the single stream takes seconds.  prime: every span's matcher starts from the 32 KiB
    of text in front of it, which buys nearly all of that back (None: the option "deflate_span_prime")."""
    eng = _engine.default_engine(device)
    st, out, _ = eng.deflate_spans(src, _engine.FORMAT_ZLIB, span=span, level=level, queue=queue, dynamic=dynamic, matcher=matcher,
                                   prime=prime)
    if st != 0:
        raise _engine.Error(_engine.STATUS_NAMES[st])
    return out
