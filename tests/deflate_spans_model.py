"""The stream md_deflate_spans_* must write, restated in Python from the definition in DESIGN.md 4h / mdeflate.h: the text
cut into spans, every span's raw body from the oracle (oracle_lib.deflate_raw: the reference's bytes for that text and
those parameters), the bodies joined - or a span stored where the joined form is strictly longer.  The model knows nothing
of slots or kernels."""
import functools
import random
import struct
import zlib

from decompress_amd import workloads

from . import oracle_lib
from .deflate_tokens import DX, LX, mk

DEFLATE, ZLIB, GZIP = 0, 1, 2
ZL, HIGHER, CLI = 0, 1, 2
QUEUE_FULL = 13
_FIXED = (mk([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), mk([5] * 30))
_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def closing_block(raw):
    """(h, e, btype) of a raw DEFLATE stream's closing block: h = the bit offset of its header (the BFINAL bit), e = the bit
    offset behind its last bit - behind the end-of-block code, or the byte-aligned end of a stored block."""
    pos = 0

    def bits(n):
        nonlocal pos
        v = 0
        for i in range(n):
            v |= ((raw[pos >> 3] >> (pos & 7)) & 1) << i
            pos += 1
        return v

    def sym(d):
        nonlocal pos
        c = l = 0
        while True:
            c = (c << 1) | ((raw[pos >> 3] >> (pos & 7)) & 1)
            pos += 1
            l += 1
            if (l, c) in d:
                return d[(l, c)]

    while True:
        h = pos
        last, t = bits(1), bits(2)
        assert t != 3
        if t == 0:
            pos = (pos + 7) & ~7
            n, nn = bits(16), bits(16)
            assert n ^ nn == 0xffff
            pos += 8 * n
        else:
            if t == 1:
                lt, dt = _FIXED
            else:
                hl, hd, hc = bits(5) + 257, bits(5) + 1, bits(4) + 4
                cl = [0] * 19
                for i in range(hc):
                    cl[_ORDER[i]] = bits(3)
                ct, ls = mk(cl), []
                while len(ls) < hl + hd:
                    s = sym(ct)
                    if s < 16:
                        ls.append(s)
                    elif s == 16:
                        ls += [ls[-1]] * (3 + bits(2))
                    elif s == 17:
                        ls += [0] * (3 + bits(3))
                    else:
                        ls += [0] * (11 + bits(7))
                lt, dt = mk(ls[:hl]), mk(ls[hl:])
            while True:
                s = sym(lt)
                if s == 256:
                    break
                if s > 256:
                    bits(LX[s - 257])
                    bits(DX[sym(dt)])
        if last:
            assert (pos + 7) // 8 == len(raw), "the stream ends with its closing block"
            return h, pos, t


def stored_form(text, final):
    """the bytes as stored blocks of at most 65 535 bytes, all but the last full (no bytes: one empty block); BFINAL on the
    last block if `final`"""
    out = bytearray()
    n = max(1, (len(text) + 65534) // 65535)
    for k in range(n):
        b = text[k * 65535:(k + 1) * 65535]
        out += struct.pack("<BHH", int(final and k == n - 1), len(b), len(b) ^ 0xffff) + b
    return bytes(out)


def joined_form(raw, h, e):
    """the first e bits of raw with bit h cleared, 0 00, zero bits up to the byte, 00 00 FF FF"""
    b = bytearray(raw[:(e + 7) // 8])
    if e & 7:
        b[-1] &= (1 << (e & 7)) - 1
    b[h >> 3] &= ~(1 << (h & 7)) & 0xff
    if (e + 3 + 7) // 8 > len(b):
        b.append(0)
    return bytes(b) + b"\x00\x00\xff\xff"


def spans_of(data, span):
    return [data[i:i + span] for i in range(0, len(data), span)] or [b""]


@functools.lru_cache(maxsize=None)
def body(data, span, level=6, queue=4096, driver=ZL, dynamic=True, matcher=0):
    """-> (the body, [per span: ('J' | 'S', e mod 8 or None, marker bytes, closing block's type or None)]), or None when a
    span's encoder would raise Queue.Full"""
    orc = oracle_lib.load()
    parts, forms = [], []
    texts = spans_of(data, span)
    for i, t in enumerate(texts):
        final = i == len(texts) - 1
        raw, _ = orc.deflate_raw(t, level, queue, driver, dynamic, matcher)
        if raw is None:
            return None
        s = stored_form(t, final)
        if len(raw) + (0 if final else 4) > len(s):  # (whatever e is: J is no shorter than that)
            parts.append(s)
            forms.append(("S", None, 0, None))
            continue
        h, e, bt = closing_block(raw)
        j = raw if final else joined_form(raw, h, e)
        if len(j) > len(s):
            parts.append(s)
            forms.append(("S", e & 7, 0, bt))
        else:
            parts.append(j)
            forms.append(("J", e & 7, len(j) - len(raw), bt))
    return b"".join(parts), forms


def gz_header(level, header):
    """Gz.Def's header bytes for the fields (the oracle's, cut off its stream of the empty text)"""
    orc = oracle_lib.load()
    h = dict(mtime=0, os=3, hcrc=False, ascii=False, filename=None, comment=None)
    h.update(header or {})
    whole = orc.gz_deflate(b"", level=level, mtime=h["mtime"], os=h["os"], hcrc=bool(h["hcrc"]), ascii=bool(h["ascii"]), name=h["filename"],
                           comment=h["comment"])
    empty, _ = orc.deflate_raw(b"", level, 4096, ZL, True, 0)
    return whole[:len(whole) - 8 - len(empty)]


def zl_header(level):
    """Zl.Def's two bytes: CM 8, CINFO 7, FLEVEL by the level, FCHECK"""
    flevel = 0 if level == 0 else 1 if level <= 5 else 2 if level == 6 else 3
    h = (0x78 << 8) | (flevel << 6)
    return struct.pack(">H", h + 31 - h % 31)


def expected(data, span, fmt, header=None, **params):
    """the whole stream, or None for Queue.Full.  FORMAT_GZIP: Gz.Def's body - the Zl driver with dynamic blocks."""
    if fmt == GZIP:
        params = dict(params, driver=ZL, dynamic=True)
    b = body(bytes(data), span, **params)
    if b is None:
        return None
    if fmt == ZLIB:
        return zl_header(params.get("level", 6)) + b[0] + struct.pack(">I", zlib.adler32(data))
    if fmt == GZIP:
        return gz_header(params.get("level", 6), header) + b[0] + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)
    return b[0]


def forms(data, span, **params):
    b = body(bytes(data), span, **params)
    return None if b is None else b[1]


# ---- the cases both test files run: (name, text, span, encoder parameters) ----
@functools.lru_cache(maxsize=None)
def _text(seed, n):
    return workloads.text(seed, n)


@functools.lru_cache(maxsize=None)
def _rand(seed, n):
    return random.Random(seed).randbytes(n)


def cases():
    out = []
    for span in (1, 2, 3, 7, 64):
        for n in sorted({0, 1, span - 1, span, span + 1, 3 * span + 1}):
            out.append(("small-%d-%d" % (span, n), _text(7, 256)[:n], span, {}))
    # level 0: stored blocks; the last span keeps the encoder's (one block: as long as the stored form)
    out.append(("level0-64", _text(7, 256)[:193], 64, dict(level=0)))
    # the CLI driver pushes its end-of-block command onto a queue that 15 literals have filled: Queue.Full in the full spans
    out.append(("queue-full", _rand(5, 40), 15, dict(driver=CLI, queue=16)))
    # several blocks a span (queue 256), the closing one not the first
    t40 = _text(11, 40 << 10)
    grid = [dict(level=lv, dynamic=bool(dy)) for lv in (0, 1, 4, 6, 9) for dy in (0, 1)]
    grid += [dict(level=6, driver=drv, matcher=m) for drv in (HIGHER, CLI) for m in (0, 1)]
    grid += [dict(level=lv, dynamic=bool(dy), matcher=1) for lv in (1, 6, 9) for dy in (0, 1)]
    for g in grid:
        out.append(("text40k-" + "-".join("%s%d" % (k[:2], int(v)) for k, v in sorted(g.items())), t40, 4 << 10, dict(g, queue=256)))
    # spans that do not compress: the stored form, split at 65 535
    for span in (65535, 65536, 131071):
        out.append(("random-%d" % span, _rand(span, span + 70001), span, {}))
    # compressible and random spans as neighbours, both ways round
    alt = b"".join(_text(20 + i, 4096) if i in (0, 3, 4, 6) else _rand(20 + i, 4096) for i in range(8))
    out.append(("alternating", alt, 4096, {}))
    # span lengths around NMAX of Adler-32 and its modulus
    for span in (5551, 5552, 5553, 65521):
        out.append(("ff-%d" % span, b"\xff" * (3 * span + 1), span, {}))
    return out


GZ_HEADER = dict(mtime=0x12345678, os=3, hcrc=True, ascii=False, filename=b"spans.txt", comment=b"joined")
