"""The stream md_deflate_spans_* must write with priming on (md_set_option "deflate_span_prime"), restated from the definition
in DESIGN.md 4h / mdeflate.h: span i is text [s_i, e_i) with a prefix of w_i = min(s_i, 32 768) bytes, and its body is what
the reference's matcher and encoder write for X_i = text[s_i - w_i, e_i) when the matcher has first walked [0, w_i) - it
inserts every position, never looks for a match and emits nothing.  That body comes from tests/primed_oracle.c: the
oracle's own lz_t, fill and insert steps and encoder, with the walk and the drivers' loop added.  Everything behind the
body - the joined and the stored form, the strict-length rule, headers, trailers - is deflate_spans_model's.  The model
knows nothing of slots or kernels."""
import atexit
import ctypes
import functools
import os
import shutil
import struct
import subprocess
import tempfile
import zlib

from . import deflate_spans_model as U
from . import lz77_cases
from .deflate_spans_model import CLI, DEFLATE, GZ_HEADER, GZIP, HIGHER, QUEUE_FULL, ZL, ZLIB  # noqa: F401  (for the tests)
from .deflate_tokens import tokens

HERE = os.path.dirname(os.path.abspath(__file__))
PRIME = 32768
MAX_DIST = 32768 - 262
_LIB = None


def _lib():
    """tests/primed_oracle.c, compiled into a temporary directory when it is first used"""
    global _LIB
    if _LIB is None:
        tmp = tempfile.mkdtemp(prefix="primed_oracle_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        so = os.path.join(tmp, "libprimed_oracle.so")
        subprocess.check_call([os.environ.get("CC", "cc"), "-O2", "-std=c99", "-fPIC", "-shared", "-Wl,-Bsymbolic", "-o", so,
                               os.path.join(HERE, "primed_oracle.c")])
        lib = ctypes.CDLL(so)
        sz, ci = ctypes.c_size_t, ctypes.c_int
        lib.prm_deflate_raw.restype = ctypes.c_void_p
        lib.prm_deflate_raw.argtypes = [ctypes.c_char_p, sz, sz, ci, ci, ci, ci, ci, ctypes.POINTER(sz)]
        lib.prm_free.argtypes = [ctypes.c_void_p]
        _LIB = lib
    return _LIB


def primed_raw(x, first, level=6, queue=4096, driver=ZL, dynamic=True, matcher=0):
    """the raw body of x[first:] from a matcher that has walked x[:first]; None: Queue.Full"""
    lib, n = _lib(), ctypes.c_size_t()
    p = lib.prm_deflate_raw(bytes(x), len(x), first, level, queue, driver, int(bool(dynamic)), matcher, ctypes.byref(n))
    if not p:
        return None
    try:
        return ctypes.string_at(p, n.value)
    finally:
        lib.prm_free(p)


def prefixes(n, span):
    """[(s_i, e_i, w_i)] of a text of n bytes"""
    return [(s, min(s + span, n), min(s, PRIME)) for s in range(0, n, span)] or [(0, 0, 0)]


@functools.lru_cache(maxsize=None)
def raws(data, span, level=6, queue=4096, driver=ZL, dynamic=True, matcher=0):
    """the primed body B_i of every span (None where the encoder would raise Queue.Full)"""
    return [primed_raw(data[s - w:e], w, level, queue, driver, dynamic, matcher) for s, e, w in prefixes(len(data), span)]


@functools.lru_cache(maxsize=None)
def body(data, span, level=6, queue=4096, driver=ZL, dynamic=True, matcher=0):
    """as deflate_spans_model.body, over the primed bodies"""
    parts, forms = [], []
    rs = raws(data, span, level, queue, driver, dynamic, matcher)
    for i, ((s, e, w), raw) in enumerate(zip(prefixes(len(data), span), rs)):
        final, t = i == len(rs) - 1, data[s:e]
        if raw is None:
            return None
        st = U.stored_form(t, final)
        if len(raw) + (0 if final else 4) > len(st):
            parts.append(st)
            forms.append(("S", None, 0, None))
            continue
        h, eb, bt = U.closing_block(raw)
        j = raw if final else U.joined_form(raw, h, eb)
        if len(j) > len(st):
            parts.append(st)
            forms.append(("S", eb & 7, 0, bt))
        else:
            parts.append(j)
            forms.append(("J", eb & 7, len(j) - len(raw), bt))
    return b"".join(parts), forms


def expected(data, span, fmt, header=None, **params):
    """the whole primed stream, or None for Queue.Full.  FORMAT_GZIP: Gz.Def's body - the Zl driver with dynamic blocks."""
    data = bytes(data)
    if fmt == GZIP:
        params = dict(params, driver=ZL, dynamic=True)
    b = body(data, span, **params)
    if b is None:
        return None
    if fmt == ZLIB:
        return U.zl_header(params.get("level", 6)) + b[0] + struct.pack(">I", zlib.adler32(data))
    if fmt == GZIP:
        return U.gz_header(params.get("level", 6), header) + b[0] + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)
    return b[0]


def forms(data, span, **params):
    b = body(bytes(data), span, **params)
    return None if b is None else b[1]


def span_tokens(data, span, i, **params):
    """the literals and matches of span i's primed body: [(offset in the span, 'L', byte) | (offset, 'M', length, distance)]"""
    return [t for t in tokens(raws(bytes(data), span, **params)[i]) if t[0] != "B"]


# ---- the cases both test files run: (name, text, span, encoder parameters) ----
def _prefix_only(same):
    """span 1 begins with 40 bytes that stand 1 900 back: its first token is a match whose source lies wholly in the prefix.
    De.Lz77 begins with match_length 0, so the first longest_match of a stream compares the byte in front of the position
    too (scan_end at best_len - 1): the match is found at the span's first byte where the bytes in front of source and
    span agree (`same`), and one position later where they differ.  (Lz begins with MIN_MATCH - 1 and finds it either way.)"""
    r = U._rand(70, 2000)
    return r[:99] + bytes([r[1999] ^ (0 if same else 1)]) + r[100:] + r[100:140] + U._rand(71, 500)


def _straddle():
    """a two-byte period cut mid-run: span 1's first match starts in the prefix and runs into the span (distance < length)"""
    return U._rand(72, 1000) + b"ab" * 500 + U._rand(73, 300)


@functools.lru_cache(maxsize=None)
def _max_dist():
    """in span 1 (start 40 000, a full prefix): 12 bytes whose only earlier occurrence is 32 506 back (-> t1), and 12 whose
    only one is 32 507 back (-> t2).  -> (text, t1, t2)"""
    fence = lz77_cases._Fence()
    buf = lz77_cases.background(42000)
    t1, _ = lz77_cases.plant_clean(buf, MAX_DIST, 7600, 12, fence)
    t2, _ = lz77_cases.plant_clean(buf, MAX_DIST + 1, 7700, 12, fence)
    assert 40000 < t1 < t2 < 40000 + 262 - 12
    return bytes(buf), t1, t2


@functools.lru_cache(maxsize=None)
def _nil():
    """three bytes of span 1 (start 1 024) whose only earlier occurrence is text offset 0: NIL.  -> (text, target)"""
    buf = lz77_cases.background(2048)
    t = 1024 + 50
    buf[0:3] = buf[t:t + 3]
    buf[3] = 7  # (not the target's fourth byte: from outside the alphabet)
    return bytes(buf), t


def cases():
    out = []
    out.append(("growth", U._text(80, (48 << 10) + 1), 4096, {}))
    out.append(("odd-5000", U._text(81, 23001), 5000, {}))
    out.append(("prefix-only", _prefix_only(True), 2000, {}))
    out.append(("prefix-only-byte-in-front", _prefix_only(False), 2000, {}))
    out.append(("prefix-only-byte-in-front-lz", _prefix_only(False), 2000, dict(matcher=1)))
    out.append(("straddle", _straddle(), 1301, {}))
    out.append(("max-dist", _max_dist()[0], 40000, {}))
    out.append(("nil", _nil()[0], 1024, {}))
    for k in (1, 2, 3):
        out.append(("short-last-%d" % k, U._text(82, 33000 + k), 33000, {}))
    for ln in (32506, 32507, 32508):
        out.append(("slide-%d" % ln, U._text(83, 3 * ln), ln, {}))
    out.append(("slide-65536", U._text(84, 2 * 65536), 65536, {}))
    # the end-of-stream families of lz77_cases (the last 340 positions, H7) as the text of a span behind a full prefix
    pre = bytes(lz77_cases.background(PRIME, start=60000))
    for name, data, _ in lz77_cases.family_f():
        for m in (0, 1) if "tail_copy" in name or "h7" in name else (0,):  # (Lz's matcher: the families about the very end)
            out.append(("%s-ma%d" % (name, m), pre + data, PRIME, dict(matcher=m)))
    for name, data, span, params in U.cases():
        if name.startswith("text40k-") or name in ("queue-full", "alternating") or name.startswith("ff-"):
            out.append((name, data, span, params))
    out.append(("repeat", U._rand(85, 4096) * 8, 4096, {}))
    return out
