"""Texts for the checksum tests: Adler-32 and CRC-32 at their arithmetic and join limits, built on the CPU from nothing but
zlib and arithmetic.  tests/test_checksum_cases.py proves on the CPU that every text is what its name says, and restates
the fixed-geometry accumulations of the kernels with exact integers; tests/test_gpu_checksums.py runs the texts through
every place of the library that computes a checksum.

Families:
  top          P + 0xFF * n.  P is 65536 bytes with adler32(P) == 0xfff0fff0: whatever sums in steps of 16, 1024, 4096 or
               65536 bytes starts its next step in state (65520, 65520) on bytes that are all 0xFF.
               `slice_top`: 65536 bytes on which every 256-byte slice of adler_segments_kernel reaches its largest sum.
  seeded       (seed, data) for the entry points that take a running Adler-32.
  zero-a, one-a, zero-b   a % 65521 == 0, a == 1, b % 65521 == 0, at lengths 257, 65521, 65536 and 2 x 65521 - and
               repeated, so that every span of deflate_spans(span=that length) has such a checksum.
  one-hot      zeros with one 0xFF: a wrong position weight anywhere changes b.
  lengths      every prefix of one random text of 8400 bytes at four base offsets of one blob; long random and zero texts.
  forged-crc   texts whose CRC-32 is 0x00000000 / 0xffffffff.
  bad-trailer  frames whose trailer is congruent to the right value but not equal to it, or one bit off."""
import functools
import random
import struct
import zlib

MOD = 65521
FF_RUNS = (1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 5552, 5553, 65535, 65536, 65537, 200000)
SEEDS = (1, 0xfff0fff0, 0x0000fff0, 0xfff00001, 0x00000000)
UNIT_LENGTHS = (257, 65521, 65536, 2 * 65521)
ONE_HOT_LENGTHS = (4096 + 17, 65536 + 257)
LENGTHS_N = 8400
BASES = (0, 1, 15, 63)
LONG_LENGTHS = (65535, 65536, 65537, 262143, 262144 + 4097, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (2 << 20) + 17)


def adler_pair(data, seed=1):
    v = zlib.adler32(data, seed)
    return v & 0xffff, v >> 16


def rand(n, seed):
    return random.Random(0xc5c5 + seed).randbytes(n)


# ---- top --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def top_prefix():
    """65536 bytes: z zeros, 256 x 0xFF, one byte v, zeros.  a = 1 + 256 * 255 + v == 65520 gives v; b is linear in z
    (a byte d at position i counts (n - i) d), so the z with b == 65520 is found by trying each"""
    n = 65536
    v = 65520 - 1 - 256 * 255
    assert 0 <= v <= 255
    for z in range(n - 257):
        b = n + 255 * (256 * (n - z) - 255 * 256 // 2) + v * (n - (z + 256))  # (sum of n - i over the 256 positions from z)
        if b % MOD == 65520:
            p = bytes(z) + b"\xff" * 256 + bytes([v]) + bytes(n - z - 257)
            assert len(p) == n and zlib.adler32(p) == 0xfff0fff0
            return p
    raise AssertionError("no such prefix")


@functools.lru_cache(None)
def top(n):
    return top_prefix() + b"\xff" * n


def top_texts():
    return [("top-%d" % n, top(n)) for n in FF_RUNS]


@functools.lru_cache(None)
def slice_head():
    """16 bytes d_0 .. d_15 with sum (256 - k) d_k == 65520 (mod 65521): what adler_segments_kernel carries out of the first
    step of a 256-byte slice is then the largest value it can carry.  Found by search: 15 bytes of 0xFF, then the last
    byte and one earlier byte varied."""
    for j in range(15):
        for x in range(256):
            for y in range(256):
                d = [255] * 16
                d[j], d[15] = x, y
                if sum((256 - k) * d[k] for k in range(16)) % MOD == 65520:
                    return bytes(d)
    raise AssertionError("no such head")


@functools.lru_cache(None)
def slice_top():
    return (slice_head() + b"\xff" * 240) * 256


# ---- seeded -----------------------------------------------------------------------------------------------------------------
def seeded():
    """[(name, seed, data)]; the reference is zlib.adler32(data, seed)"""
    out = []
    for s in SEEDS:
        for n in FF_RUNS:
            out.append(("seed-%08x-ff-%d" % (s, n), s, b"\xff" * n))
        out.append(("seed-%08x-random-70000" % s, s, rand(70000, 1)))
    return out


# ---- zero-a, one-a, zero-b --------------------------------------------------------------------------------------------------
ZERO_A_CORE = b"\xff" * 256 + b"\xf0"  # 1 + 256 * 255 + 240 == 65521


@functools.lru_cache(None)
def zero_a(n):
    """n - 257 zeros, then the 257 bytes that bring a to 65521"""
    assert n >= 257
    return bytes(n - 257) + ZERO_A_CORE


@functools.lru_cache(None)
def one_a(n):
    return bytes(n)


@functools.lru_cache(None)
def zero_b(n):
    """random bytes with one byte near the end replaced so that b % 65521 == 0: replacing byte p by x changes b by
    (x - old) (n - p); the search goes back from the end until some x in 0 .. 255 fits (a short text may have no such
    byte: then the next random text is tried)"""
    for attempt in range(64):
        base = bytearray(rand(n, 2 + n + 1000003 * attempt))
        b0 = adler_pair(bytes(base))[1]
        for p in range(n - 1, max(-1, n - 2001), -1):
            w = (n - p) % MOD
            if w == 0:
                continue
            for x in range(256):
                if (b0 + (x - base[p]) * w) % MOD == 0:
                    base[p] = x
                    return bytes(base)
    raise AssertionError("no such text")


KINDS = {"zero-a": zero_a, "one-a": one_a, "zero-b": zero_b}


def unit_texts():
    return [("%s-%d" % (k, n), f(n)) for k, f in KINDS.items() for n in UNIT_LENGTHS]


def units(kind, n, count):
    """`count` units of length n back to back: deflate_spans(span=n) gives every span the unit's checksum"""
    return KINDS[kind](n) * count


# ---- one-hot ----------------------------------------------------------------------------------------------------------------
def one_hot_positions(n):
    """the first and last byte of the text, of every 16-byte chunk next to 0, 1024 and 4096, and of the last partial chunk"""
    ps = {0, n - 1}
    for edge in (0, 1024, 4096):
        for c in (edge - 16, edge, edge + 16):
            ps.update((c, c + 15))
    last = (n - 1) // 16 * 16
    ps.update((last - 16, last - 1, last, n - 1))
    return sorted(p for p in ps if 0 <= p < n)


def one_hot_text(n, p):
    return bytes(p) + b"\xff" + bytes(n - p - 1)


def one_hot():
    return [("one-hot-%d-at-%d" % (n, p), one_hot_text(n, p)) for n in ONE_HOT_LENGTHS for p in one_hot_positions(n)]


# ---- lengths ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def lengths_text(kind="random"):
    """8400 random bytes; kind "four": drawn from 0x00, 0x01, 0xfe and 0xff only, for the encoder that refuses a text
    which no Huffman code makes shorter (De.Def.Ns, as its model does)"""
    if kind == "four":
        return bytes(b"\x00\x01\xfe\xff"[v & 3] for v in rand(LENGTHS_N, 8))
    return rand(LENGTHS_N, 3)


@functools.lru_cache(None)
def lengths_blob(kind="random"):
    """-> (blob, starts): the text once per base offset, its copy for base q starting at a byte that is q mod 64"""
    blob, starts = bytearray(), []
    for q in BASES:
        blob += bytes((q - len(blob)) % 64)
        starts.append(len(blob))
        blob += lengths_text(kind)
    blob += bytes(64)
    return bytes(blob), starts


def lengths_descriptors():
    """[(offset in the blob, k)] for every base and every prefix [0, k), k = 0 .. 8400"""
    _, starts = lengths_blob()
    return [(s, k) for s in starts for k in range(LENGTHS_N + 1)]


@functools.lru_cache(None)
def prefix_sums(kind="random"):
    """(adler32, crc32) of every prefix of lengths_text, each from the one before"""
    t, a, c = lengths_text(kind), [1], [0]
    for k in range(LENGTHS_N):
        a.append(zlib.adler32(t[k:k + 1], a[-1]))
        c.append(zlib.crc32(t[k:k + 1], c[-1]))
    return a, c


@functools.lru_cache(None)
def long_random(n):
    return rand(n, 4)  # (random.Random(seed).randbytes(n) of a smaller n is no prefix of a larger one's: they differ)


@functools.lru_cache(None)
def long_zero(n):
    return bytes(n)


def long_texts():
    return [("random-%d" % n, long_random(n)) for n in LONG_LENGTHS] + [("zero-%d" % n, long_zero(n)) for n in LONG_LENGTHS]


# ---- forged-crc -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _crc_table():
    t = []
    for i in range(256):
        c = i
        for _ in range(8):
            c = (c >> 1) ^ (0xedb88320 if c & 1 else 0)
        t.append(c)
    return t


@functools.lru_cache(None)
def forged(n, target, seed=5):
    """n random bytes and four more that make the CRC-32 of the n + 4 bytes `target`: the register a byte leaves is
    T[(r ^ d) & 255] ^ (r >> 8), whose top byte names the table entry, so the four steps are walked back from the
    register `target` needs"""
    t = _crc_table()
    by_top = {v >> 24: j for j, v in enumerate(t)}
    assert len(by_top) == 256
    data = rand(n, seed + (target & 1))
    w = target ^ 0xffffffff
    for _ in range(4):
        j = by_top[w >> 24]
        w = ((w ^ t[j]) << 8 | j) & 0xffffffff
    out = data + struct.pack("<I", w ^ zlib.crc32(data) ^ 0xffffffff)
    assert zlib.crc32(out) == target
    return out


FORGED_TARGETS = (0x00000000, 0xffffffff)
EMBED_SEG = 1024              # crc32_wave's lane segment for a text of 61 * 1024 bytes: roundup(ceil(len / 64), 64)
EMBED_LEN = 61 * EMBED_SEG    # lanes 0 .. 60 have a full segment, lanes 61 .. 63 none


def forged_texts():
    return [("forged-%08x" % t, forged(1000, t)) for t in FORGED_TARGETS]


@functools.lru_cache(None)
def forged_embedded(target):
    """61 x 1024 bytes whose last 1024 are a forged text: the last lane that has bytes computes `target`, the lanes behind it
    have nothing"""
    return rand(EMBED_LEN - EMBED_SEG, 7) + forged(EMBED_SEG - 4, target)


def forged_embedded_texts():
    return [("forged-embedded-%08x" % t, forged_embedded(t)) for t in FORGED_TARGETS]


# ---- bad-trailer ------------------------------------------------------------------------------------------------------------
SMALL_SUM_TEXT = b"\x04"  # a == 5, b == 5


@functools.lru_cache(None)
def small_sum_long(n):
    """n zero bytes with one 0x04: a == 5, and the 0x04 stands where b == n + 4 (n - p) (mod 65521) is at most 14, so
    that b + 65521 still fits in 16 bits"""
    for p in range(n - 1, -1, -1):
        if (n + 4 * (n - p)) % MOD <= 14:
            return bytes(p) + b"\x04" + bytes(n - p - 1)
    raise AssertionError("no such position")


def stored_body(plain):
    """a raw DEFLATE body of stored blocks (what zlib writes at level 0)"""
    c = zlib.compressobj(0, zlib.DEFLATED, -15)
    return c.compress(plain) + c.flush()


def bad_trailers(plain, raw):
    """[(name, "zl" | "gz", frame, "checksum" | "size")] around the raw body `raw` of `plain`, whose a and b are both at most
    14: every frame is invalid"""
    a, b = adler_pair(plain)
    assert a + MOD <= 0xffff and b + MOD <= 0xffff
    crc, n = zlib.crc32(plain), len(plain) & 0xffffffff
    zl = lambda aa, bb: b"\x78\x9c" + raw + struct.pack(">I", (bb << 16 | aa) & 0xffffffff)
    gz = lambda c, s: b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + raw + struct.pack("<II", c & 0xffffffff, s & 0xffffffff)
    return [
        ("zl a + 65521", "zl", zl(a + MOD, b), "checksum"),
        ("zl b + 65521", "zl", zl(a, b + MOD), "checksum"),
        ("zl a and b + 65521", "zl", zl(a + MOD, b + MOD), "checksum"),
        ("zl a bit 0 flipped", "zl", zl(a ^ 1, b), "checksum"),
        ("zl a bit 15 flipped", "zl", zl(a ^ 0x8000, b), "checksum"),
        ("zl b bit 0 flipped", "zl", zl(a, b ^ 1), "checksum"),
        ("zl b bit 15 flipped", "zl", zl(a, b ^ 0x8000), "checksum"),
        ("gz crc bit 0 flipped", "gz", gz(crc ^ 1, n), "checksum"),
        ("gz crc bit 31 flipped", "gz", gz(crc ^ 0x80000000, n), "checksum"),
        ("gz isize bit 0 flipped", "gz", gz(crc, n ^ 1), "size"),
        ("gz isize bit 31 flipped", "gz", gz(crc, n ^ 0x80000000), "size"),
    ]


def good_frames(plain, raw):
    """the two valid frames the bad ones differ from"""
    return [("zl", b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(plain))),
            ("gz", b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + raw + struct.pack("<II", zlib.crc32(plain), len(plain) & 0xffffffff))]
