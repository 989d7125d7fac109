"""tests/checksum_cases.py on the CPU: every text is what its name says (zlib and exact Python integers), and the four
checksum accumulations of fixed geometry - the step loops of adler_of (csrc/deflate_kernel.hip), of csrc/deflate_ns.hip, of
adler_segments_kernel (csrc/inflate_chunked.hip, joined by par_adler) and of md::adler32_update (csrc/host_util.hpp) - are
restated with exact integers.  A model returns the Adler-32 it arrives at, which must be zlib's, and the largest value any of
its 32-bit intermediates holds, which must stay below 2^32 on every text - and on the `top` texts must BE the largest value
the step can reach at all: the texts are the worst case, not merely heavy.

The analytic maxima (state (65520, 65520) in front of a full step of 0xFF bytes; the last sum of the step is the largest):
  adler_of         b + 4096 a + sum (4096 - i) 255 = 65520 + 4096 * 65520 + 255 * 4096 * 4097 / 2 = 2 408 052 720
  deflate_ns       the same with 1024:               65520 + 1024 * 65520 + 255 * 1024 * 1025 / 2 =   200 982 000
  adler32_update   the same with 5552:               65520 + 5552 * 65520 + 255 * 5552 * 5553 / 2 = 4 294 690 200
                   (277 096 below 2^32: 5552 is zlib's NMAX, the longest step that fits)
  adler_segments_kernel   keeps no (a, b): a thread sums a slice of 256 bytes of a 65536-byte segment, 16 bytes a step,
                   t2 = (t2 + (256 - off) c1 - ck) % 65521.  t2 is 0 at off = 0 and at most 65520 from off = 16 on, c1 at
                   most 16 * 255: the largest value is max(256 * 4080, 65520 + 240 * 4080) = 1 044 720, reached at
                   off = 16 when the first 16 bytes leave t2 == 65520 and the next 16 are 0xFF (checksum_cases.slice_top);
                   a slice of 0xFF alone reaches 256 * 4080 = 1 044 480 at off = 0, which is what `top` shows."""
import zlib

import numpy as np
import pytest

from tests import checksum_cases as cc

MOD = cc.MOD
MAX_ADLER_OF = 65520 + 4096 * 65520 + 255 * 4096 * 4097 // 2
MAX_DEFLATE_NS = 65520 + 1024 * 65520 + 255 * 1024 * 1025 // 2
MAX_UPDATE = 65520 + 5552 * 65520 + 255 * 5552 * 5553 // 2
MAX_SEGMENTS = 65520 + 240 * 4080
MAX_SEGMENTS_FF = 256 * 4080
assert (MAX_ADLER_OF, MAX_DEFLATE_NS, MAX_UPDATE, MAX_SEGMENTS) == (2408052720, 200982000, 4294690200, 1044720)


# ---- the models -------------------------------------------------------------------------------------------------------------
def _arr(data):
    return np.frombuffer(bytes(data), np.uint8).astype(np.int64)


def _step_sums(d, step):
    """of d cut into steps of `step` bytes (the last one shorter): per step its length, sum d_i and sum (len - i) d_i"""
    n = len(d)
    k = (n + step - 1) // step
    full = np.zeros(k * step, np.int64)
    full[:n] = d
    m = full.reshape(k, step)
    lens = np.full(k, step, np.int64)
    lens[-1] = n - (k - 1) * step
    s1 = m.sum(1)
    s2 = (m * (step - np.arange(step))).sum(1) - (step - lens) * s1  # (the weights count from the step's real end)
    return lens.tolist(), s1.tolist(), s2.tolist()


def _run_steps(d, step, seed):
    """b = (b + len a + s2) % 65521, a = (a + s1) % 65521 per step -> (adler, the largest sum in front of a `%`)"""
    a, b, peak = seed & 0xffff, seed >> 16, 0
    if len(d):
        for ln, s1, s2 in zip(*_step_sums(d, step)):
            v1 = b + ln * a
            v2 = v1 + s2
            v3 = a + s1
            peak = max(peak, v1, v2, v3, s1, s2)
            b, a = v2 % MOD, v3 % MOD
    return b << 16 | a, peak


def model_adler_of(data, seed=1):
    """4096 bytes a step from the text's start; a lane's 16 bytes at x0 add t1 = sum d and (b0 - x0) t1 - tk, tk = sum k d_k"""
    d = _arr(data)
    n = len(d)
    adler, peak = _run_steps(d, 4096, seed)
    if n:
        c = (n + 15) // 16
        m = np.zeros(c * 16, np.int64)
        m[:n] = d
        m = m.reshape(c, 16)
        x0 = 16 * np.arange(c)
        b0 = np.minimum((x0 // 4096 + 1) * 4096, n)
        prod = (b0 - x0) * m.sum(1)
        assert ((prod - (m * np.arange(16)).sum(1)) >= 0).all()  # (the subtraction never goes below zero)
        peak = max(peak, int(prod.max()))
    return adler, peak


def model_deflate_ns(data):
    """1024 bytes a step, a byte at x adds d and (b0 - x) d, 16 bytes a lane"""
    d = _arr(data)
    return _run_steps(d, 1024, 1)  # ((b0 - x) d <= 1024 * 255 and a lane's 16 of them are below the step's s2, or equal to it)


def model_update(data, seed=1):
    """md::adler32_update: a += d, b += a byte by byte, `%` every 5552 bytes: both only grow inside a step, so the largest
    values are those in front of the `%`"""
    return _run_steps(_arr(data), 5552, seed)


def model_segments(data, seed=1, seg=65536):
    """adler_segments_kernel with par_adler's join: thread t of a segment's 256 sums the slice [t per, (t + 1) per), per =
    roundup(ceil(len / 256), 16), in steps of 16 bytes and then byte by byte; the 32-bit values are t1 and t2 + weight * sum
    (the join itself is 64-bit on both sides)"""
    d = _arr(data)
    a, b, peak = seed & 0xffff, seed >> 16, 0
    k16 = np.arange(16)
    for s0 in range(0, len(d), seg):
        ln = min(seg, len(d) - s0)
        per = ((ln + 255) // 256 + 15) & ~15
        full = ln // per
        sum1 = sum2 = 0
        if full:
            m = d[s0:s0 + full * per].reshape(full, per // 16, 16)
            c1, ck = m.sum(2), (m * k16).sum(2)
            t2 = np.zeros(full, np.int64)
            for j in range(per // 16):
                v = t2 + (per - 16 * j) * c1[:, j]
                peak = max(peak, int(v.max()))
                assert (v >= ck[:, j]).all()
                t2 = (v - ck[:, j]) % MOD
            t1 = c1.sum(1)
            peak = max(peak, int(t1.max()))
            a1 = per * (np.arange(full) + 1)
            t2 = (t2 + (ln - a1) % MOD * (t1 % MOD)) % MOD
            sum1, sum2 = int((t1 % MOD).sum()) % MOD, int(t2.sum()) % MOD
        a0 = full * per
        if a0 < ln:  # the one shorter slice
            sl, t1, t2, i = ln - a0, 0, 0, 0
            x = d[s0 + a0:s0 + ln].tolist()
            while i + 16 <= sl:
                c1, ck = sum(x[i:i + 16]), sum(k * v for k, v in enumerate(x[i:i + 16]))
                v = t2 + (sl - i) * c1
                peak = max(peak, v)
                t1, t2, i = t1 + c1, (v - ck) % MOD, i + 16
            for i in range(i, sl):
                v = t2 + (sl - i) * x[i]
                peak = max(peak, v)
                t1, t2 = t1 + x[i], v % MOD
            peak = max(peak, t1)
            sum1, sum2 = (sum1 + t1) % MOD, (sum2 + t2) % MOD  # (len - a1 == 0: nothing lies behind this slice)
        b = (b + ln % MOD * a + sum2) % MOD
        a = (a + sum1) % MOD
    return b << 16 | a, peak


# ---- what the names claim ---------------------------------------------------------------------------------------------------
def test_top():
    p = cc.top_prefix()
    assert len(p) == 65536 and all(len(p) % k == 0 for k in (16, 1024, 4096, 65536))
    assert zlib.adler32(p) == 0xfff0fff0 and cc.adler_pair(p) == (65520, 65520)
    assert set(p) == {0, 0xef, 0xff} and p.count(0xff) == 256 and p.count(0xef) == 1
    print("top: %d zeros, 256 x ff, ef, %d zeros" % (p.index(0xff), len(p) - p.index(0xef) - 1))
    for (name, t), n in zip(cc.top_texts(), cc.FF_RUNS):
        assert t[:65536] == p and t[65536:] == b"\xff" * n, name
    h = cc.slice_head()
    assert len(h) == 16 and sum((256 - k) * v for k, v in enumerate(h)) % MOD == 65520
    assert len(cc.slice_top()) == 65536 and cc.slice_top()[:256] == h + b"\xff" * 240 == cc.slice_top()[-256:]


def test_seeded():
    cases = cc.seeded()
    assert len(cases) == len(cc.SEEDS) * (len(cc.FF_RUNS) + 1)
    assert {(s & 0xffff, s >> 16) for s in cc.SEEDS} == {(1, 0), (65520, 65520), (65520, 0), (1, 65520), (0, 0)}
    for name, s, d in cases:
        assert set(d) == {0xff} or len(d) == 70000, name
        assert len({zlib.adler32(d, t) for t in cc.SEEDS}) == len(cc.SEEDS), name  # (the seed matters: every one gives another value)


def test_units():
    for n in cc.UNIT_LENGTHS:
        for kind, want in (("zero-a", lambda a, b: a == 0), ("one-a", lambda a, b: a == 1), ("zero-b", lambda a, b: b == 0 and a != 0)):
            t = cc.KINDS[kind](n)
            a, b = cc.adler_pair(t)
            assert len(t) == n and want(a, b), (kind, n, a, b)
            u = cc.units(kind, n, 3)
            assert [u[i * n:(i + 1) * n] for i in range(3)] == [t] * 3
    # exact integers, not zlib's reduced ones: a of zero-a IS 65521, and a length of 65521 counts as 0 in b
    assert 1 + sum(cc.zero_a(257)) == MOD and cc.adler_pair(cc.one_a(65521)) == (1, 0) and cc.adler_pair(cc.one_a(2 * 65521)) == (1, 0)


def test_one_hot():
    seen = set()
    for n in cc.ONE_HOT_LENGTHS:
        ps = cc.one_hot_positions(n)
        assert {0, 15, 16, 31, 1008, 1023, 1024, 1039, 4080, 4095, 4096, 4111, n - 1, (n - 1) // 16 * 16} <= set(ps)
        for p in ps:
            t = cc.one_hot_text(n, p)
            assert len(t) == n and t[p] == 0xff and t.count(0) == n - 1
            assert cc.adler_pair(t) == (256, (n + 255 * (n - p)) % MOD)
            seen.add(zlib.adler32(t))
    assert len(seen) == len(cc.one_hot())  # every position has a checksum of its own: a wrong weight shows


def test_lengths():
    blob, starts = cc.lengths_blob()
    t = cc.lengths_text()
    assert len(t) == 8400 and [s % 64 for s in starts] == list(cc.BASES)
    assert all(blob[s:s + 8400] == t for s in starts) and len(blob) >= starts[-1] + 8400
    desc = cc.lengths_descriptors()
    assert len(desc) == 4 * 8401 and desc[0] == (starts[0], 0) and desc[-1] == (starts[-1], 8400)
    adl, crc = cc.prefix_sums()
    for k in (0, 1, 63, 64, 65, 4095, 4096, 5553, 8399, 8400):
        assert (adl[k], crc[k]) == (zlib.adler32(t[:k]), zlib.crc32(t[:k]))
    for (name, x), n in zip(cc.long_texts(), cc.LONG_LENGTHS * 2):
        assert len(x) == n and (name.startswith("random") or x.count(0) == n)
    # the CRC-32 of a zero run depends on its length alone, and differs from length to length
    assert len({zlib.crc32(cc.long_zero(n)) for n in cc.LONG_LENGTHS}) == len(cc.LONG_LENGTHS)


def test_forged_crc():
    for (name, t), target in zip(cc.forged_texts(), cc.FORGED_TARGETS):
        assert len(t) == 1004 and zlib.crc32(t) == target, name
        assert zlib.crc32(t[:1000]) != target
    assert ((cc.EMBED_LEN + 63) // 64 + 63) & ~63 == cc.EMBED_SEG  # crc32_wave's lane segment (csrc/gz_crc.hpp)
    for (name, t), target in zip(cc.forged_embedded_texts(), cc.FORGED_TARGETS):
        assert len(t) == cc.EMBED_LEN == 61 * cc.EMBED_SEG
        assert zlib.crc32(t[60 * cc.EMBED_SEG:]) == target and zlib.crc32(t) != target, name
        assert 61 * cc.EMBED_SEG >= len(t) and 64 * cc.EMBED_SEG > len(t)  # lanes 61 .. 63: nothing


def _rejected(fmt, frame):
    try:
        zlib.decompress(frame, 15 if fmt == "zl" else 31)
    except zlib.error as e:
        return str(e)
    return None


def test_bad_trailers():
    long = cc.small_sum_long(200000)
    assert len(long) == 200000 and long.count(4) == 1 and long.count(0) == 199999
    for plain in (cc.SMALL_SUM_TEXT, long):
        a, b = cc.adler_pair(plain)
        assert a == 5 and b <= 14
        raw = cc.stored_body(plain)
        assert zlib.decompress(raw, -15) == plain
        for fmt, frame in cc.good_frames(plain, raw):
            assert _rejected(fmt, frame) is None and zlib.decompress(frame, 15 if fmt == "zl" else 31) == plain
        bad = cc.bad_trailers(plain, raw)
        assert len(bad) == 11 and len({f for _, _, f, _ in bad}) == 11
        good = dict(cc.good_frames(plain, raw))
        for name, fmt, frame, what in bad:
            msg = _rejected(fmt, frame)
            assert msg is not None, name
            assert ("length" in msg) == (what == "size"), (name, msg)
            assert frame[:-8] == good[fmt][:-8] and frame != good[fmt]  # only the trailer differs
        for name, fmt, frame, _ in bad[:3]:  # congruent, not equal
            got, want = int.from_bytes(frame[-4:], "big"), zlib.adler32(plain)
            assert got != want and (got & 0xffff) % MOD == want & 0xffff and (got >> 16) % MOD == want >> 16, name


# ---- the models on the texts ------------------------------------------------------------------------------------------------
def _all_texts():
    out = cc.top_texts() + [("slice-top", cc.slice_top())] + cc.unit_texts() + cc.one_hot() + cc.long_texts()
    out += cc.forged_texts() + cc.forged_embedded_texts() + [("lengths", cc.lengths_text()), ("empty", b"")]
    return out + [("units-%s-x3" % k, cc.units(k, 65521, 3) + b"\0") for k in cc.KINDS]


@pytest.fixture(scope="module")
def peaks():
    """every model on every text: the Adler-32 is zlib's; -> {model: {text: peak}}"""
    out = {"adler_of": {}, "deflate_ns": {}, "segments": {}, "update": {}}
    for name, t in _all_texts():
        want = zlib.adler32(t)
        for key, f in (("adler_of", model_adler_of), ("deflate_ns", model_deflate_ns), ("segments", model_segments), ("update", model_update)):
            got, out[key][name] = f(t)
            assert got == want, (key, name)
    return out


def test_models_equal_zlib_and_stay_below_2_32(peaks):
    for key, per_text in peaks.items():
        assert len(per_text) == len(_all_texts())
        worst = max(per_text, key=per_text.get)
        print("%-10s largest 32-bit value over %d texts: %d (%s), %.4f of 2^32" % (key, len(per_text), per_text[worst], worst, per_text[worst] / 2 ** 32))
        assert max(per_text.values()) < 1 << 32


def test_top_attains_the_analytic_maxima(peaks):
    """a step of 0xFF in state (65520, 65520) is the worst case of a step, and the `top` texts hold one whenever the run of
    0xFF is a whole step long"""
    for n in cc.FF_RUNS:
        name = "top-%d" % n
        assert (peaks["adler_of"][name] == MAX_ADLER_OF) == (n >= 4096), name
        assert (peaks["deflate_ns"][name] == MAX_DEFLATE_NS) == (n >= 1024), name
        assert peaks["segments"][name] == MAX_SEGMENTS_FF, name  # (P's own run of 0xFF crosses into a slice that begins with 16 of them)
    assert peaks["segments"]["slice-top"] == MAX_SEGMENTS
    for key, bound in (("adler_of", MAX_ADLER_OF), ("deflate_ns", MAX_DEFLATE_NS), ("segments", MAX_SEGMENTS), ("update", MAX_UPDATE)):
        assert max(peaks[key].values()) <= bound, key  # no text goes above what the analysis calls the maximum
    print("maxima attained: adler_of %d, deflate_ns %d, adler_segments_kernel %d (a slice of 0xFF alone: %d)"
          % (MAX_ADLER_OF, MAX_DEFLATE_NS, MAX_SEGMENTS, MAX_SEGMENTS_FF))


def test_seeded_and_pieces():
    """the models that take a running value: adler_of (a stream encoded in slices), par_adler (the continue path) and
    adler32_update (the streaming shims, one call per piece the caller hands in).  adler32_update's steps count from the
    start of a CALL, so its worst case is a call that starts in (65520, 65520): `top` handed in as P, then the run"""
    worst = {"adler_of": 0, "segments": 0, "update": 0}
    for name, seed, d in cc.seeded():
        want = zlib.adler32(d, seed)
        for key, f in (("adler_of", model_adler_of), ("segments", model_segments), ("update", model_update)):
            got, peak = f(d, seed)
            assert got == want and peak < 1 << 32, (key, name)
            worst[key] = max(worst[key], peak)
            if seed == 0xfff0fff0 and set(d) == {0xff}:
                step, bound = {"adler_of": (4096, MAX_ADLER_OF), "segments": (0, MAX_SEGMENTS_FF), "update": (5552, MAX_UPDATE)}[key]
                if key != "segments":
                    assert (peak == bound) == (len(d) >= step), (key, name)
                elif len(d) >= 65536:  # (a 0xFF slice of 256 bytes: a segment of 65536)
                    assert peak == bound, (key, name)
    assert (worst["adler_of"], worst["update"]) == (MAX_ADLER_OF, MAX_UPDATE)
    p = cc.top_prefix()
    for n in cc.FF_RUNS:
        for piece in (4095, 4096, 4097, 65536, 65537):  # adler32_update chained over pieces, as md_def_src does
            t = cc.top(n)
            s, peak = 1, 0
            for i in range(0, len(t), piece):
                s, pk = model_update(t[i:i + piece], s)
                peak = max(peak, pk)
            assert s == zlib.adler32(t) and peak < 1 << 32
            if piece == 65536:
                assert (peak == MAX_UPDATE) == (n >= 5552), n
    print("maxima attained: adler32_update %d" % MAX_UPDATE)
