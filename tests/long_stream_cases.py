"""Hand-built streams for the long-stream inflate path (csrc/inflate_chunked.hip, par_decode in csrc/capi_long_stream.cpp),
and a CPU-side prediction of how that path cuts them into pieces.  tests/test_long_stream_cases.py proves on the CPU that
every stream has the shape its family names; tests/test_gpu_long_stream.py runs them through the kernels.

A stream is put together from UNITS: `dw.write(blocks + [an empty stored block])` ends byte-aligned on a flush marker
(00 00 ff ff), so units concatenate as bytes and dw's slow bit writer runs once per distinct unit.  Non-empty stored
blocks between units (written here directly: a byte-aligned stored block is 00 LEN NLEN data) move the next unit to the
byte where a test wants it.  The plaintext is dw.expand's; the true block starts come from dw.write(starts=).

With inflate_parallel_chunk = 4 the path cuts the body into chunks of K = 4096 bytes and takes the first candidate block
start of every chunk behind the first (a flush marker, or a non-final dynamic header that parses).  `predict` restates
those rules, so a case knows its piece count before a GPU sees it: `Stream.goto` ends a padding block exactly where the
next piece shall start, and a piece of an exact size is a unit whose end lies one byte into a later chunk.

A single stream reaches the path from 16 KiB of input through md_de_inf_continue_host, but only from 128 KiB through the
*_higher_uncompress entry points (md_inflate_batch_host hands a stream of a batch of n to it from max(inflate_parallel_min,
n x 128 KiB) on), so every case but family H's is filled up to HIGHER_MIN bytes with stored noise, which holds no
candidates (predict would say so) and adds no pieces.

Families: W windows, S piece sizes, R reach in front of the stream's start, G jump groups, F finder, X expansion,
C checksums, H history."""
import functools
import random
import struct
import zlib
from collections import namedtuple

import numpy as np

from tests import deflate_writer as dw
from tests.deflate_writer import Block

K = 4096                # inflate_parallel_chunk = 4
HIGHER_MIN = 128 << 10  # a stream of a batch of one takes the path from here on
CONT_MIN = 16 << 10     # inflate_parallel_min = 16: md_de_inf_continue_host
WIN = 32768
JUMP_FROM = 24          # pieces from which the windows come by pointer jumping (below: the one-workgroup chain)
GROUP = 1023            # pieces of a jump group
MARKER = b"\x00\x00\xff\xff"

# pieces: {frame: predicted piece count, or None where a false candidate or a growing piece makes the path decode again};
# false: the predicted piece starts that are no block starts; design: bits the case means to be piece starts
Case = namedtuple("Case", "name family variant raw plain starts status pieces rounds2 false design meta")


# ---- the prediction -------------------------------------------------------------------------------------------------------
_HEADER_BITS = [0]  # the length of the header that header_parses read last


def header_parses(body, q):
    """a non-final dynamic header at bit q that the finder admits: HLIT / HDIST fields <= 29, a complete code-length
    code, lengths that decode without overrunning HLIT + HDIST (and no repeat at the first), a complete literal/length code
    with an end-of-block code, a distance code that is complete, empty or one 1-bit code - all inside the body"""
    v = int.from_bytes(body[q >> 3:(q >> 3) + 640], "little") >> (q & 7)
    if v & 7 != 4 or (v >> 3) & 31 > 29 or (v >> 8) & 31 > 29:
        return False
    hlit, hdist, hclen = ((v >> 3) & 31) + 257, ((v >> 8) & 31) + 1, ((v >> 13) & 15) + 4
    v >>= 17
    cl = [0] * 19
    for i in range(hclen):
        cl[dw.CL_ORDER[i]] = v & 7
        v >>= 3
    used = 17 + 3 * hclen
    if sum(128 >> l for l in cl if l) != 128:
        return False
    lut = [None] * 128
    for sym, (code, l) in dw.canonical(cl).items():
        rev = int(format(code, "0%db" % l)[::-1], 2)
        for k in range(rev, 128, 1 << l):
            lut[k] = (sym, l)
    total, i, prev = hlit + hdist, 0, 0
    lsum = dsum = dcodes = d1 = 0
    eob = False
    while i < total:
        sym, l = lut[v & 127]
        v >>= l
        used += l
        rep, val = 1, sym
        if sym == 16:
            if i == 0:
                return False
            rep, val = 3 + (v & 3), prev
            v >>= 2
            used += 2
        elif sym == 17:
            rep, val = 3 + (v & 7), 0
            v >>= 3
            used += 3
        elif sym == 18:
            rep, val = 11 + (v & 127), 0
            v >>= 7
            used += 7
        if i + rep > total:
            return False
        if val:
            nl = max(0, min(i + rep, hlit) - i)
            nd = rep - nl
            lsum += nl * (32768 >> val)
            dsum += nd * (32768 >> val)
            dcodes += nd
            d1 += nd if val == 1 else 0
            eob = eob or i <= 256 < i + rep
            if lsum > 32768 or dsum > 32768:
                return False
        i += rep
        prev = val
    _HEADER_BITS[0] = used
    if q + used > 8 * len(body):
        return False
    return eob and lsum == 32768 and (dsum == 32768 or dcodes == 0 or (dcodes == 1 and d1 == 1))


def _filter(seg, k):
    """of the chunk seg[5:5 + k] (five bytes in front of it, the bytes behind it as far as the body goes): the bit
    positions, relative to the chunk, whose first 17 bits read as a non-final dynamic header with HLIT / HDIST fields <= 29
    and whose code-length code is complete, sorted; and the chunk's flush markers"""
    a = np.frombuffer(seg, np.uint8)
    by = np.arange(5, min(len(a), 5 + k))
    marks = by[(a[by - 4] == 0) & (a[by - 3] == 0) & (a[by - 2] == 255) & (a[by - 1] == 255) & ((a[by - 5] & 0xe0) == 0)] - 5
    n = len(by)
    pad = np.concatenate([a[5:], np.zeros(24, np.uint8)]).astype(np.uint64)
    lo = np.zeros(n, np.uint64)
    hi = np.zeros(n, np.uint64)
    for b in range(8):
        lo |= pad[b:b + n] << np.uint64(8 * b)
        hi |= pad[8 + b:8 + b + n] << np.uint64(8 * b)
    out, u = [], np.uint64
    for s in range(8):
        v0 = lo if s == 0 else (lo >> u(s)) | (hi << u(64 - s))
        ok = ((v0 & u(7)) == u(4)) & (((v0 >> u(3)) & u(31)) <= u(29)) & (((v0 >> u(8)) & u(31)) <= u(29))
        idx = np.nonzero(ok)[0]
        a0, a1 = v0[idx], hi[idx] >> u(s)
        hclen = ((a0 >> u(13)) & u(15)).astype(np.int64) + 4
        kraft = np.zeros(len(idx), np.int64)
        for i in range(19):
            at = 17 + 3 * i
            f = (((a0 >> u(at)) | (a1 << u(64 - at)) if at < 64 else a1 >> u(at - 64)) & u(7)).astype(np.int64)
            kraft += np.where((i < hclen) & (f > 0), 128 >> f, 0)
        out.append(idx[kraft == 128] * 8 + s)
    return np.sort(np.concatenate(out)).tolist(), (marks * 8).tolist()


_CHUNKS = {}  # what a chunk's bytes say, for the streams that share them (a family's streams differ in a few chunks)


def _first_candidate(body, c, k):
    """the first candidate bit of chunk c, or None: a marker or a header that parses, with 29 bits left in chunk and body"""
    lo, nbits = c * k, 8 * len(body)
    seg = body[lo - 5:lo + k + 700]
    key = (seg, k, nbits - 8 * lo if lo + k + 700 >= len(body) else None)
    if key not in _CHUNKS:
        end = min(8 * k, nbits - 8 * lo)
        heads, marks = _filter(seg, k)
        best = next((q for q in marks if q + 29 <= end), None)
        for q in heads:
            if best is not None and q > best or q + 29 > end:
                break
            if header_parses(seg[5:], q) and 8 * lo + q + _HEADER_BITS[0] <= nbits:
                best = q
                break
        _CHUNKS[key] = best
    return None if _CHUNKS[key] is None else 8 * lo + _CHUNKS[key]


def _hop_stored(body, pos, k):
    """the run of non-final stored blocks from bit pos on -> (the bit behind it, block starts in it at least k bytes apart)"""
    mids, last_mid, n = [], pos, len(body)
    while True:
        by = pos >> 3
        if by + 5 > n:
            break
        if ((body[by] | body[by + 1] << 8) >> (pos & 7)) & 7:
            break
        at = (pos + 10) >> 3
        if at + 4 > n:
            break
        ln, nl = struct.unpack_from("<HH", body, at)
        if ln ^ nl != 0xffff or at + 4 + ln > n:
            break
        if pos >= last_mid + 8 * k:
            mids.append(pos)
            last_mid = pos
        pos = 8 * (at + 4 + ln)
    return pos, mids


def predict(body, k=K, start_bit=0):
    """the piece starts (bits) the path begins with: the stream's start, the stored-run seeds behind it, then of every
    chunk [c k, (c + 1) k), c >= 1, the first candidate with 29 bits left inside the chunk and the body"""
    body = bytes(body)
    nbits = 8 * len(body)
    cand = [_first_candidate(body, c, k) for c in range(1, (len(body) + k - 1) // k)]
    starts = [start_bit]
    x, mids = _hop_stored(body, start_bit, k)
    if start_bit < x < nbits:
        mids.append(x)
    for s in mids:
        if s > starts[-1]:
            starts.append(s)
    seeded = starts[-1]
    for q in cand:
        if q is not None and q > seeded and q > starts[-1]:
            starts.append(q)
    return starts


def judge(starts, true_starts, final_bit):
    """(piece count when every start is a block start: the pieces up to the one that holds the final block; false starts)"""
    true = {b for b, _ in true_starts}
    false = [s for s in starts[1:] if s not in true and s <= final_bit]
    if false or len(starts) < 3:
        return None, false
    return sum(1 for s in starts if s <= final_bit), false


# ---- units and streams ----------------------------------------------------------------------------------------------------
def out_len(block):
    return sum(1 if isinstance(t, int) else dw._norm(t).length for t in block.tokens)


def _plain_twin(b):
    """the same tokens without a spelled-out header: what dw.expand accepts (the header does not change the bytes)"""
    if b.cl_lens is None and b.hclen is None and b.cl_syms is None:
        return b
    return Block(b.kind, b.tokens, lit_lens=b.lit_lens, dist_lens=b.dist_lens, hlit=b.hlit, hdist=b.hdist, extra=b.extra, last=b.last)


class Unit:
    """blocks (every one with `last` set) and an empty stored block behind them: byte-aligned at both ends"""

    def __init__(self, blocks, marker=True):
        self.blocks = list(blocks) + ([Block("stored", [], last=False)] if marker else [])
        assert all(b.last is not None for b in self.blocks)
        self.starts = []
        self.raw = dw.write(self.blocks, starts=self.starts)
        self.outs = [out_len(b) for b in self.blocks]
        self.blocks = [_plain_twin(b) for b in self.blocks]


def stored_unit(data, last=False):
    """a byte-aligned stored block, written directly (tests/test_long_stream_cases.py compares it with dw.write)"""
    assert isinstance(data, bytes) and len(data) <= 65535
    u = Unit.__new__(Unit)
    b = Block("stored", (), last=last)  # (its tokens set directly: Block would look at every byte of 60 000 again)
    b.tokens = list(data)
    u.blocks, u.starts, u.outs = [b], [0], [len(data)]
    u.raw = bytes([1 if last else 0]) + struct.pack("<HH", len(data), len(data) ^ 0xffff) + bytes(data)
    return u


class Stream:
    def __init__(self, seed, fill=None):
        self.rng, self.fill = random.Random(seed), fill
        self.raw, self.blocks, self.starts, self.out = bytearray(), [], [], 0
        self.design = []

    def add(self, unit):
        base = 8 * len(self.raw)
        for b, s, o in zip(unit.blocks, unit.starts, unit.outs):
            self.blocks.append(b)
            self.starts.append((base + s, self.out))
            self.out += o
        self.raw += unit.raw
        return base

    def noise(self, n):
        return bytes([self.fill]) * n if self.fill is not None else self.rng.randbytes(n)

    def stored(self, n):
        while n > 0:
            m = min(n, 60001)
            self.add(stored_unit(self.noise(m)))
            n -= m

    def goto(self, target):
        """padding and a marker that ends at byte `target`: a piece is meant to start there"""
        rem = target - len(self.raw) - 5  # (the marker's five bytes)
        assert rem >= 6, (target, len(self.raw))
        while rem:
            m = min(rem, 60006)
            if 0 < rem - m < 6:  # (a stored block is its five-byte header and at least one byte here)
                m -= 6
            self.add(stored_unit(self.noise(m - 5)))
            rem -= m
        self.add(stored_unit(b""))
        assert len(self.raw) == target, (len(self.raw), target)
        self.design.append(8 * target)

    def next_chunk(self, skip=0):
        """the next piece starts one byte into the next chunk (or `skip` chunks further)"""
        self.goto(((len(self.raw) + 11) // K + 1 + skip) * K + 1)

    def exact(self, unit):
        """`unit` as a piece of its own: it ends one byte into a chunk, and starts in a chunk that has no piece start yet"""
        L = len(unit.raw)
        last = self.design[-1] // 8 if self.design else 0
        c = 1
        while c * K + 1 - L < len(self.raw) + 11 or (c * K + 1 - L) // K <= last // K:
            c += 1
        self.goto(c * K + 1 - L)
        self.add(unit)
        self.design.append(8 * len(self.raw))

    def fill_to(self, nbytes):
        if len(self.raw) < nbytes:
            self.stored(nbytes - len(self.raw))

    def finish(self, tokens=(), kind="fixed"):
        final = 8 * len(self.raw)
        self.add(Unit([Block(kind, tokens, last=True)], marker=False))
        return final


def frame(raw, plain, fmt):
    if fmt == "zl":
        return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(plain))
    if fmt == "gz":
        return b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + raw + struct.pack("<II", zlib.crc32(plain), len(plain) & 0xffffffff)
    return raw


TRAILER = {"de": 0, "zl": 4, "gz": 8}


def _case(name, family, variant, s, final, frames=("de",), rounds2=False, hist=b"", plain=None, meta=None, cut=None):
    raw = bytes(s.raw)
    if plain is None:
        status, full = dw.expand([Block("stored", hist, last=False)] + s.blocks if hist else s.blocks)
        plain = full[len(hist):]
    else:
        status = dw.OK
    pieces, false, preds = {}, [], {}
    if status != dw.OK or cut is not None:
        frames = ("de",)
    for fmt in frames:
        body = frame(raw, plain, fmt)[{"de": 0, "zl": 2, "gz": 10}[fmt]:] if cut is None else raw[:cut]
        preds[fmt] = predict(body)
        pieces[fmt], f = judge(preds[fmt], s.starts, final if cut is None else 8 * cut)
        false = false or f
    meta = dict(meta or {}, total=s.out, final=final, hist=hist, cut=cut, predicted=preds)
    return Case(name, family, variant, raw, plain, list(s.starts), status, pieces, rounds2, false, list(s.design), meta)


# ---- shared units ---------------------------------------------------------------------------------------------------------
LENS = (3, 4, 5, 17, 258)
DISTS = (1, 4097, WIN - 255, WIN - 1, WIN)


@functools.lru_cache(None)
def mixed(seed, ntok=2600, pmatch=0.2, dists=DISTS, kind="dynamic"):
    """random literals mixed with matches of the lengths and distances above: needs 32 KiB of output in front"""
    rng = random.Random(1000 + seed)
    toks = [(rng.choice(LENS), rng.choice(dists)) if rng.random() < pmatch else rng.randrange(256) for _ in range(ntok)]
    return Unit([Block(kind, toks, last=False)])


def lits(rng, n, lo=0, hi=256):
    return [rng.randrange(lo, hi) for _ in range(n)]


@functools.lru_cache(None)
def window_copy():
    """exactly 32768 bytes, every one of them the byte 32768 in front of it"""
    return Unit([Block("fixed", [(258, WIN)] * 126 + [(130, WIN)] * 2, last=False)])


@functools.lru_cache(None)
def reader(seed):
    """reads deep into the window: its first and last bytes, and all of it once"""
    rng = random.Random(2000 + seed)
    toks = [(258, WIN), (3, WIN), (17, WIN - 1), (5, WIN - 255)]
    for d in range(WIN, 300, -1290):
        toks += [(258, d), rng.randrange(256)]
    return Unit([Block("dynamic", toks + [(258, WIN)] * 4, last=False)])


def _front(s):
    s.add(stored_unit(s.noise(40000)))  # (piece 1 starts behind it: a stored run at the stream's start is followed on the host)
    s.design.append(8 * len(s.raw))
    s.add(Unit([Block("fixed", [s.rng.randrange(144) if s.fill is None else s.fill], last=False)]))  # (the run ends here: the padding behind it is the finder's)


def _extras(s, n, seed=0):
    for i in range(n):
        s.add(mixed(seed + i % 5))
        s.next_chunk()


def _close(s, ntail=3):
    s.fill_to(HIGHER_MIN)
    return s.finish(lits(s.rng, ntail))


# ---- W, S, R --------------------------------------------------------------------------------------------------------------
def family_w():
    cases = []
    for variant, n in (("chain", 4), ("jump", 14)):
        s = Stream(11)
        _front(s)
        _extras(s, n)
        s.exact(window_copy())
        s.add(reader(0))
        s.next_chunk()
        s.exact(window_copy())  # (a copy of a copy: the window behind it descends from the one in front of the first)
        _extras(s, n, seed=2)
        cases.append(_case("W " + variant, "W", variant, s, _close(s)))
    return cases


SIZES = (0, 1, 15, 16, 17, WIN - 1, WIN, WIN + 1, 65536 + 5)


@functools.lru_cache(None)
def sized(n, seed=0):
    """a piece of exactly n bytes: literals below 144 and, from 300 bytes on, matches at the far end of the window"""
    if n == 0:
        return Unit([])  # two markers with nothing between them
    rng = random.Random(3000 + n + seed)
    toks, left = [], n
    while left:
        if left >= 300 and rng.random() < 0.5:
            m = min(258, left - 3) if left < 600 else 258
            toks.append((m, rng.choice((WIN, WIN - 1, 1))))
            left -= m
        else:
            toks.append(rng.randrange(144))
            left -= 1
    return Unit([Block("fixed", toks, last=False)])


def family_s():
    cases = []
    for variant, extra in (("chain", 0), ("jump", 8)):
        s = Stream(21)
        _front(s)
        _extras(s, extra)
        for i, n in enumerate(SIZES):
            s.exact(sized(n))
            s.add(reader(i))
        s.next_chunk()
        cases.append(_case("S sizes " + variant, "S", variant, s, _close(s), meta={"sizes": SIZES}))
    # runs of pieces that are all shorter than 4 KiB of output: the window slides across many of them
    for variant, runs in (("chain", 14), ("jump", 40)):
        s = Stream(22)
        _front(s)
        s.goto(11 * K + K - 48)
        for i in range(runs):  # each starts 90 bytes earlier in its chunk than the one before (4006 bytes of input) and ends in it
            s.add(Unit([Block("fixed", lits(s.rng, 5) + [(17, WIN), (4, WIN - 1)] + [(3, WIN - (3 + j) * 3900) for j in range(4)], last=False)]))
            assert len(s.raw) % K > 40  # (the unit and its marker end in the chunk they start in)
            s.goto((12 + i) * K + K - 48 - 90 * (i + 1))
        s.add(reader(1))
        s.next_chunk()
        cases.append(_case("S short run " + variant, "S", variant, s, _close(s), meta={"short": runs}))
    # every residue of a piece's length mod 16 (resolve_kernel's tail)
    # (16 sized pieces and their readers are too many for the chain: two streams there)
    for name, variant, extra, rs in (("jump", "jump", 10, range(16)), ("chain 0-7", "chain", 0, range(8)), ("chain 8-15", "chain", 0, range(8, 16))):
        s = Stream(23)
        _front(s)
        _extras(s, extra)
        for r in rs:
            s.exact(sized(32 + r if r % 2 else 4112 + r, seed=r))
            s.add(reader(r))
        s.next_chunk()
        cases.append(_case("S mod 16 " + name, "S", variant, s, _close(s), meta={"mod16": list(rs)}))
    return cases


def family_r():
    """the stream's first pieces, with less than 32 KiB in front of them: matches that reach byte 0 of the output (valid),
    and one byte further (Invalid_distance).  bad: None, "resolve" (early in a piece of more than 32 KiB: only
    resolve_kernel meets it), "tail1" / "tail2" / "taillast" (in the last 32 KiB of piece 1, 2, the last such piece)"""
    cases = []
    for variant, extra in (("chain", 3), ("jump", 22)):
        for bad in (None, "resolve", "tail1", "tail2", "taillast"):
            s = Stream(31)
            s.add(Unit([Block("fixed", lits(s.rng, 3000, 100, 256), last=False)]))  # (9-bit literals: piece 8 starts ~300 bytes short of 32 KiB)
            s.next_chunk()
            p, front = 1, []
            while s.out < WIN - 60:
                last_one = s.out + 4060 >= WIN - 60
                o = s.out
                front.append(o)
                if bad == "resolve" and p == 1:
                    toks = [(3, o + 1), 65] + [(258, 1)] * 130
                elif bad == "tail%d" % p or (bad == "taillast" and last_one):
                    toks = lits(s.rng, 20) + [(3, o + 21)] + lits(s.rng, 5)
                else:  # byte 0 exactly, twice, and bytes that mix literals with it
                    toks = [(10, o)] + lits(s.rng, 30) + [(7, o + 40), 66, (3, o + 48), 67, (4, o + 52)]
                s.add(Unit([Block("fixed", toks, last=False)]))
                s.next_chunk()
                p += 1
            s.stored(max(0, WIN + 100 - s.out))
            s.next_chunk()
            _extras(s, extra)
            cases.append(_case("R %s %s" % (bad or "byte 0", variant), "R", variant, s, _close(s), meta={"front": front, "bad": bad}))
    return cases


# ---- G --------------------------------------------------------------------------------------------------------------------
def family_g():
    """1023, 1024, 1025, 1026 and 1100 pieces: 16 distinct units of about 2 KiB in a seeded random order, so that nearly
    every chunk holds a marker; the streams are prefixes of one another, and so are their plaintexts"""
    rng = random.Random(41)
    units = [mixed(100 + i, ntok=1500 + 100 * (i % 7), pmatch=0.03) for i in range(16)]
    s = Stream(41)
    _front(s)
    marks = []  # (body length, blocks, starts, output) after every unit
    for i in range(2500):
        s.add(units[rng.randrange(16)])
        marks.append((len(s.raw), len(s.blocks), s.out))
    status, full = dw.expand(s.blocks)
    assert status == dw.OK
    whole = predict(bytes(s.raw))
    cases = []
    # (with 1023 pieces in front of it a second group begins at piece 1024; the window it is handed is first USED for the
    # window in front of piece 1025, so from 1026 pieces on)
    for want in (GROUP, GROUP + 1, GROUP + 2, GROUP + 3, 1100):
        # every unit boundary is a candidate of the whole stream and of its prefix alike: the pieces of a prefix are about the
        # starts up to its end.  The final block is a reader: the last piece reads all of the window in front of it
        i0 = next(i for i, (nraw, _, _) in enumerate(marks) if sum(1 for q in whole[:want + 1] if q <= 8 * nraw) == want)
        for nraw, nblk, nout in marks[max(0, i0 - 3):i0 + 4]:
            t = Stream(42)
            t.raw, t.blocks, t.starts, t.out = bytearray(s.raw[:nraw]), s.blocks[:nblk], s.starts[:nblk], nout
            tail = reader(0).blocks[0].tokens + lits(t.rng, 7)
            final = t.finish(tail, kind="dynamic")
            status, read = dw.expand([Block("stored", full[nout - WIN:nout], last=False), t.blocks[-1]])
            case = _case("G %d pieces" % want, "G", "jump", t, final, plain=full[:nout] + read[WIN:], meta={"want": want})
            if case.pieces["de"] == want and status == dw.OK:
                cases.append(case)
                break
        else:
            raise AssertionError("no prefix with %d pieces" % want)
    return cases


# ---- F --------------------------------------------------------------------------------------------------------------------
def _behind_fixed(s, block, phase, at_chunk_end=0):
    """`block` (dynamic) behind a small fixed block so that it starts at bit `phase` of a byte, one byte into a chunk
    (at_chunk_end: that many bits in front of a chunk's end instead) -> the bit where it starts"""
    n9 = (phase - 2) % 8  # a fixed block of n 9-bit and three 8-bit literals is 3 + 9 n + 24 + 7 bits long
    u = Unit([Block("fixed", [200] * n9 + [65] * 3, last=False), block])
    rel = u.starts[1]
    assert rel % 8 == phase
    c = (len(s.raw) + 11 + rel // 8) // K + 2
    target = c * K + 1 if not at_chunk_end else c * K - (at_chunk_end + 7) // 8
    s.goto(target - rel // 8)
    s.design.pop()  # (the unit's own start may lie in the chunk's last 29 bits)
    base = s.add(u)
    return base + rel


def _copy(block):
    import copy
    b = copy.copy(block)
    b.last = False
    return b


def header_blocks():
    """valid non-final headers from tests/deflate_header_cases.py's stock: (name, block)"""
    from tests import deflate_header_cases as hc
    rng = random.Random(51)
    few = hc._lit(hc.FEW_LIT)
    out = [("no distance code, HCLEN %d" % k, hc.dyn(hc._hclen_needed(k), [0])) for k in (5, 12, 18, 19)]
    out.append(("HCLEN 5 sent as 19", hc.dyn(hc._hclen_needed(5), [0], hclen=19)))
    for sd in (0, 29):
        out.append(("lone distance code %d" % sd, hc.dyn(few, [0] * sd + [1], have=33000, hdist=sd + 1)))
    lit = hc._lit({97: 1, 256: 2, 285: 2}, 286)
    out.append(("HLIT 29 HDIST 29", hc.dyn(lit, [1] + [0] * 28 + [1], have=33000, hlit=286, hdist=30)))
    lit8 = [0] + [8] * 256
    out.append(("two 1-bit code-length codes", hc.spelled(lit8, [0], [(l, 0) for l in lit8 + [0]])))
    out.append(("longest codes 15 bits", hc.dyn(hc.spread(hc.complete_code(286, 15, rng), 286, (256,), rng), hc.NEAR_DIST)))
    return [(n, _copy(b)) for n, b in out]


FRAMES = ("de", "zl", "gz")


def family_f():
    cases = []
    small = lambda i: Block("dynamic", mixed(i).blocks[0].tokens[:300], last=False)
    for variant, extra in (("chain", 0), ("jump", 16)):
        s = Stream(51)
        _front(s)
        _extras(s, extra)
        want = [_behind_fixed(s, small(ph), ph) for ph in range(8)]
        late = _behind_fixed(s, small(9), 3, at_chunk_end=16)  # 16 bits in front of a chunk's end: no candidate
        s.next_chunk()
        cases.append(_case("F phases " + variant, "F", variant, s, _close(s), frames=FRAMES, meta={"want": want, "late": late}))
    hb = header_blocks()
    for variant, extra, part in (("chain", 0, hb[:6]), ("chain", 0, hb[6:]), ("jump", 14, hb)):
        s = Stream(52)
        _front(s)
        _extras(s, extra)
        want = [_behind_fixed(s, b, 1 + i % 7) for i, (_, b) in enumerate(part)]
        s.next_chunk()
        cases.append(_case("F headers %s %s" % (variant, part[0][0]), "F", variant, s, _close(s), frames=FRAMES,
                           meta={"headers": list(zip([n for n, _ in part], want))}))
    for variant, extra in (("chain", 3), ("jump", 20)):  # ends in an empty stored block: the trailer is a candidate
        s = Stream(53)
        _front(s)
        _extras(s, extra)
        s.fill_to(HIGHER_MIN)
        s.goto((len(s.raw) // K + 3) * K - 2)  # (in a chunk's last 29 bits: the final block's start is no candidate, the trailer is)
        s.design.pop()
        final = s.finish((), kind="stored")
        cases.append(_case("F trailer " + variant, "F", variant, s, final, frames=FRAMES, meta={"trailer": 8 * len(s.raw)}))
    for what in ("header", "marker"):
        for variant, extra in (("chain", 3), ("jump", 20)):
            s = Stream(54)
            _front(s)
            _extras(s, extra)
            s.next_chunk()
            payload = mixed(7).raw if what == "header" else b"\x15" + MARKER + s.noise(40)
            here = len(s.raw) + 5
            at = (here // K + 2) * K + 9  # the payload is the first thing a candidate can be in its chunk
            s.add(stored_unit(s.noise(at - here) + payload + s.noise(3 * K)))
            false = 8 * at if what == "header" else 8 * (at + 5)
            _extras(s, 2)
            cases.append(_case("F false %s %s" % (what, variant), "F", variant, s, _close(s), frames=FRAMES, rounds2=True,
                               meta={"false": false}))
    return cases


# ---- X --------------------------------------------------------------------------------------------------------------------
def family_x():
    cases = []
    for variant, extra in (("chain", 3), ("jump", 20)):
        s = Stream(61)
        _front(s)
        _extras(s, extra)
        s.add(Unit([Block("fixed", [7] + [(258, 1)] * 600, last=False)]))  # 975 bytes in, 154 801 out
        s.next_chunk()
        _extras(s, 2)
        cases.append(_case("X fixed 258-matches " + variant, "X", variant, s, _close(s), rounds2=True))
    s = Stream(62)
    _front(s)
    _extras(s, 3)
    s.add(Unit([Block("dynamic", [9] + [(258, 1)] * 16256, last=False)]))  # two bits a match: 4 064 bytes in, 4 MiB out
    s.next_chunk()
    _extras(s, 2)
    cases.append(_case("X 1032 to 1 chain", "X", "chain", s, _close(s), rounds2=True))
    return cases


# ---- C --------------------------------------------------------------------------------------------------------------------
ADLER_RES = (0, 1, 15, 16, 17, 4095, 4096, 4097, 65535)
CRC_LENS = ((1 << 20) - 1, 1 << 20, (1 << 20) + 1, (2 << 20) + 17)


def _sized_stream(seed, extra, total=None, residue=None, fill=None):
    s = Stream(seed, fill=fill)
    _front(s)
    for i in range(extra):
        if fill is None:
            s.add(mixed(i % 5))
        else:
            s.add(Unit([Block("fixed", [fill] * 40 + [(258, 1), (17, 4097), (258, WIN), fill, (5, WIN - 1)] * 20, last=False)]))
        s.next_chunk()
    s.fill_to(HIGHER_MIN)
    k = 3
    if total is None:
        total = s.out + 70
        total += (residue - total) % 65536
    s.stored(total - k - s.out)
    final = s.finish([fill if fill is not None else 33] * k)
    assert s.out == total
    return s, final


def family_c():
    cases = []
    for variant, extra in (("chain", 5), ("jump", 26)):
        for r in ADLER_RES:
            s, final = _sized_stream(71, extra, residue=r)
            cases.append(_case("C zlib %d mod 65536 %s" % (r, variant), "C", variant, s, final, frames=("de", "zl"), meta={"residue": r}))
        s, final = _sized_stream(72, extra, residue=65535, fill=0xff)
        cases.append(_case("C all ff " + variant, "C", variant, s, final, frames=FRAMES, meta={"ff": True, "residue": 65535}))
    for n in CRC_LENS:
        s, final = _sized_stream(73, 5, total=n)
        cases.append(_case("C gzip %d bytes" % n, "C", "chain", s, final, frames=("de", "gz"), meta={"length": n}))
    s, final = _sized_stream(73, 26, total=CRC_LENS[-1])
    cases.append(_case("C gzip %d bytes jump" % CRC_LENS[-1], "C", "jump", s, final, frames=("de", "gz"), meta={"length": CRC_LENS[-1]}))
    return cases


# ---- H --------------------------------------------------------------------------------------------------------------------
NEAR = (1, 2, 300, 4000)


def family_h():
    """the second piece of the decode protocol: `hist` bytes of window in front, the body from a block boundary on.
    reach: "first" = matches in pieces 1 and later at the history's first byte, "past" = one byte in front of it,
    "window" = at distance 32768 (the history is a full window: nothing of it lies further)"""
    cases = []
    for variant, extra in (("chain", 4), ("jump", 26)):
        for hl, reach in ((1, "first"), (1, "past"), (20000, "first"), (20000, "past"), (WIN - 1, "window"), (WIN, "window")):
            s = Stream(81 + hl)
            hist = s.noise(hl)
            s.add(Unit([Block("fixed", lits(s.rng, 3000, 0, 144), last=False)]))
            s.next_chunk()
            for p in (1, 2):
                o = s.out
                if reach == "window":
                    toks = [(9, WIN)] + lits(s.rng, 9) + [(258, WIN), (3, WIN - 1)]
                elif reach == "first" or p == 1:
                    toks = [(9, o + hl)] + lits(s.rng, 9) + [(4, o + hl + 18)]
                else:
                    toks = lits(s.rng, 9) + [(3, o + hl + 10)]
                s.add(Unit([Block("fixed", toks, last=False)]))
                s.next_chunk()
            for i in range(extra):
                s.add(mixed(200 + i % 5, ntok=3300, pmatch=0.1, dists=NEAR))
                s.next_chunk()
            s.fill_to(CONT_MIN)
            final = s.finish(lits(s.rng, 3))
            cases.append(_case("H hist %d %s %s" % (hl, reach, variant), "H", variant, s, final, hist=hist, meta={"reach": reach}))
    # the piece ends inside a block: the complete blocks by the pieces, the rest by the serial path
    s = Stream(89)
    hist = s.noise(WIN)
    s.add(mixed(0))
    s.next_chunk()
    _extras(s, 6)
    last = mixed(3)
    cut = len(s.raw) + len(last.raw) // 2
    s.add(last)
    final = s.finish(lits(s.rng, 3))
    cases.append(_case("H cut inside a block", "H", "chain", s, final, hist=hist, cut=cut))
    return cases


COUNTS = {"W": 2, "S": 7, "R": 10, "G": 5, "F": 11, "X": 3, "C": 25, "H": 13}  # cases per family: what the tests are parametrised by
FAMILIES = {"W": family_w, "S": family_s, "R": family_r, "G": family_g, "F": family_f, "X": family_x, "C": family_c, "H": family_h}


@functools.lru_cache(None)
def family(name):
    return FAMILIES[name]()


def piece_fronts(case, fmt="de"):
    """the output in front of every predicted piece (of those that are block starts and lie in the stream), and the total"""
    at = dict(case.starts)
    final = case.meta["final"] if case.meta["cut"] is None else 8 * case.meta["cut"]
    return [at[q] for q in case.meta["predicted"][fmt] if q in at and q <= final] + [case.meta["total"]]


def all_cases():
    return [c for f in FAMILIES for c in family(f)]
