"""Token-level RFC 1951 writer for tests: the stream is exactly the blocks and tokens the caller lists, so a test can
put a match, a block end or an invalid symbol where a kernel's round limits are.

    blocks = [Block("stored", b"abc"), Block("dynamic", [97, 98, (3, 2), match(258, 1, lsym=284)])]
    raw = write(blocks)                       # the raw deflate stream
    status, out = expand(blocks, cap)         # what a decoder must produce (the plain reference)

A token is a literal (0..255), a match `(length, distance)`, or a `Match` from `match()`, which can also choose how it
is coded: 258 as symbol 284 with extra 31, the symbols 286/287, the distance codes 30/31.  End-of-block is written at the
end of every Huffman block (unless the block or the call says eob=False).  A dynamic block's header can be spelled out
too: the code-length code's lengths (cl_lens), how many of them are sent (hclen) and the exact run-length symbols
(cl_syms), valid or not; `Bits(value, nbits)` in a token list (or in cl_syms) writes raw bits, e.g. the unused slot of a
one-code table.  expand() refuses such blocks: what they decode to is for tests/deflate_header_model.py to say.  `expand` replays the tokens byte by byte with forward-copy overlap and stops in front of the
first token that fails (the statuses of include/mdeflate.h): a literal or a whole match that does not fit `cap`, a
distance beyond the output written so far or beyond 32 KiB, a distance code 30/31.  Everything before it is written."""
from collections import namedtuple

from tests.deflate_tokens import DB, DX, LB, LX

OK, END_OF_OUTPUT, INVALID_DISTANCE, INVALID_DISTANCE_CODE = 0, 2, 6, 7
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32

# lsym / dsym: the symbol to code (None: the usual one); lext / dext: the value of its extra bits (None: what the
# length / distance needs).  Symbols 286/287 carry no extra bits; distance codes 30/31 carry none either.
Match = namedtuple("Match", "length dist lsym lext dsym dext")
Bits = namedtuple("Bits", "value nbits")  # raw bits in a block's token stream, least significant first


def match(length, dist, lsym=None, lext=None, dsym=None, dext=None):
    return Match(length, dist, lsym, lext, dsym, dext)


class Block:
    """kind: "stored", "fixed" or "dynamic".  Dynamic blocks: lit_lens / dist_lens give the code lengths (otherwise
    length-limited ones are built from the token counts), hlit / hdist send more lengths than the code needs (the extra
    ones are 0 unless lit_lens / dist_lens say otherwise), and `extra` lists symbols (286, 287, 1030 + d for distance
    code d) that get a code although no token uses them.  last: None = only the last block of the list.
    Header spelled out (all optional, the stream is byte-identical without them): cl_lens = the 19 code-length code
    lengths as given (incomplete, over-subscribed, all zero, one code); hclen = how many 3-bit fields are sent (4..19;
    the lengths behind it must be 0); cl_syms = the exact `(symbol, extra value)` sequence (or `Bits`) that codes the
    lengths, instead of the run-length coder - hlit and hdist are then sent exactly as given, and lit_lens / dist_lens
    (what the sequence decodes to) only code the body.  Every symbol of cl_syms must have a code in cl_lens unless
    cl_check=False (a symbol without one then writes its extra bits only).  eob: False leaves out the end-of-block code."""

    def __init__(self, kind, tokens=(), lit_lens=None, dist_lens=None, hlit=None, hdist=None, extra=(), last=None,
                 cl_lens=None, hclen=None, cl_syms=None, cl_check=True, eob=None):
        assert kind in ("stored", "fixed", "dynamic")
        self.kind, self.tokens = kind, list(tokens)
        self.lit_lens, self.dist_lens, self.hlit, self.hdist = lit_lens, dist_lens, hlit, hdist
        self.extra, self.last = tuple(extra), last
        self.cl_lens, self.hclen, self.cl_syms, self.cl_check, self.eob = cl_lens, hclen, cl_syms, cl_check, eob
        if cl_syms is not None:
            assert hlit is not None and hdist is not None and lit_lens is not None and dist_lens is not None
        if kind == "stored":
            assert all(isinstance(t, int) for t in self.tokens) and len(self.tokens) <= 65535


def _norm(t):
    if isinstance(t, int):
        return t
    if isinstance(t, (Match, Bits)):
        return t
    return Match(t[0], t[1], None, None, None, None)


def length_code(length, lsym=None, lext=None):
    """(symbol, extra value, extra bits) of a match length"""
    if lsym is None:
        lsym = 285 if length == 258 else 257 + max(i for i in range(28) if LB[i] <= length)
    i = lsym - 257
    nb = LX[i] if i < 29 else 0
    if lext is None:
        lext = length - LB[i] if i < 29 else 0
    assert 0 <= lext < (1 << nb) or (nb == 0 and lext == 0), (length, lsym, lext)
    return lsym, lext, nb


def dist_code(dist, dsym=None, dext=None):
    if dsym is None:
        dsym = max(i for i in range(30) if DB[i] <= dist)
    nb = DX[dsym] if dsym < 30 else 0
    if dext is None:
        dext = dist - DB[dsym] if dsym < 30 else 0
    assert 0 <= dext < (1 << nb) or (nb == 0 and dext == 0), (dist, dsym, dext)
    return dsym, dext, nb


def limited_lengths(freqs, maxbits):
    """length-limited Huffman code lengths (package-merge); a lone used symbol gets length 1"""
    used = sorted((f, s) for s, f in enumerate(freqs) if f > 0)
    lens = [0] * len(freqs)
    if len(used) == 1:
        lens[used[0][1]] = 1
    if len(used) <= 1:
        return lens
    assert len(used) <= (1 << maxbits)
    leaves = [(f, (s,)) for f, s in used]
    cur = leaves
    for _ in range(maxbits - 1):
        pk = [(cur[i][0] + cur[i + 1][0], cur[i][1] + cur[i + 1][1]) for i in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + pk, key=lambda x: x[0])
    for _, ss in cur[:2 * len(used) - 2]:
        for s in ss:
            lens[s] += 1
    return lens


def canonical(lens):
    """symbol -> (code, length) of the canonical code (RFC 1951 3.2.2)"""
    bl = [0] * 16
    for l in lens:
        bl[l] += 1
    bl[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.buf = 0, 0, bytearray()

    def bits(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def huff(self, code_len):
        code, n = code_len
        self.bits(int(format(code, "0%db" % n)[::-1], 2), n)  # Huffman codes go most significant bit first

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n else b"")


def _rle(lens):
    """code-length symbols (sym, extra value, extra bits) for a list of lengths: 16 / 17 / 18 for runs"""
    out, i = [], 0
    while i < len(lens):
        l, j = lens[i], i
        while j < len(lens) and lens[j] == l:
            j += 1
        run = j - i
        if l == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11, 7))
                run -= k
            if run >= 3:
                out.append((17, run - 3, 3))
                run = 0
            out += [(0, 0, 0)] * run
        else:
            out.append((l, 0, 0))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3, 2))
                run -= k
            out += [(l, 0, 0)] * run
        i = j
    return out


def _tables(b, toks):
    """lit/len and distance code lengths of a dynamic block"""
    lf, df = [0] * 288, [0] * 32
    lf[256] = 1
    for t in toks:
        if isinstance(t, int):
            lf[t] += 1
        elif not isinstance(t, Bits):
            ls, _, _ = length_code(t.length, t.lsym, t.lext)
            ds, _, _ = dist_code(t.dist, t.dsym, t.dext)
            lf[ls] += 1
            df[ds] += 1
    for s in b.extra:
        if s >= 1000:
            df[s - 1000] += 1
        else:
            lf[s] += 1
    if sum(1 for f in lf if f) == 1:  # only the end-of-block code: a second one makes the code complete
        lf[0] = 1
    if sum(1 for f in df if f) < 2:  # no or one distance code: two 1-bit codes (zlib does the same)
        a = next((i for i, f in enumerate(df) if f), 0)
        df[a] = max(df[a], 1)
        df[1 if a == 0 else 0] = 1
    lit = b.lit_lens if b.lit_lens is not None else limited_lengths(lf, 15)
    dist = b.dist_lens if b.dist_lens is not None else limited_lengths(df, 15)
    return list(lit), list(dist)


def _write_dynamic_header(w, lit, dist, hlit, hdist, b=None):
    if b is not None and b.cl_syms is not None:  # the header spelled out: nothing is derived from the lengths
        assert 257 <= hlit <= 288 and 1 <= hdist <= 32
        syms = [s if isinstance(s, Bits) else (s[0], s[1], {16: 2, 17: 3, 18: 7}.get(s[0], 0)) for s in b.cl_syms]
    else:
        hlit = max(hlit or 0, 257, max((i + 1 for i, l in enumerate(lit) if l), default=257))
        hdist = max(hdist or 0, 1, max((i + 1 for i, l in enumerate(dist) if l), default=1))
        assert hlit <= 288 and hdist <= 32
        lit = (lit + [0] * 288)[:hlit]
        dist = (dist + [0] * 32)[:hdist]
        syms = _rle(lit + dist)
    if b is not None and b.cl_lens is not None:
        cl = list(b.cl_lens)
        assert len(cl) == 19 and all(0 <= l <= 7 for l in cl)
        if b.cl_check:
            assert all(cl[s[0]] for s in syms if not isinstance(s, Bits)), "a symbol of the header has no code"
    else:
        cf = [0] * 19
        for s in syms:
            if not isinstance(s, Bits):
                cf[s[0]] += 1
        cl = limited_lengths(cf, 7)
        if sum(1 for l in cl if l) == 1:  # a one-symbol code-length code: complete it
            cl[next(i for i in range(19) if cl[i] == 0)] = 1
    hclen = max(4, max((i + 1 for i, s in enumerate(CL_ORDER) if cl[s]), default=4))
    if b is not None and b.hclen is not None:
        assert 4 <= b.hclen <= 19 and not any(cl[CL_ORDER[i]] for i in range(b.hclen, 19))
        hclen = b.hclen
    w.bits(hlit - 257, 5)
    w.bits(hdist - 1, 5)
    w.bits(hclen - 4, 4)
    for i in range(hclen):
        w.bits(cl[CL_ORDER[i]], 3)
    cc = canonical(cl)
    for s in syms:
        if isinstance(s, Bits):
            w.bits(s.value, s.nbits)
            continue
        if s[0] in cc:
            w.huff(cc[s[0]])
        w.bits(s[1], s[2])


def write(blocks, eob=True, starts=None):
    """the raw deflate stream of `blocks`; eob=False: no end-of-block codes (a block's own `eob` overrides it);
    starts: a list that receives the bit position of every block's header"""
    w = BitWriter()
    for k, b in enumerate(blocks):
        last = b.last if b.last is not None else k == len(blocks) - 1
        if starts is not None:
            starts.append(8 * len(w.buf) + w.n)
        toks = [_norm(t) for t in b.tokens]
        w.bits(1 if last else 0, 1)
        if b.kind == "stored":
            w.bits(0, 2)
            w.align()
            n = len(toks)
            w.bits(n, 16)
            w.bits(n ^ 0xffff, 16)
            for t in toks:
                w.bits(t, 8)
            continue
        if b.kind == "fixed":
            w.bits(1, 2)
            lit, dist = FIXED_LIT, FIXED_DIST
        else:
            w.bits(2, 2)
            lit, dist = _tables(b, toks)
            _write_dynamic_header(w, lit, dist, b.hlit, b.hdist, b)
        lc, dc = canonical(lit), canonical(dist)
        for t in toks:
            if isinstance(t, int):
                w.huff(lc[t])
                continue
            if isinstance(t, Bits):
                w.bits(t.value, t.nbits)
                continue
            ls, lv, ln = length_code(t.length, t.lsym, t.lext)
            ds, dv, dn = dist_code(t.dist, t.dsym, t.dext)
            w.huff(lc[ls])
            w.bits(lv, ln)
            w.huff(dc[ds])
            w.bits(dv, dn)
        if eob if b.eob is None else b.eob:
            w.huff(lc[256])
    return w.getvalue()


def expand(blocks, cap=1 << 62):
    """(status, output) of decoding `blocks` into a buffer of `cap` bytes: the tokens replayed byte by byte"""
    out = bytearray()
    for b in blocks:
        toks = b.tokens if b.kind == "stored" else [_norm(t) for t in b.tokens]  # (a stored block's are bytes: Block checks)
        assert b.cl_lens is None and b.hclen is None and b.cl_syms is None and b.eob is None, "a spelled-out header"
        assert b.kind == "stored" or not any(isinstance(t, Bits) for t in toks), "raw bits: expand() cannot say what they decode to"
        if b.kind == "stored":
            if len(toks) > cap - len(out):
                return END_OF_OUTPUT, bytes(out)
            out += bytes(toks)
            continue
        for t in toks:
            if isinstance(t, int):
                if len(out) >= cap:
                    return END_OF_OUTPUT, bytes(out)
                out.append(t)
                continue
            if t.dsym is not None and t.dsym >= 30:
                return INVALID_DISTANCE_CODE, bytes(out)
            if t.dist > min(len(out), 32768):
                return INVALID_DISTANCE, bytes(out)
            if t.length > cap - len(out):
                return END_OF_OUTPUT, bytes(out)
            s = len(out) - t.dist
            for j in range(t.length):
                out.append(out[s + j])
    return OK, bytes(out)
