"""A plain reader of a raw deflate stream with De.Inf.Ns's rules (lib/de.ml:1534-1823), the slow way: bits one at a
time, codes matched against the canonical (length, code) list, no tables.  It is the second opinion next to the CPU
oracle (oracle/de_inflate.c) for hand-built dynamic headers, and it says WHICH rule a header fails.

    r = inflate(raw, cap)            # r.status, r.consumed, r.output as the oracle; r.tag; r.info

The order of checks is the reference's (lib/de.ml:1718-1793) with the three documented divergences (DESIGN.md 2,
head of oracle/de_inflate.c): D1 bits the input does not hold are Unexpected_end_of_input; D2 the empty distance
table's other slot is Invalid_distance_code; D3 a table that needs more than 852 / 592 entries is Invalid_dictionary.
The need is computed here from the sorted lengths by zlib's rule (inftrees.c: a sub-table is as wide as the codes that
remain let it be filled), not by building a table.

r.tag names the rule of the first failing dynamic header, or "ok" for the last one read (None: no dynamic block):
cl_over, cl_incomplete, cl_empty_slot, rep16_first, run_overflow, no_eob, lit_over, lit_incomplete, dist_over,
dist_incomplete, lit_enough, dist_enough, eoi_at:<field> (hlit, cl_lens, cl_sym, rep_extra).  r.info describes that
header: hlit, hdist, hclen, cl_lens, lit_lens, dist_lens, lit_need, dist_need, start / end (bit positions), incomplete,
slots (how often its block read an unused slot of a one-code table), empty_reads (how often it read the empty distance
table); r.headers lists every dynamic header's.

`defects` switches on named mistakes (DEFECTS): the corpus tests use them to show that some stream tells each apart."""
from collections import namedtuple

from tests.deflate_tokens import DB, DX, LB, LX

OK, END_OF_INPUT, END_OF_OUTPUT, INVALID_KIND, INVALID_DICTIONARY, INVALID_COMPLEMENT = 0, 1, 2, 3, 4, 5
INVALID_DISTANCE, INVALID_DISTANCE_CODE = 6, 7
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LIT_ENOUGH, DIST_ENOUGH = 852, 592
DEFECTS = {
    "dist_limit_594": "the distance table may need 594 entries",
    "lit_limit_856": "the literal/length table may need 856 entries",
    "no_rep16_first": "a 16 as the first symbol repeats a zero",
    "rep16_last_nonzero": "a 16 after a 17 / 18 repeats the last non-zero length",
    "run_overshoot_ge": "a run that ends exactly at hlit + hdist is refused",
    "no_eob_late": "the end-of-block length is looked at after the table verdicts",
    "lone_cl_code": "a lone 1-bit code-length code is accepted",
    "lone_dist_any_length": "an incomplete code is accepted when the distance alphabet has one code of any length",
    "slot_eats_bit": "the unused slot of a one-code table consumes one bit",
    "d2_dictionary": "the empty distance table's other slot is Invalid_dictionary",
}

Result = namedtuple("Result", "status consumed output tag info headers")


class _Stop(Exception):
    def __init__(self, status, tag=None):
        self.status, self.tag = status, tag


def kraft(lens):
    """(over-subscribed, leaves left over at 15 bits) of a list of code lengths"""
    left = 1
    for l in range(1, 16):
        left = left * 2 - sum(1 for x in lens if x == l)
        if left < 0:
            return True, 0
    return False, left


def table_shape(lens, rootpref):
    """(root width, widths of the sub-tables) of zlib's two-level table for these code lengths (inftrees.c), from the
    sorted lengths alone: walking the codes longer than the root in canonical order, every new root prefix opens a
    sub-table of 2^curr entries, curr = the code's length - root, widened while the codes that remain (this one
    included) of the lengths up to root + curr do not fill it."""
    ls = sorted(l for l in lens if l)
    if not ls:
        return 0, []
    root = min(max(rootpref, ls[0]), ls[-1])
    widths, code, prev_len, prefix = [], 0, ls[0], None
    for k, l in enumerate(ls):
        code <<= l - prev_len
        prev_len = l
        if l > root and code >> (l - root) != prefix:
            prefix = code >> (l - root)
            curr = l - root
            left = 1 << curr
            while curr + root < ls[-1]:
                left -= sum(1 for x in ls[k:] if x == curr + root)
                if left <= 0:
                    break
                curr += 1
                left <<= 1
            widths.append(curr)
        code += 1
    return root, widths


def table_need(lens, rootpref):
    """entries that table needs: 2^root and 2^width for every sub-table"""
    root, widths = table_shape(lens, rootpref)
    return (1 << root) + sum(1 << w for w in widths)


def canonical_list(lens):
    """{(length, code): symbol} of the canonical code (RFC 1951 3.2.2)"""
    out, code = {}, 0
    for l in range(1, 16):
        code <<= 1
        for s, x in enumerate(lens):
            if x == l:
                out[(l, code)] = s
                code += 1
    return out


class _Reader:
    def __init__(self, raw, cap, defects):
        self.raw, self.cap, self.defects = raw, cap, frozenset(defects)
        assert self.defects <= set(DEFECTS)
        self.pos, self.total, self.out = 0, 8 * len(raw), bytearray()
        self.tag, self.info, self.headers = None, None, []

    def left(self):
        return self.total - self.pos

    def peekbit(self, k=0):
        p = self.pos + k
        return (self.raw[p >> 3] >> (p & 7)) & 1 if p < self.total else 0  # (bits behind the input read as zero)

    def bits(self, n, field=None):
        if self.left() < n:
            raise _Stop(END_OF_INPUT, "eoi_at:" + field if field else None)  # D1
        v = 0
        for k in range(n):
            v |= self.peekbit(k) << k
        self.pos += n
        return v

    def symbol(self, codes, longest):
        """the next code of `codes`, a bit at a time.  Where no code matches (an incomplete code's unused slot) the
        reference's zero table entry answers: symbol 0, no bits (lib/de.ml:521)."""
        acc = 0
        for l in range(1, longest + 1):
            acc = acc << 1 | self.peekbit(l - 1)
            if (l, acc) in codes:
                if self.left() < l:
                    raise _Stop(END_OF_INPUT)  # D1
                self.pos += l
                return codes[(l, acc)]
        if "slot_eats_bit" in self.defects:
            self.bits(1)
        if self.info is not None:
            self.info["slots"] += 1
        return 0

    # ---- a dynamic header, lib/de.ml:1733-1793 ----
    def header(self):
        d = self.defects
        info = self.info = {"start": self.pos - 3, "slots": 0, "empty_reads": 0}
        self.headers.append(info)
        self.tag = "ok"
        if self.left() < 14:
            raise _Stop(END_OF_INPUT, "eoi_at:hlit")
        hlit, hdist, hclen = self.bits(5) + 257, self.bits(5) + 1, self.bits(4) + 4
        info.update(hlit=hlit, hdist=hdist, hclen=hclen)
        cl = [0] * 19
        for i in range(hclen):
            cl[CL_ORDER[i]] = self.bits(3, "cl_lens")
        info["cl_lens"] = cl
        if any(cl):
            over, left = kraft(cl)
            if over:
                raise _Stop(INVALID_DICTIONARY, "cl_over")
            if left and not ("lone_cl_code" in d and sorted(cl)[-2:] == [0, 1]):
                raise _Stop(INVALID_DICTIONARY, "cl_incomplete")  # a lone code too: unlike the other two alphabets
            codes, cmax = canonical_list(cl), max(cl)
        else:
            codes, cmax = None, 1  # empty_table: symbol 0 on the bit 0, the other slot is outside the table
        n, lens, last_nonzero = hlit + hdist, [], 0
        while len(lens) < n:
            if self.left() < cmax:  # the reference fills up to the longest code before it looks
                raise _Stop(END_OF_INPUT, "eoi_at:cl_sym")
            if codes is None:
                if self.bits(1):
                    raise _Stop(INVALID_DICTIONARY, "cl_empty_slot")
                sym = 0
            else:
                sym = self.symbol(codes, cmax)
            if sym < 16:
                lens.append(sym)
                last_nonzero = sym or last_nonzero
                continue
            if sym == 16:
                if not lens and "no_rep16_first" not in d:
                    raise _Stop(INVALID_DICTIONARY, "rep16_first")
                copy, val = self.bits(2, "rep_extra") + 3, lens[-1] if lens else 0
                if "rep16_last_nonzero" in d:
                    val = last_nonzero
            elif sym == 17:
                copy, val = self.bits(3, "rep_extra") + 3, 0
            else:
                copy, val = self.bits(7, "rep_extra") + 11, 0
            if len(lens) + copy > n or ("run_overshoot_ge" in d and len(lens) + copy >= n):
                raise _Stop(INVALID_DICTIONARY, "run_overflow")
            lens += [val] * copy
        lit, dist = lens[:hlit], lens[hlit:]
        info.update(lit_lens=lit, dist_lens=dist, end=self.pos, lit_need=table_need(lit, 9), dist_need=table_need(dist, 6))
        if lit[256] == 0 and "no_eob_late" not in d:
            raise _Stop(INVALID_DICTIONARY, "no_eob")
        lone_ok = "lone_dist_any_length" in d and sum(1 for l in dist if l) == 1
        inc = False
        for name, ls, limit in (("lit", lit, LIT_ENOUGH + (4 if "lit_limit_856" in d else 0)),
                                ("dist", dist, DIST_ENOUGH + (2 if "dist_limit_594" in d else 0))):
            if not any(ls):
                continue  # empty_table (only the distance alphabet gets here: lit[256] is not 0)
            over, left = kraft(ls)
            if over:
                raise _Stop(INVALID_DICTIONARY, name + "_over")
            if left and max(ls) != 1 and not lone_ok:  # lib/de.ml:549-550: a lone 1-bit code is let through
                raise _Stop(INVALID_DICTIONARY, name + "_incomplete")
            inc = inc or left > 0
            if info[name + "_need"] > limit:
                raise _Stop(INVALID_DICTIONARY, name + "_enough")  # D3
        if lit[256] == 0:
            raise _Stop(INVALID_DICTIONARY, "no_eob")
        info["incomplete"] = inc
        return lit, dist

    # ---- a Huffman block's tokens, lib/de.ml:1667-1712 ----
    def block(self, lit, dist):
        lc = canonical_list(lit)
        dc = canonical_list(dist) if any(dist) else None
        out, cap = self.out, self.cap
        lmax, dmax = max(lit), max(dist)
        while True:
            sym = self.symbol(lc, lmax)
            if sym < 256:
                if len(out) >= cap:
                    raise _Stop(END_OF_OUTPUT)
                out.append(sym)
                continue
            if sym == 256:
                return
            i = sym - 257
            length = (LB[i] if i < 28 else 258 if i == 28 else 3) + self.bits(LX[i] if i < 28 else 0)
            if dc is None:  # empty_table (D2): one entry, symbol 0 on one bit; the bit 1 indexes outside it
                if self.info is not None:
                    self.info["empty_reads"] += 1
                if self.peekbit():
                    raise _Stop(INVALID_DICTIONARY if "d2_dictionary" in self.defects else INVALID_DISTANCE_CODE)
                self.bits(1)
                ds = 0
            else:
                ds = self.symbol(dc, dmax)
            if ds >= 30:
                raise _Stop(INVALID_DISTANCE_CODE)
            dd = DB[ds] + self.bits(DX[ds])
            if dd > min(len(out), 32768):
                raise _Stop(INVALID_DISTANCE)
            if length > cap - len(out):
                raise _Stop(END_OF_OUTPUT)
            for _ in range(length):
                out.append(out[-dd])

    def stored(self):
        self.pos = (self.pos + 7) & ~7
        if self.left() < 32:
            raise _Stop(END_OF_INPUT)
        n, c = self.bits(16), self.bits(16)
        if c != 0xffff - n:
            raise _Stop(INVALID_COMPLEMENT)
        if 8 * n > self.left():
            raise _Stop(END_OF_INPUT)
        if n > self.cap - len(self.out):
            raise _Stop(END_OF_OUTPUT)
        self.out += self.raw[self.pos >> 3:(self.pos >> 3) + n]
        self.pos += 8 * n

    def run(self):
        while True:
            if self.left() < 3:
                raise _Stop(END_OF_INPUT)
            last, kind = self.bits(1), self.bits(2)
            if kind == 0:
                self.stored()
            elif kind == 1:
                self.block([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32)
            elif kind == 2:
                self.block(*self.header())
            else:
                raise _Stop(INVALID_KIND)
            if last:
                return


def inflate(raw, cap, defects=()):
    r = _Reader(bytes(raw), cap, defects)
    try:
        r.run()
    except _Stop as e:
        if e.tag is not None:
            r.tag = e.tag
        return Result(e.status, 0, bytes(r.out), r.tag, r.info, r.headers)
    return Result(OK, (r.pos + 7) >> 3, bytes(r.out), r.tag, r.info, r.headers)
