"""LZO1X written instruction by instruction (test infrastructure, the LZO counterpart of tests/deflate_writer.py).

A compressor uses a narrow part of the format; this writer places any instruction anywhere and knows what the decoder
has to make of it.  Instructions:

    ("first", n)            the first-byte literal form, byte 17 + n and n literals (1 <= n <= 238); first only
    ("run", n[, data])      n >= 4 literals: one byte up to 18, two bytes up to 273, zero-byte continuation above
    ("M1", off, 2, lit)     two bytes, a match of 2 at off <= 1024
    ("M2", off, mlen, lit)  two bytes, mlen 3..8, off <= 2048
    ("M3", off, mlen, lit)  off <= 16 384; one opcode byte up to mlen 33, a length byte up to 288, zero bytes above
    ("M4", off, mlen, lit)  off 16 385 .. 49 151; one opcode byte up to mlen 9, a length byte up to 264, zero bytes above
    ("end",)                the end marker 17 0 0
    ("raw", bytes)          bytes as they are: malformed instructions (what follows has no expected output)

lit (0..3) literals follow a match.  The decoder's state decides what an opcode below 16 is (lib/lzo.ml:322-336 as
restated in oracle/lzo.c): zero after a match without literals and after the first-byte run - then it is a run of
literals; not zero after a run and after a match with 1..3 literals - then it is the two-byte match M1.  The writer
tracks that state, asserts that each instruction can be written where it stands and that its offset reaches no further
back than the output so far, and replays the copies byte by byte for the expected output.  liblzo reads an opcode below
16 right after a literal RUN (the first-byte one included) as a match of its own: `liblzo_compatible` says whether a
stream avoids that."""
import collections

M1_MAX_OFF, M2_MAX_OFF, M3_MAX_OFF, M4_MAX_OFF = 1024, 2048, 16384, 49151
M3_SHORT, M3_BYTE = 33, 33 + 255   # longest match with one opcode byte / with a length byte
M4_SHORT, M4_BYTE = 9, 9 + 255
RUN_SHORT, RUN_BYTE = 18, 18 + 255
FIRST_MAX = 238

# one written instruction: where it starts in the stream and in the output, its opcode bytes (k), what it does, the
# decoder's state in front of it, and whether its length goes on over zero bytes
Rec = collections.namedtuple("Rec", "idx form ipos opos k off mlen lit zero cont")


def _count(n):
    """a length that goes on: zero bytes of 255 each, then 1..255"""
    assert n >= 1
    z = (n - 1) // 255
    return bytes(z) + bytes([n - 255 * z])


def encode(form, off, mlen, lit):
    """the opcode bytes of a match (no checks against the output: `raw` places what this returns)"""
    assert 0 <= lit <= 3
    if form == "M1":
        assert mlen == 2 and 1 <= off <= M1_MAX_OFF
        return bytes([(((off - 1) & 3) << 2) | lit, (off - 1) >> 2])
    if form == "M2":
        assert 3 <= mlen <= 8 and 1 <= off <= M2_MAX_OFF
        return bytes([((mlen - 1) << 5) | (((off - 1) & 7) << 2) | lit, (off - 1) >> 3])
    if form == "M3":
        assert mlen >= 3 and 1 <= off <= M3_MAX_OFF
        head = bytes([32 | (mlen - 2)]) if mlen <= M3_SHORT else bytes([32]) + _count(mlen - M3_SHORT)
        s = ((off - 1) << 2) | lit
    else:
        assert form == "M4" and mlen >= 3 and M3_MAX_OFF < off <= M4_MAX_OFF
        d = off - 16384
        top = 16 | ((d >> 11) & 8)
        head = bytes([top | (mlen - 2)]) if mlen <= M4_SHORT else bytes([top]) + _count(mlen - M4_SHORT)
        s = ((d & 0x3fff) << 2) | lit
    return head + bytes([s & 0xff, s >> 8])


def form_for(off, mlen):
    """the shortest form that holds the match"""
    if mlen == 2:
        return "M1"
    if mlen <= 8 and off <= M2_MAX_OFF:
        return "M2"
    return "M3" if off <= M3_MAX_OFF else "M4"


class Writer:
    """an LZO1X stream under construction: .stream, .out (the expected output), .recs, .zero (the decoder's state)"""

    def __init__(self, rng):
        self.rng = rng
        self.stream, self.out, self.recs = bytearray(), bytearray(), []
        self.zero = True       # the state in front of the next instruction is zero
        self.ended = self.malformed = self.compatible_break = False

    ipos = property(lambda self: len(self.stream))
    opos = property(lambda self: len(self.out))

    def _lits(self, n, data=None):
        data = bytes(self.rng.getrandbits(8) for _ in range(n)) if data is None else bytes(data)
        assert len(data) == n
        self.stream += data
        self.out += data

    def add(self, ins):
        assert not self.ended, "instruction behind the end marker"
        form, ipos, opos, zero = ins[0], self.ipos, self.opos, self.zero
        off = mlen = lit = 0
        cont = False
        if form == "raw":
            self.stream += bytes(ins[1])
            self.malformed = True
            k = len(ins[1])
        elif self.malformed:
            raise AssertionError("only raw bytes may follow raw bytes")
        elif form == "first":
            lit = ins[1]
            assert ipos == 0 and 1 <= lit <= FIRST_MAX
            self.stream.append(17 + lit)
            self._lits(lit)
            k, self.zero = 1, True
        elif form == "run":
            lit = ins[1]
            assert zero and lit >= 4, "a run of literals needs 4 bytes and the state zero"
            if self.recs and self.recs[-1].form == "first":  # (liblzo: a match, its state there is not zero)
                self.compatible_break = True
            op = bytes([lit - 3]) if lit <= RUN_SHORT else bytes([0]) + _count(lit - RUN_SHORT)
            cont = lit > RUN_BYTE
            self.stream += op
            self._lits(lit, ins[2] if len(ins) > 2 else None)
            k, self.zero = len(op), False
        elif form == "end":
            self.stream += bytes([17, 0, 0])
            k, self.ended = 3, True
        else:
            _, off, mlen, lit = ins
            assert form != "M1" or not zero, "M1 needs a state that is not zero"
            assert off <= opos, "offset beyond the output so far"
            if form == "M1" and self.recs and self.recs[-1].form == "run":
                self.compatible_break = True
            op = encode(form, off, mlen, lit)
            cont = (form == "M3" and mlen > M3_BYTE) or (form == "M4" and mlen > M4_BYTE)
            self.stream += op
            src = opos - off
            if off >= mlen:
                self.out += self.out[src:src + mlen]
            else:
                for j in range(mlen):
                    self.out.append(self.out[src + j])
            self._lits(lit)
            k, self.zero = len(op), lit == 0
        rec = Rec(len(self.recs), form, ipos, opos, k, off, mlen, lit, zero, cont)
        self.recs.append(rec)
        return rec

    def extend(self, ins):
        for i in ins:
            self.add(i)
        return self

    @property
    def liblzo_compatible(self):
        """valid, and no opcode below 16 right after a literal run (oracle/lzo.c's header: liblzo reads that one differently)"""
        return self.ended and not self.malformed and not self.compatible_break

    def counts(self):
        """bookkeeping: what kinds of instruction this stream sends through a decoder"""
        c = collections.Counter()
        for r in self.recs:
            c[r.form] += 1
            c["mlen288"] += r.mlen == M3_BYTE
            c["off49151"] += r.off == M4_MAX_OFF and r.mlen > 0
            c["low_opcode_run"] += r.form == "run" and r.k == 1 and r.lit <= 18
        return c


def write(ins, rng):
    """instructions -> (stream, expected output); the expected output is None when raw bytes are among them"""
    w = Writer(rng).extend(ins)
    return bytes(w.stream), None if w.malformed else bytes(w.out)


# the lengths where an opcode grows and the offsets where the form changes
M3_EDGES = (3, 33, 34, M3_BYTE, M3_BYTE + 1, M3_BYTE + 255, M3_BYTE + 256, 900)
M4_EDGES = (3, 9, 10, M4_BYTE, M4_BYTE + 1, M4_BYTE + 255, M4_BYTE + 256)
RUN_EDGES = (4, 18, 19, RUN_BYTE, RUN_BYTE + 1, RUN_BYTE + 255, RUN_BYTE + 256)
OFF_EDGES = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 16383, 16384, 16385, 32767, 32768, 49150, 49151)


def random_instructions(rng, compatible):
    """a valid instruction list over every form, the lengths where an opcode grows and the offsets where the form changes;
    compatible: nothing that liblzo reads differently (an opcode below 16 right behind a literal run)"""
    w = Writer(rng)
    ins = []

    def add(i):
        ins.append(i)
        return w.add(i)

    start = rng.random()
    if start < 0.4:
        add(("first", rng.choice((1, 2, 3, 4, 237, 238, rng.randrange(1, 239)))))
    elif start < 0.9:
        add(("run", rng.choice(RUN_EDGES + (50000,) * 3)))
    else:
        add(("first", 238))
        if not compatible:
            add(("run", rng.choice(RUN_EDGES)))
    for _ in range(rng.randrange(0, 120)):
        after_run = w.recs[-1].form in ("run", "first")
        forms = ["M2", "M3", "M3"] + (["M4"] if w.opos > 16384 else [])
        if w.zero and not (compatible and after_run):
            forms += ["run", "run"]
        if not w.zero and not (compatible and after_run):
            forms += ["M1", "M1"]
        f, lit = rng.choice(forms), rng.randrange(4)
        offs = [o for o in OFF_EDGES if o <= w.opos] + [rng.randrange(1, w.opos + 1)] * 3 + [w.opos]
        if f == "run":
            add(("run", rng.choice(RUN_EDGES + (rng.randrange(4, 40),) * 6)))
        elif f == "M1":
            add((f, rng.choice([o for o in offs if o <= 1024]), 2, lit))
        elif f == "M2":
            add((f, rng.choice([o for o in offs if o <= 2048]), rng.randrange(3, 9), lit))
        elif f == "M3":
            add((f, rng.choice([o for o in offs if o <= 16384]), rng.choice(M3_EDGES + (rng.randrange(3, 300),) * 4), lit))
        else:
            add((f, rng.choice([o for o in offs if 16384 < o <= M4_MAX_OFF]), rng.choice(M4_EDGES + (rng.randrange(3, 300),) * 4), lit))
    add(("end",))
    assert w.liblzo_compatible or not compatible
    return ins, w
