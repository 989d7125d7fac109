"""Hand-built LZO1X streams at the limits of the batched decoder (csrc/lzo_kernels.hip), shared by tests/test_lzo_writer.py
(the CPU side: every family's claimed geometry) and tests/test_gpu_lzo_batches.py (the GPU side).  Test infrastructure.

The decoder takes a batch of up to kWindows windows of 64 input bytes; a batch produces at most kBatchMax bytes and ends
in front of an instruction the fast path does not take (a length that goes on over zero bytes, the end marker, M3 at
offset 16 384, anything near the input's end or that would fail) - that one is the one-instruction interpreter's.
batches() replays those cut rules, as the kernel's comment states them, over a writer's records.  It is used to BUILD
and DESCRIBE inputs only: what a stream has to decode to comes from the writer's byte-serial replay and the oracle."""
import collections
import functools
import itertools
import os
import random
import re
import zlib

from tests.lzo_writer import M3_BYTE, M3_MAX_OFF, M4_BYTE, M4_MAX_OFF, RUN_BYTE, Writer, encode, form_for

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Geometry = collections.namedtuple("Geometry", "kWave kWindows kInBlk kInRing kStage kBatchMax")
UNCHECKED_FROM = 49152  # from this output position on every offset of the format (<= 49 151) has its bytes behind it


def geometry():
    """the decoder's sizes from its source: a resize keeps the streams at the limits (no match: an error, not a skip)"""
    with open(os.path.join(ROOT, "decompress_amd", "csrc", "lzo_kernels.hip")) as f:
        src = f.read()
    get = lambda k: int(re.search(r"constexpr [^;]*\b%s = (\d+)\b" % k, src).group(1))
    stage = get("kStage")
    return Geometry(get("kWave"), get("kWindows"), get("kInBlk"), get("kInRing"), stage,
                    stage - int(re.search(r"\bkBatchMax = kStage - (\d+);", src).group(1)))


G = geometry()
CHECK_ZONE = 64 + 4 + RUN_BYTE + 1  # a window this close to the input's end tests every instruction against it

# one batch: the output position it starts at, its windows [(base, [records])], its bytes, and what ended it:
# (reason, record, window, lane) with reason "exotic" | "full" | "bad" | "raw", or None (kWindows windows taken)
Batch = collections.namedtuple("Batch", "o0 wins osum stop")


def exotic(r):
    return r.cont or r.form == "end" or (r.form == "M3" and r.off == M3_MAX_OFF)


def batches(recs, n, cap, g=G):
    """the batches and slow steps ("slow", record) the decoder makes of a stream of n input bytes with room `cap`"""
    ev, i = [], 1 if recs and recs[0].form == "first" else 0
    while i < len(recs):
        o0, wins, osum, stop = recs[i].opos, [], 0, None
        checked = o0 < UNCHECKED_FROM or cap - o0 < g.kStage
        for w in range(g.kWindows):
            if i >= len(recs):
                break
            base, lanes = recs[i].ipos, []
            near_end = base + CHECK_ZONE > n
            while i < len(recs) and recs[i].ipos - base < 64:
                r = recs[i]
                where = (r, w, r.ipos - base)
                if r.form == "raw":
                    stop = ("raw",) + where
                elif exotic(r) or (near_end and not (r.ipos + r.k < n and r.ipos + r.k + r.lit <= n)):
                    stop = ("exotic",) + where
                elif osum + r.mlen + r.lit > g.kBatchMax:
                    stop = ("full",) + where
                elif checked and (r.mlen + r.lit > cap - r.opos or r.opos > cap):
                    stop = ("bad",) + where
                if stop:
                    break
                lanes.append(r)
                osum += r.mlen + r.lit
                i += 1
            wins.append((base, lanes))
            if stop or not lanes:
                break
        ev.append(Batch(o0, wins, osum, stop))
        if stop and stop[0] != "full":
            if stop[0] == "raw" or stop[0] == "bad" or stop[1].ipos + stop[1].k + stop[1].lit > n:
                return ev  # the interpreter fails there (or the test does not say what raw bytes do)
            ev.append(("slow", recs[i]))
            i += 1
    return ev


def only_batches(ev):
    return [e for e in ev if isinstance(e, Batch)]


class Build(Writer):
    """a writer that knows where the current batch began: sync() places an instruction of the slow path (a match of
    289 and more bytes), the next instruction is lane 0 of window 0 of a new batch"""

    def __init__(self, rng, pre):
        super().__init__(rng)
        self.add(("first", pre) if pre <= 200 else ("run", pre))  # `pre` bytes of output in front of everything
        self.sync()

    def off(self, lo=1, hi=M3_MAX_OFF - 1):
        return self.rng.randrange(lo, min(self.opos, hi) + 1)

    def m(self, off, mlen, lit=0, form=None):
        return self.add((form or form_for(off, mlen), off, mlen, lit))

    def sync(self, lit=0, extra=0):
        r = self.m(self.off(), M3_BYTE + 1 + extra, lit, "M3")
        self.b0, self.o0 = self.ipos, self.opos
        return r

    r = property(lambda self: self.opos - self.o0)  # bytes of the batch so far (while nothing has cut it)

    def fill(self, n):
        """n short matches without literals, two or three opcode bytes each"""
        for _ in range(n):
            if self.rng.random() < 0.6:
                self.m(self.off(hi=2048), self.rng.randrange(3, 9), 0, "M2")
            else:
                self.m(self.off(), self.rng.randrange(3, 34), 0, "M3")

    def pad_in(self, target):
        """two-byte matches (one of three bytes for an odd distance) up to input position `target`; the state ends zero"""
        d = target - self.ipos
        assert d == 0 or d >= 2, d
        if d & 1:
            self.m(self.off(), 3, 0, "M3")
        while self.ipos < target:
            self.m(self.off(hi=2048), 3, 0, "M2")
        assert self.ipos == target

    def place(self, w, lane):
        """right behind sync(): the next instruction is lane `lane` of window w (windows of exactly 64 bytes)"""
        for k in range(1, w + 1):
            if self.b0 + 64 * k > self.ipos:
                self.pad_in(self.b0 + 64 * k)
        self.pad_in(self.b0 + 64 * w + lane)

    def dense(self, count, m4=None):
        """random instructions of every form and every number of literals: the state alternates inside a window"""
        rng = self.rng
        for _ in range(count):
            forms = ["M2", "M2", "M3", "M3"] + (["run"] if self.zero else ["M1", "M1", "M1"])
            if self.opos > M3_MAX_OFF:
                forms += ["M4", "M4"] if m4 is None else ["M4"] * 6
            f, lit = rng.choice(forms), rng.randrange(4)
            if f == "run":
                self.add(("run", rng.randrange(4, 19)))
            elif f == "M1":
                self.m(min(self.opos, rng.choice([1, 2, 1023, 1024, self.off(hi=1024)])), 2, lit, f)
            elif f == "M2":
                self.m(self.off(hi=2048), rng.randrange(3, 9), lit, f)
            elif f == "M3":
                self.m(self.off(), rng.choice([rng.randrange(3, 34), rng.randrange(3, 34), rng.randrange(34, M3_BYTE + 1)]), lit, f)
            else:
                off = m4 if m4 is not None and rng.random() < 0.7 else rng.randrange(M3_MAX_OFF + 1, min(self.opos, M4_MAX_OFF) + 1)
                self.m(off, rng.choice([rng.randrange(3, 10), rng.randrange(10, M4_BYTE + 1)]), lit, f)

    def finish(self, tail=True):
        """the end marker, behind `tail` ordinary instructions long enough to keep what is in front of them away from the
        tests of the input's end (or right away: then the last instructions are inside that zone)"""
        if tail:
            self.tail(CHECK_ZONE)
        self.add(("end",))
        return self

    def tail(self, nbytes):
        t0 = self.ipos
        while self.ipos - t0 < nbytes:
            self.m(self.off(hi=2048), 3, 0, "M2")
            self.add(("run", 18))


# a stream for the decoder: expected bytes (`out`) when the stream is valid, whole, and `cap` holds them - else None
# and the oracle alone says what the status is (the output is then empty)
Case = collections.namedtuple("Case", "name stream cap out b")


def case(name, b, cap=None, cut=None):
    need = len(b.out)
    cap = need if cap is None else cap
    ok = not b.malformed and b.ended and cut is None and cap >= need
    return Case(name, bytes(b.stream) if cut is None else bytes(b.stream[:cut]), cap, bytes(b.out) if ok else None, b)


def _rng(name):
    return random.Random(zlib.crc32(name.encode()))


# ---- A. the two states of the decoder on the fast path ----------------------------------------------------------------
def _a_dense(b):
    b.dense(400)


def _a_m1_after(b):
    """M1 right after a run and after a match with 1, 2 and 3 literals, at its smallest and largest offsets"""
    for off, prev in itertools.product((1, 2, 1023, 1024), ("run", 1, 2, 3)):
        if prev == "run":
            b.m(b.off(hi=2048), 4, 0, "M2")
            b.add(("run", b.rng.randrange(4, 19)))
        else:
            b.m(b.off(hi=2048), 4, prev, "M2")
        b.m(off, 2, b.rng.randrange(4), "M1")


def _a_low_opcodes(b):
    """opcodes 1..15: a run of literals behind a match without literals, next to the same two bytes behind a match with
    one literal, where they are M1"""
    for c in range(1, 16):
        h = b.rng.getrandbits(8)
        b.m(b.off(hi=2048), 3, 0, "M2")
        b.add(("run", c + 3, bytes([h]) + bytes(b.rng.getrandbits(8) for _ in range(c + 2))))
        b.m(b.off(hi=2048), 3, 1, "M2")
        r = b.m((h << 2) + (c >> 2) + 1, 2, c & 3, "M1")
        assert bytes(b.stream[r.ipos:r.ipos + 2]) == bytes([c, h])


def _a_dense32(b):
    """32 two-byte instructions in one window, the first of them M1 / all of them M2"""
    b.sync(lit=1)
    b.m(b.off(hi=1024), 2, 0, "M1")
    for _ in range(31):
        b.m(b.off(hi=2048), 3, 0, "M2")
    b.sync()
    for _ in range(32):
        b.m(b.off(hi=2048), b.rng.randrange(3, 9), 0, "M2")
    b.sync()


A_STREAMS = (("A dense", 17000, _a_dense), ("A M1 after", 1100, _a_m1_after), ("A low opcodes", 1100, _a_low_opcodes),
             ("A dense32", 1100, _a_dense32))


@functools.lru_cache(None)
def family_a():
    cases = []
    for name, pre, fn in A_STREAMS:
        for tail in (True, False):  # the same instructions away from the input's end and next to it
            b = Build(_rng(name), pre)
            fn(b)
            cases.append(case("%s, %s" % (name, "tail" if tail else "no tail"), b.finish(tail)))
    return cases


# ---- B. the edges between the fast path and the interpreter -------------------------------------------------------
def _edges():
    e = []
    for mlen in (33, 34, M3_BYTE, M3_BYTE + 1, M3_BYTE + 255, M3_BYTE + 256):
        e.append(("B M3 length %d" % mlen, 700, lambda b, mlen=mlen: b.m(b.off(), mlen, b.rng.randrange(4), "M3")))
    for mlen in (9, 10, M4_BYTE, M4_BYTE + 1):
        e.append(("B M4 length %d" % mlen, 17000,
                  lambda b, mlen=mlen: b.m(b.rng.randrange(M3_MAX_OFF + 1, b.opos + 1), mlen, b.rng.randrange(4), "M4")))
    for n in (18, 19, RUN_BYTE, RUN_BYTE + 1):
        e.append(("B run %d" % n, 700, lambda b, n=n: b.add(("run", n))))
    for off in (M3_MAX_OFF - 1, M3_MAX_OFF):
        e.append(("B M3 offset %d" % off, off + 300, lambda b, off=off: b.m(off, b.rng.choice((20, 40)), b.rng.randrange(4), "M3")))
    for off in (M3_MAX_OFF + 1, 32767, 32768, M4_MAX_OFF):
        e.append(("B M4 offset %d" % off, off + 300, lambda b, off=off: b.m(off, b.rng.choice((6, 30)), b.rng.randrange(4), "M4")))
    return e


def _edge_stream(b, put):
    """the instruction as the first, a middle and the last one of a batch -> its three records"""
    marks = [put(b)]
    b.fill(8), b.sync(), b.fill(6)
    marks.append(put(b))
    b.fill(6), b.sync(), b.fill(8)
    marks.append(put(b))
    b.sync(), b.fill(3)
    return marks


@functools.lru_cache(None)
def b_edges():
    """-> [(case, [first, middle, last record])]"""
    out = []
    for name, pre, put in _edges():
        b = Build(_rng(name), pre)
        marks = _edge_stream(b, put)
        out.append((case(name, b.finish()), marks))
    return out


def family_b():
    return [c for c, _ in b_edges()]


# ---- C. windows, input blocks, the ring -------------------------------------------------------------------------------
C_OPCODES = {"M1": 2, "M2": 2, "M3 short": 3, "M3 long": 4}


def _c_put(b, kind, lit=3):
    if kind == "M1":
        return b.m(b.off(hi=1024), 2, lit, "M1")
    if kind == "M2":
        return b.m(b.off(hi=2048), 5, lit, "M2")
    if kind == "run":
        return b.add(("run", 18))
    return b.m(b.off(), 20 if kind == "M3 short" else 60, lit, "M3")


@functools.lru_cache(None)
def c_window_edges():
    """-> [(case, [(record, window, lane)])]: an opcode of 2, 3 and 4 bytes whose first byte is byte 60..63 of a window"""
    out = []
    for kind in C_OPCODES:
        b, marks = Build(_rng("C edge " + kind), 1100), []
        for w, lane in itertools.product(range(G.kWindows), range(60, 64)):
            if kind == "M1":  # behind a match with one literal, three bytes in front
                b.place(w, lane - 3)
                b.m(b.off(hi=2048), 3, 1, "M2")
            else:
                b.place(w, lane)
            marks.append((_c_put(b, kind), w, lane))
            b.fill(2)
            b.sync()
        out.append((case("C window edge " + kind, b.finish()), marks))
    return out


@functools.lru_cache(None)
def c_long_runs():
    """literal runs that start in one window and end three and more windows on"""
    b, marks = Build(_rng("C runs"), 700), []
    for lane, n in ((60, RUN_BYTE), (63, 190), (0, 200), (30, 170)):
        b.place(0, lane)
        marks.append(b.add(("run", n)))
        b.fill(40)
        b.sync()
    return case("C runs over windows", b.finish()), marks


@functools.lru_cache(None)
def c_block_edges():
    """-> [(case, [(record, boundary)])]: opcodes and literals over input offsets 1024, 2048, 3072 (and 4096)"""
    out = []
    bounds = [G.kInBlk * k for k in (1, 2, 3, 4)]
    for kind in ("M2", "M3 short", "M3 long", "run"):
        k = C_OPCODES.get(kind, 1)
        for d in sorted({1, k, k + 1}):  # the boundary inside the opcode / right behind it / inside the literals
            b, marks = Build(_rng("C block %s %d" % (kind, d)), 700), []
            for bd in bounds:
                b.pad_in(bd - d)
                r = _c_put(b, kind)
                marks.append((r, bd))
            out.append((case("C block edge %s -%d" % (kind, d), b.finish()), marks))
    return out


@functools.lru_cache(None)
def c_ring_wrap():
    """-> [(case, [record])]: runs whose literals start at ring byte kInRing - 7 .. kInRing - 1: the 8-byte load of the
    literals runs over the ring's end (short runs: the lane's own load; longer ones: the wave's)"""
    out = []
    for rb in range(G.kInRing - 7, G.kInRing):
        b, marks = Build(_rng("C ring %d" % rb), 700), []
        for turn, n in ((0, 12), (1, 16), (2, 40)):
            b.pad_in(turn * G.kInRing + rb - (1 if n <= 18 else 2))
            marks.append(b.add(("run", n)))
        out.append((case("C ring byte %d" % rb, b.finish()), marks))
    return out


@functools.lru_cache(None)
def c_reload():
    b = Build(_rng("C reload"), 200)
    b.add(("run", 5000))
    b.dense(200)
    b.pad_in(b.ipos + 2)
    b.add(("run", 20000))
    b.dense(200)
    return case("C runs of 5000 and 20000", b.finish())


@functools.lru_cache(None)
def c_last_load():
    """inputs 0..17 bytes longer than a multiple of 1 KiB: the last 16-byte load of a block is partial"""
    out = []
    for e in range(18):
        b = Build(_rng("C last %d" % e), 300)
        b.dense(300)
        total = (b.ipos // G.kInBlk + 2) * G.kInBlk + e
        b.pad_in(total - 3 - 10)
        b.add(("run", 9))
        out.append(case("C input length %d" % total, b.finish(tail=False)))
        assert len(out[-1].stream) == total
    return out


@functools.lru_cache(None)
def family_c():
    return ([c for c, _ in c_window_edges()] + [c_long_runs()[0]] + [c for c, _ in c_block_edges()] +
            [c for c, _ in c_ring_wrap()] + [c_reload()] + c_last_load())


# ---- D. a full batch ----------------------------------------------------------------------------------------------------
def _lengths(rng, j, total, lo=34, hi=M3_BYTE):
    """j match lengths of the 4-byte M3 form that add up to `total`"""
    assert lo * j <= total <= hi * j, (j, total)
    ls = [total // j + (1 if k < total % j else 0) for k in range(j)]
    for _ in range(4 * j):
        a, c = rng.randrange(j), rng.randrange(j)
        d = rng.randrange(0, min(ls[a] - lo, hi - ls[c]) + 1)
        if a != c:
            ls[a] -= d
            ls[c] += d
    assert sum(ls) == total and all(lo <= x <= hi for x in ls)
    return ls


@functools.lru_cache(None)
def d_overflow_places():
    """-> [(case, window, lane, bytes in front)]: 4-byte M3 instructions, 16 a window; the one that does not fit the batch
    any more is lane 0, a middle lane or the last marked lane (60) of each window.  (Not lane 0 of window 0 - a batch holds
    its first instruction - and in window 0 the middle lane is 48: eleven matches of 288 are needed to fill a batch.)"""
    out = []
    for w, which in itertools.product(range(G.kWindows), ("first", "middle", "last")):
        if w == 0 and which == "first":
            continue
        j = 16 * w + {"first": 0, "middle": 12 if w == 0 else 8, "last": 15}[which]
        b = Build(_rng("D %d %s" % (w, which)), 3000)
        total = G.kBatchMax - b.rng.randrange(0, 34)
        for ln in _lengths(b.rng, j, total) + [M3_BYTE] + _lengths(b.rng, 5, 600):
            b.m(b.off(), ln, 0, "M3")
        out.append((case("D overflow at window %d %s" % (w, which), b.finish()), w, 4 * (j % 16), total))
    return out


@functools.lru_cache(None)
def d_totals():
    """-> [(case, total)]: twelve matches that add up to kBatchMax - 1, kBatchMax and kBatchMax + 1"""
    out = []
    for total in (G.kBatchMax - 1, G.kBatchMax, G.kBatchMax + 1):
        b = Build(_rng("D total %d" % total), 3000)
        for ln in _lengths(b.rng, 12, total) + _lengths(b.rng, 5, 600):
            b.m(b.off(), ln, 0, "M3")
        out.append((case("D total %d" % total, b.finish()), total))
    return out


@functools.lru_cache(None)
def d_alignments():
    """one stream of 256 one-match batches: start and end of the batch at every pair of residues mod 16, with an empty
    and a non-empty 16-byte body between head and tail"""
    b = Build(_rng("D align"), 700)
    for a, e in itertools.product(range(16), range(16)):
        b.sync(extra=(a - (b.opos + M3_BYTE + 1)) % 16)
        assert b.opos % 16 == a
        t = (e - a) % 16 + 16 * b.rng.choice((0, 0, 1, 2, 5))
        b.m(b.off(), t if t >= 3 else t + 16, 0, "M3")
    b.sync()
    return case("D alignments", b.finish())


@functools.lru_cache(None)
def family_d():
    return [c[0] for c in d_overflow_places()] + [c[0] for c in d_totals()] + [d_alignments()]


# ---- E. where a match's bytes come from ---------------------------------------------------------------------------
FAR_LENGTHS = (2, 7, 8, 9, 15, 16, 17, 24, 25, M3_BYTE)
OVERLAP_OFFSETS = (1, 2, 3, 5, 63, 64, 65, 287)


def _e_far(b):
    """sources that end in front of the batch: the first one exactly at its start, then 1, 5 and 100 bytes earlier"""
    for mlen in FAR_LENGTHS:
        b.sync(lit=1 if mlen == 2 else 0)
        b.m(mlen, mlen, 1 if mlen == 2 else 0)
        for gap in (0, 1, 5, 100):
            b.m(b.r + mlen + gap, mlen, 1 + gap % 3)


def _e_straddle(b):
    """sources that start `back` bytes in front of the batch and end inside it"""
    for group in (((100, 50), (100, 50), (M3_BYTE, 100), (20, 5), (64, 1), (65, 64)), ((M3_BYTE, 1), (9, 8), (3, 2)),
                  ((65, 64), (200, 199), (M3_BYTE, 287)), ((8, 7), (16, 3), (17, 16), (M3_BYTE, 5))):
        b.sync()
        for mlen, back in group:  # (the first of a group: offset < length; behind it the offset grows with the batch)
            assert 0 < back < mlen
            b.m(b.r + back, mlen, b.rng.randrange(4))


def _e_near(b):
    """sources inside the batch: short ones without overlap, then overlaps at the offsets where the copy's cases change"""
    b.sync()
    b.add(("run", 70))
    for mlen, off in ((3, 3), (8, 60), (64, 64), (64, 70), (33, 33), (2, 2), (40, 200)):
        b.m(off, mlen, 1)
    for off in OVERLAP_OFFSETS:
        b.sync()
        if off + 10 <= RUN_BYTE:
            b.add(("run", max(off + 10, 4)))
        else:
            b.add(("run", RUN_BYTE))
            b.m(b.off(), 40, 0)
        assert b.r >= off
        for mlen in sorted({max(off + 1, 3), 65, off + 64, M3_BYTE}):
            b.m(off, min(mlen, M3_BYTE), b.rng.randrange(4))


def _e_chains(b):
    """a near match whose source is a far match of the batch, a near match, a near match of an earlier window, the
    literals of a run of the batch"""
    b.sync()
    b.m(b.r + 500, 40, 0)   # far
    b.m(40, 30, 0)          # its bytes
    b.m(30, 20, 2)          # the near match's bytes
    at = b.opos
    b.place(1, 5)           # a window on
    b.m(b.opos - at + 22, 22, 0)
    b.place(3, 9)
    b.m(b.opos - at + 52, 60, 3)
    b.sync()
    b.add(("run", 50))
    b.m(50, 40, 0)
    b.m(25, 60, 0)
    b.add(("run", 200))
    b.m(200, 200, 1)


def _e_small_last_batch(b):
    """a last batch of far matches that starts less than 8 bytes in front of the output's end"""
    b.sync()
    b.m(b.r + 500, 3, 2)
    b.add(("end",))
    return b


E_STREAMS = (("E far", _e_far), ("E straddle", _e_straddle), ("E near", _e_near), ("E chains", _e_chains))


@functools.lru_cache(None)
def family_e():
    cases = []
    for name, fn in E_STREAMS:
        b = Build(_rng(name), 3000)
        fn(b)
        b.tail(CHECK_ZONE)  # (finish()'s tail, then the small last batch in front of the end)
        _e_small_last_batch(b)
        cases += [case(name + ", exact room", b), case(name + ", room to spare", b, cap=len(b.out) + 64)]
    return cases


# ---- F. the room ------------------------------------------------------------------------------------------------------
def _caps(need):
    return [need - G.kStage + d for d in (-1, 0, 1)] + [need + d for d in (-1, 0, 1)]


@functools.lru_cache(None)
def f_small():
    b = Build(_rng("F small"), 700)
    b.dense(900)
    return b.finish(tail=False)


@functools.lru_cache(None)
def f_big():
    """more than 49 152 + 2 batches of output, offset 49 151 in the batch that crosses 49 152 and behind it"""
    b = Build(_rng("F big"), UNCHECKED_FROM - 1200)
    b.sync()
    while b.opos < M4_MAX_OFF:
        b.m(b.off(), 150, 0, "M3")
    for _ in range(6):
        b.m(M4_MAX_OFF, b.rng.randrange(3, 10), b.rng.randrange(4), "M4")
    while b.opos < UNCHECKED_FROM + 3 * G.kBatchMax + 500:
        b.dense(20, m4=M4_MAX_OFF)
    return b.finish(tail=False)


F_PLACES = ((0, 0), (1, 28), (3, 36))
F_KINDS = ("offset one too far", "match one byte short of room", "literals one byte short of room", "input ends in the opcode",
           "input ends behind the opcode", "input ends in the literals", "input ends behind the literals")


@functools.lru_cache(None)
def f_failures():
    """-> [(case, kind, window, lane, record index)]: an M3 of 4 opcode bytes, 40 bytes and 3 literals that fails at a
    chosen place of a batch"""
    out = []
    for (w, lane), kind in itertools.product(F_PLACES, F_KINDS):
        b = Build(_rng("F %d %d" % (w, lane)), 200)
        b.place(w, lane)
        if kind == "offset one too far":
            r = b.add(("raw", encode("M3", b.opos + 1, 40, 3)))
            b.add(("raw", bytes(b.rng.getrandbits(8) for _ in range(CHECK_ZONE + 60))))
            c = case("F %s at %d/%d" % (kind, w, lane), b, cap=b.opos + 4000)
        else:
            r = b.m(b.off(), 40, 3, "M3")
            b.fill(5)
            b.finish()
            cap, cut = {"match one byte short of room": (r.opos + 39, None), "literals one byte short of room": (r.opos + 42, None),
                        "input ends in the opcode": (None, r.ipos + 2), "input ends behind the opcode": (None, r.ipos + 4),
                        "input ends in the literals": (None, r.ipos + 6),
                        "input ends behind the literals": (None, r.ipos + 7)}[kind]
            c = case("F %s at %d/%d" % (kind, w, lane), b, cap=cap, cut=cut)
        out.append((c, kind, w, lane, r.idx))
    return out


@functools.lru_cache(None)
def family_f():
    cases = []
    for name, b in (("F small", f_small()), ("F big", f_big())):
        cases += [case("%s, room %d" % (name, cap), b, cap=cap) for cap in _caps(len(b.out))]
    return cases + [c[0] for c in f_failures()]


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "E": family_e, "F": family_f}


@functools.lru_cache(None)
def family_g(count=2000, small=1600):
    """every stream of A-F, and the small ones again and again, shuffled: `count` streams, which the caller makes more
    than the device's resident workgroups - then the counter hands the streams out in an order of its own"""
    rng = random.Random(7007)
    cases = [c for f in FAMILIES.values() for c in f()]
    again = [c for c in cases if c.cap <= small and len(c.stream) <= small]
    cases = cases + [rng.choice(again) for _ in range(count - len(cases))]
    rng.shuffle(cases)
    return cases


def counts():
    """from the writer's records and the replay: what the families send through the decoder"""
    tot = collections.Counter()
    seen = set()
    for f in FAMILIES.values():
        for c in f():
            if id(c.b) in seen:
                continue
            seen.add(id(c.b))
            tot.update(c.b.counts())
            if not c.b.malformed:
                ev = only_batches(batches(c.b.recs, len(c.b.stream), len(c.b.out)))
                tot["full batch cuts"] += sum(1 for e in ev if e.stop and e.stop[0] == "full")
                tot["M1 on the fast path, away from the input's end"] += sum(
                    1 for e in ev for base, lanes in e.wins for r in lanes if r.form == "M1" and base + CHECK_ZONE <= len(c.b.stream))
    return tot
