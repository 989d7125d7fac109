"""A size-only reading of `Lzo.uncompress_with_buffer` (lib/lzo.ml:199-216, :246-293, :315-414) in Python - test
infrastructure, the yardstick of the size query (md_lzo_sizes_batch_*, md_lzo_uncompress_with_buffer).

It follows the reference's fiber instruction by instruction with a buffer that grows: no byte is produced, only the
buffer's length is kept.  What can go wrong is what can go wrong there:

    1   "Unexpected end of input"   an instruction of `run` other than State / Return with the input used up (:268-269)
    4   `Invalid_dictionary         copy_to_buffer with an offset beyond the buffer's length (:216)
    14  "Invalid input"             count reaches the input's end (:234)
    15  "No dictionary at offset 0 available"   the first byte is 16 (:376)
    17  "Malformed input"           the exception Out_of_bound (:414): literals (bigstring_to_string, :200) or a two-byte
                                    operand (get_int16 / Junk Short, :276-281) over the input's end

size(src) -> (status, size); the size is 0 unless the status is 0."""
import re

OK, END_OF_INPUT, INVALID_DICTIONARY, INVALID_INPUT, NO_DICTIONARY, OUT_OF_BOUND, MALFORMED = 0, 1, 4, 14, 15, 16, 17
STATUSES = (OK, END_OF_INPUT, INVALID_DICTIONARY, INVALID_INPUT, NO_DICTIONARY, MALFORMED)
_NOT_ZERO = re.compile(b"[^\\x00]")


class _Stop(Exception):
    pass


class _Reader:
    def __init__(self, src):
        self.src, self.n, self.i, self.o, self.state = src, len(src), 0, 0, 0

    def guard(self):
        """every Peek / Junk / Count / Transmit / Copy of `run` begins with this test"""
        if self.i >= self.n:
            raise _Stop(END_OF_INPUT)

    def byte(self):
        self.guard()   # Peek Byte
        b = self.src[self.i]
        self.guard()   # Junk Byte
        self.i += 1
        return b

    def short(self):
        self.guard()   # Peek (Short `LE)
        if self.i + 2 > self.n:
            raise _Stop(MALFORMED)
        s = self.src[self.i] | (self.src[self.i + 1] << 8)
        self.guard()   # Junk (Short _)
        self.i += 2
        return s

    def count(self):
        self.guard()
        m = _NOT_ZERO.search(self.src, self.i)   # the 4-byte and the 1-byte scan count the same zeros
        if m is None:
            raise _Stop(INVALID_INPUT)
        zeros = m.start() - self.i
        self.i = m.start() + 1
        return zeros * 255 + self.src[m.start()]

    def transmit(self, n, state):
        self.guard()
        self.state = state
        self.literals(n)

    def literals(self, n):
        if n > self.n - self.i:
            raise _Stop(MALFORMED)
        self.i += n
        self.o += n

    def copy(self, off, length, state):
        self.guard()
        self.state = state
        if off > self.o:
            raise _Stop(INVALID_DICTIONARY)
        self.o += length + 2
        self.literals(state & 3)   # copy_done: transmit of `run`'s argument, not an instruction of its own


def _run(r):
    r.guard()   # peek byte
    first = r.src[0]
    if first == 16:
        raise _Stop(NO_DICTIONARY)
    if first >= 18:
        r.guard()
        r.i = 1
        r.transmit(first - 17, 0)
    while True:
        c = r.byte()
        st = r.state & 3   # (State._no_extra is -1: -1 land 3 = 3, the arm for -1 is never taken)
        if c < 16 and st == 0:
            r.transmit(c + 3 if c else 18 + r.count(), -1)
        elif c < 16:
            h = r.byte()
            r.copy((h << 2) + (c >> 2) + 1, 0, c & 3)
        elif c < 32:
            length = c & 7 or 7 + r.count()
            s = r.short()
            off = 16384 + ((c & 8) << 11) + (s >> 2)
            if off == 16384:
                return
            r.copy(off, length, s & 0xff)
        elif c < 64:
            length = c & 31 or 31 + r.count()
            s = r.short()
            r.copy((s >> 2) + 1, length, s & 0xff)
        else:
            h = r.byte()
            r.copy((h << 3) + ((c >> 2) & 7) + 1, (c >> 5) - 1, c)


def size(src):
    r = _Reader(bytes(src))
    try:
        _run(r)
    except _Stop as e:
        return e.args[0], 0
    return OK, r.o


def as_uncompress(status):
    """the status Lzo.uncompress gives where uncompress_with_buffer gives `status` (room that never runs out): both
    `Invalid_dictionary and "Malformed input" are its "Input is malformed or output is not large enough\""""
    return OUT_OF_BOUND if status in (INVALID_DICTIONARY, MALFORMED) else status


# ---- streams the CPU and the GPU tests of the size query share --------------------------------------------------------
def random_streams(seed=5, count=3000):
    """short random streams, 1..59 bytes; a byte is 0 (twice as likely as each of the others), 17, any byte, a value
    below 16 or a value in 16..63: the opcodes where lengths go on, the end marker's first byte, every form of match"""
    import random
    rng = random.Random(seed)
    draw = (lambda: 0, lambda: 0, lambda: 17, lambda: rng.getrandbits(8), lambda: rng.randrange(16), lambda: rng.randrange(16, 64))
    return [bytes(rng.choice(draw)() for _ in range(rng.randrange(1, 60))) for _ in range(count)]


def cut_streams():
    """one stream of family A (tests/lzo_batches.py) cut at every byte, the whole stream last"""
    from tests import lzo_batches
    c = next(c for c in lzo_batches.family_a() if c.name == "A M1 after, no tail")
    return [c.stream[:k] for k in range(len(c.stream) + 1)]
