"""The test-side LZO1X writer (tests/lzo_writer.py) against the CPU oracle and, on the streams liblzo reads the same way,
minilzo; and the hand-built families of tests/lzo_batches.py: each is where it claims to be in the decoder's batches,
by the kernel's own sizes (read from its source).  The GPU tests (tests/test_gpu_lzo_batches.py) decode these streams,
so the writer must be right and the streams must be at the limits."""
import random

import pytest

from tests import lzo_batches as lb
from tests import oracle_lib
from tests.lzo_batches import G, batches, only_batches
from tests.lzo_writer import M3_BYTE, M4_MAX_OFF, Writer, encode, random_instructions, write

OUT_OF_BOUND = 16


@pytest.mark.parametrize("block", range(6))
def test_random_instructions_equal_oracle(oracle, block):
    """300 seeded lists: status 0, the writer's bytes and exactly its room; one byte less room is the oracle's error"""
    forms = set()
    for seed in range(50 * block, 50 * block + 50):
        ins, w = random_instructions(random.Random(seed), compatible=False)
        stream, want = write(ins, random.Random(seed))  # (the same generator state: the same literals)
        assert len(stream) == len(w.stream) and want is not None
        stream, want = bytes(w.stream), bytes(w.out)
        assert oracle.lzo_uncompress(stream, len(want)) == (0, want), seed
        assert oracle.lzo_uncompress(stream, len(want) + 100) == (0, want), seed
        if want:
            assert oracle.lzo_uncompress(stream, len(want) - 1) == (OUT_OF_BOUND, b""), seed
        forms |= {r.form for r in w.recs}
    assert forms >= {"first", "run", "M1", "M2", "M3", "M4", "end"}


def test_minilzo_agrees_on_the_compatible_subset(oracle):
    """(absent where oracle/_ref is) liblzo's decoder on streams without an opcode below 16 right behind a literal run"""
    m = oracle_lib.load_minilzo()
    if m is None:
        return
    n_m1 = 0
    for seed in range(1000, 1150):
        ins, w = random_instructions(random.Random(seed), compatible=True)
        assert m.decompress(bytes(w.stream), len(w.out)) == (0, bytes(w.out)), seed
        n_m1 += w.counts()["M1"]
    assert n_m1 > 100
    for fam in lb.FAMILIES.values():
        for c in fam():
            if c.out is not None and c.b.liblzo_compatible:
                assert m.decompress(c.stream, c.cap)[1] == c.out, c.name


def test_state_rule_and_raw_bytes(oracle):
    """an opcode below 16 is a run in state zero and M1 otherwise - the same two bytes, both ways; raw bytes; asserts"""
    rng = random.Random(3)
    a = Writer(rng).extend([("first", 40), ("M2", 7, 3, 0), ("run", 5, bytes([9, 1, 2, 3, 4])), ("M2", 1, 3, 0), ("end",)])
    b = Writer(rng).extend([("first", 40), ("M2", 7, 3, 1), ("M1", (9 << 2) + 1, 2, 2), ("M2", 1, 3, 0), ("end",)])
    assert bytes(a.stream[43:45]) == bytes(b.stream[44:46]) == bytes([2, 9])
    for w in (a, b):
        assert oracle.lzo_uncompress(bytes(w.stream), len(w.out)) == (0, bytes(w.out))
    assert (a.recs[2].zero, b.recs[2].zero) == (True, False)
    with pytest.raises(AssertionError):
        Writer(rng).extend([("first", 40), ("M2", 7, 3, 0), ("M1", 1, 2, 0)])   # M1 in state zero
    with pytest.raises(AssertionError):
        Writer(rng).extend([("first", 40), ("M2", 7, 3, 1), ("run", 5)])         # a run in a state that is not zero
    with pytest.raises(AssertionError):
        Writer(rng).extend([("first", 40), ("M2", 41, 3, 0)])                    # an offset beyond the output
    stream, want = write([("first", 40), ("raw", encode("M2", 41, 3, 0)), ("raw", bytes(8))], rng)
    assert want is None and oracle.lzo_uncompress(stream, 100) == (OUT_OF_BOUND, b"")


def test_geometry_is_read_from_the_kernel():
    assert G.kWave == 64 and G.kWindows >= 1 and G.kInRing == 2 * G.kInBlk and G.kBatchMax < G.kStage
    assert 12 * 34 <= G.kBatchMax - 33 and G.kBatchMax <= 12 * M3_BYTE  # (family D's window 0: twelve 4-byte matches can fill a batch)


def _replay(c):
    return batches(c.b.recs, len(c.stream), c.cap)


def _find(ev, rec):
    """-> (batch, window, lane) of a record on the fast path, or None"""
    for e in only_batches(ev):
        for w, (base, lanes) in enumerate(e.wins):
            if rec in lanes:
                return e, w, rec.ipos - base
    return None


def _is_slow(ev, rec):
    return ("slow", rec) in ev


def test_every_family_equals_the_oracle(oracle):
    seen = set()
    for fam in lb.FAMILIES.values():
        for c in fam():
            st, out = oracle.lzo_uncompress(c.stream, c.cap)
            assert (st, out) == ((0, c.out) if c.out is not None else (st, b"")) and (st == 0) == (c.out is not None), c.name
            seen.add(st)
    assert seen >= {0, 1, 16}


def test_family_a_geometry():
    cases = {c.name: c for c in lb.family_a()}
    for name, _, _ in lb.A_STREAMS:
        far, near = cases[name + ", tail"], cases[name + ", no tail"]
        assert far.b.recs[:len(near.b.recs) - 1] == near.b.recs[:-1]  # the same instructions
        for c, zone in ((far, False), (near, True)):
            m1 = [(e, base) for e in only_batches(_replay(c)) for base, lanes in e.wins for r in lanes if r.form == "M1"]
            few = 1 if name == "A dense32" else 15
            assert len(m1) >= few, (c.name, len(m1))
            if zone:  # the last M1 instructions are inside the zone next to the input's end
                assert sum(1 for _, base in m1 if base + lb.CHECK_ZONE > len(c.stream)) >= min(few, 5), c.name
            else:
                assert all(base + lb.CHECK_ZONE <= len(c.stream) for _, base in m1), c.name
    ev = only_batches(_replay(cases["A dense, tail"]))
    assert any(len({r.zero for r in lanes}) == 2 and {r.form for r in lanes} >= {"M1", "M2", "M3", "run"} for e in ev for _, lanes in e.wins)
    assert {r.form for e in ev for _, lanes in e.wins for r in lanes} >= {"M1", "M2", "M3", "M4", "run"}
    assert {(r.form, r.lit) for e in ev for _, lanes in e.wins for r in lanes} >= {(f, k) for f in ("M1", "M2", "M3", "M4") for k in range(4)}
    after = cases["A M1 after, tail"].b.recs
    prev = {(after[r.idx - 1].form if after[r.idx - 1].form == "run" else after[r.idx - 1].lit, r.off) for r in after if r.form == "M1"}
    assert prev >= {(p, off) for p in ("run", 1, 2, 3) for off in (1, 2, 1023, 1024)}
    low = cases["A low opcodes, tail"].b
    assert {low.stream[r.ipos] for r in low.recs if r.form == "run" and r.zero} >= set(range(1, 16))
    assert {low.stream[r.ipos] for r in low.recs if r.form == "M1"} >= set(range(1, 16))
    d32 = only_batches(_replay(cases["A dense32, tail"]))
    full = [lanes for e in d32 for _, lanes in e.wins if len(lanes) == 32]
    assert len(full) == 2 and {lanes[0].form for lanes in full} == {"M1", "M2"}


def test_family_b_geometry():
    assert len(lb.b_edges()) == 20
    for c, (first, middle, last) in lb.b_edges():
        ev = _replay(c)
        if lb.exotic(first):  # the interpreter's: right behind another slow step, between two batches, in front of another
            for r in (first, middle, last):
                assert _is_slow(ev, r), c.name
            k = [ev.index(("slow", r)) for r in (first, middle, last)]
            assert ev[k[0] - 1].osum == 0 and ev[k[0] - 2][0] == "slow" and ev[k[0] + 1].osum > 0, c.name
            assert ev[k[1] - 1].osum > 0 and ev[k[1] + 1].osum > 0, c.name
            assert ev[k[2] - 1].osum > 0 and ev[k[2] + 1].osum == 0 and ev[k[2] + 2][0] == "slow", c.name
        else:
            (e0, w0, l0), (e1, w1, l1), (e2, w2, l2) = (_find(ev, r) for r in (first, middle, last))
            assert (w0, l0) == (0, 0) and ev[ev.index(e0) - 1][0] == "slow" and sum(len(lanes) for _, lanes in e0.wins) > 1, c.name
            recs1 = [r for _, lanes in e1.wins for r in lanes]
            assert recs1[0] != middle != recs1[-1], c.name
            assert [r for _, lanes in e2.wins for r in lanes][-1] == last and e2.stop[0] == "exotic", c.name
    names = " ".join(c.name for c, _ in lb.b_edges())
    for what in ("M3 length 33", "M3 length 34", "M3 length 288", "M3 length 289", "M3 length 543", "M3 length 544", "M4 length 9",
                 "M4 length 10", "M4 length 264", "M4 length 265", "run 18", "run 19", "run 273", "run 274", "M3 offset 16383",
                 "M3 offset 16384", "M4 offset 16385", "M4 offset 32767", "M4 offset 32768", "M4 offset 49151"):
        assert what in names
    slow = {c.name for c, m in lb.b_edges() if lb.exotic(m[0])}
    assert slow == {"B M3 length 289", "B M3 length 543", "B M3 length 544", "B M4 length 265", "B run 274", "B M3 offset 16384"}


def test_family_c_geometry():
    for c, marks in lb.c_window_edges():
        ev = _replay(c)
        assert {(w, lane) for _, w, lane in marks} == {(w, lane) for w in range(G.kWindows) for lane in range(60, 64)}
        for rec, w, lane in marks:
            assert _find(ev, rec)[1:] == (w, lane), (c.name, w, lane)
    assert {m[0].k for _, marks in lb.c_window_edges() for m in marks} == {2, 3, 4}
    c, marks = lb.c_long_runs()
    ev = _replay(c)
    for rec in marks:
        e, w, lane = _find(ev, rec)
        assert w == 0 and lane + rec.k + rec.lit >= 3 * 64 and len(e.wins) > 1, c.name
    for c, marks in lb.c_block_edges():
        ev = _replay(c)
        assert [bd for _, bd in marks] == [G.kInBlk * k for k in (1, 2, 3, 4)] and G.kInRing == 2 * G.kInBlk
        for rec, bd in marks:
            assert rec.ipos < bd < rec.ipos + rec.k + rec.lit and _find(ev, rec), (c.name, bd)
    assert {(bd - r.ipos < r.k, bd - r.ipos == r.k) for _, marks in lb.c_block_edges() for r, bd in marks} == {(True, False), (False, True), (False, False)}
    starts = set()
    for c, marks in lb.c_ring_wrap():
        ev = _replay(c)
        for rec in marks:
            assert _find(ev, rec) and rec.lit >= 8, c.name
            starts.add(((rec.ipos + rec.k) % G.kInRing, rec.lit > 16))
    assert starts >= {(rb, long) for rb in range(G.kInRing - 7, G.kInRing) for long in (False, True)}
    ev = _replay(lb.c_reload())
    for n in (5000, 20000):
        k = next(i for i, e in enumerate(ev) if e[0] == "slow" and e[1].form == "run" and e[1].lit == n)
        assert n > 2 * G.kInRing and sum(len(lanes) for _, lanes in ev[k + 1].wins) >= 4 * G.kWindows
    assert [len(c.stream) % G.kInBlk for c in lb.c_last_load()] == list(range(18))


def test_family_d_geometry():
    places = set()
    for c, w, lane, total in lb.d_overflow_places():
        e = next(e for e in only_batches(_replay(c)) if e.osum)  # (behind the preamble, which is the interpreter's)
        assert e.osum == total <= G.kBatchMax and e.stop[0] == "full" and e.stop[2:] == (w, lane), c.name
        assert all(r.k == 4 and r.mlen <= M3_BYTE for _, lanes in e.wins for r in lanes) and e.stop[1].mlen == M3_BYTE
        last = e.wins[w][1][-1].ipos - e.wins[w][0] if w < len(e.wins) and e.wins[w][1] else None
        places.add((w, "first" if lane == 0 else "last" if lane == 60 and last == 56 else "middle"))
    assert places == {(w, p) for w in range(G.kWindows) for p in ("first", "middle", "last")} - {(0, "first")}
    for c, total in lb.d_totals():
        e = next(e for e in only_batches(_replay(c)) if e.osum)
        assert e.stop[0] == "full" and e.osum == (total if total <= G.kBatchMax else total - e.stop[1].mlen), c.name
    assert [t - G.kBatchMax for _, t in lb.d_totals()] == [-1, 0, 1]
    ev = only_batches(_replay(lb.d_alignments()))
    pairs = {(e.o0 % 16, (e.o0 + e.osum) % 16) for e in ev if e.osum and e.stop and e.stop[0] == "exotic"}
    assert pairs == {(a, b) for a in range(16) for b in range(16)}
    body = lambda e: ((e.o0 + e.osum) & ~15) - ((e.o0 + 15) & ~15)
    assert any(body(e) <= 0 for e in ev if e.osum) and any(body(e) >= 32 for e in ev if e.osum)


def _sources(c):
    """-> [(kind, record, batch)] for every match on the fast path: where its source lies"""
    out = []
    for e in only_batches(_replay(c)):
        for _, lanes in e.wins:
            for r in lanes:
                if r.mlen:
                    s = r.opos - r.off
                    out.append(("far" if s + r.mlen <= e.o0 else "straddle" if s < e.o0 else "near", r, e))
    return out


def test_family_e_geometry():
    cases = {c.name: c for c in lb.family_e()}
    far = [(r, e) for k, r, e in _sources(cases["E far, exact room"]) if k == "far"]
    assert {r.mlen for r, _ in far} >= set(lb.FAR_LENGTHS)
    assert {r.mlen for r, e in far if r.opos - r.off + r.mlen == e.o0} >= set(lb.FAR_LENGTHS)  # one ends exactly at the batch's start
    st = [r for k, r, _ in _sources(cases["E straddle, exact room"]) if k == "straddle"]
    assert len(st) >= 16 and any(r.off < r.mlen for r in st) and any(r.off >= r.mlen > 64 for r in st)
    assert any(r.off == 1 and r.mlen == M3_BYTE for r in st) and any(r.off >= r.mlen <= 64 for r in st)
    near = [r for k, r, _ in _sources(cases["E near, exact room"]) if k == "near"]
    assert any(r.off >= r.mlen and r.mlen <= 64 for r in near) and any(r.mlen == 2 for r in near)
    for off in lb.OVERLAP_OFFSETS:
        assert any(r.off == off < r.mlen for r in near) and any(r.off == off and r.mlen == M3_BYTE for r in near), off
    assert any(r.off == 287 and r.mlen == 65 for r in near)  # no overlap, but longer than a wavefront
    src = _sources(cases["E chains, exact room"])
    inside = lambda r, q: q.opos <= r.opos - r.off and r.opos - r.off + min(r.mlen, r.off) <= q.opos + q.mlen + q.lit
    for kind, other_window in (("far", False), ("near", False), ("near", True)):
        assert any(k == "near" and k2 == kind and e is e2 and inside(r, r2) and r2.mlen and
                   (not other_window or r.ipos - r2.ipos >= 64) for k, r, e in src for k2, r2, e2 in src), (kind, other_window)
    runs = [r for e in only_batches(_replay(cases["E chains, exact room"])) for _, lanes in e.wins for r in lanes if r.form == "run"]
    assert any(k == "near" and q.opos <= r.opos - r.off and r.opos - r.off + r.mlen <= q.opos + q.lit for k, r, _ in src for q in runs)
    for name, c in cases.items():
        last = only_batches(_replay(c))[-1]
        assert last.osum and all(k == "far" for k, r, e in _sources(c) if e is last)
        assert (last.o0 + 8 > c.cap) == name.endswith("exact room"), name  # the guarded loader / whole 8-byte words


def test_family_f_geometry():
    for b, name in ((lb.f_small(), "F small"), (lb.f_big(), "F big")):
        need = len(b.out)
        assert [c.cap - need for c in lb.family_f() if c.name.startswith(name)] == [-G.kStage - 1, -G.kStage, -G.kStage + 1, -1, 0, 1]
        assert b.recs[-2].form != "end" and not lb.exotic(b.recs[-2])  # the stream ends in a plain batch
    b = lb.f_big()
    need = len(b.out)
    assert need > lb.UNCHECKED_FROM + 2 * G.kBatchMax
    ev = only_batches(batches(b.recs, len(b.stream), need))
    has = lambda e: any(r.off == M4_MAX_OFF for _, lanes in e.wins for r in lanes)
    assert any(e.o0 < lb.UNCHECKED_FROM and has(e) for e in ev)
    unchecked = [e for e in ev if e.o0 >= lb.UNCHECKED_FROM and need - e.o0 >= G.kStage and has(e)]
    checked = [e for e in ev if e.o0 >= lb.UNCHECKED_FROM and need - e.o0 < G.kStage and has(e)]
    assert len(unchecked) >= 2 and checked  # the switch flips between two batches
    for cap in (need - G.kStage, need - 1):  # too little room: the batch that fails is one the switch has turned on
        last = only_batches(batches(b.recs, len(b.stream), cap))[-1]
        assert last.stop[0] == "bad" and last.o0 >= lb.UNCHECKED_FROM, cap
    got = set()
    for c, kind, w, lane, idx in lb.f_failures():
        last = only_batches(_replay(c))[-1]
        reason = {"offset one too far": "raw"}.get(kind, "bad" if "room" in kind else "exotic")
        if kind == "input ends behind the literals":  # nothing is missing from it: the fast path takes it, the next one fails
            assert last.wins[-1][1][-1].idx == idx and last.stop[1].ipos == len(c.stream), c.name
            assert last.stop[0] == "exotic" and last.stop[1].idx == idx + 1 and last.stop[2:] == (w, lane + 7), c.name
        else:
            assert last.stop[0] == reason and last.stop[1].idx == idx and last.stop[2:] == (w, lane), (c.name, last.stop)
        assert c.out is None and (w, lane) in lb.F_PLACES
        got.add((kind, w, lane))
    assert len(got) == len(lb.F_KINDS) * len(lb.F_PLACES)


def test_family_g_and_counts():
    g = lb.family_g()
    assert len(g) >= 2000 and {id(c) for f in lb.FAMILIES.values() for c in f()} <= {id(c) for c in g}
    assert sum(c.cap for c in g) < 16 << 20 and sum(c.cap for c in lb.family_g(12000)) < 16 << 20  # (a device's worth)
    for fam in lb.FAMILIES.values():
        assert sum(c.cap for c in fam()) < 16 << 20
    n = lb.counts()
    # what the compressor-made streams of the suite never held (tests/test_gpu_lzo.py): now by the hundred
    assert n["M1 on the fast path, away from the input's end"] >= 1000 and n["mlen288"] >= 30 and n["off49151"] >= 30
    assert n["full batch cuts"] >= 15
