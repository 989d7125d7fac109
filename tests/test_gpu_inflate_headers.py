"""The inflate kernels' dynamic-header parser (dynamic_tables, build_walk, canon_counts in csrc/inflate_wave_core.hpp,
compiled into the batch decoder and into the size query) on hand-built headers: the corpus of
tests/deflate_header_cases.py, whose streams tests/test_deflate_headers.py proves (on the CPU) to reach the rules they
are named for.  A failure here therefore names a header rule: the case's name and its reason tag.

Every stream is compared with the CPU oracle in status, consumed and bytes (the plain model equals the oracle on all of
them: the CPU test), under both forms of the kernel; the size query, the ZLIB frame and the streaming decoders see the
same headers.  No profile counter tells the budget form of the walks (incomplete codes) from the plain one, so there is
no probe of it: H5's streams reach it by construction - the header parser sets it for every one-code block."""
import zlib

import pytest

from tests import deflate_header_model as model
from tests.deflate_header_cases import FAMILIES, UNBOUNDED, pieces_streams
from tests.test_gpu_inf_batch import run_batch, run_single
from tests.test_gpu_inflate_rounds import _bounds_run
from tests.test_gpu_inflate_sizes import _sizes

pytestmark = pytest.mark.gpu

OK, END_OF_OUTPUT, DICTIONARY, CHECKSUM = 0, 2, 4, 9
DE, ZL = 0, 1
END, MALFORMED = 2, 3
_REF = {}


@pytest.fixture(scope="module")
def eng():
    import decompress_amd
    return decompress_amd.Engine(0)


@pytest.fixture(params=[2, 1], ids=["two-wavefronts", "one-wavefront"])
def eng_ring(eng, request):
    eng.set_option("inflate_waves", request.param)
    yield eng
    eng.set_option("inflate_waves", 2)


def _ref(oracle, raw, cap):
    if (raw, cap) not in _REF:
        _REF[(raw, cap)] = oracle.de_inflate(raw, cap)
    return _REF[(raw, cap)]


def _check(oracle, cases, results):
    for (name, raw, cap, tag), (st, used, out, adler) in zip(cases, results):
        ost, oused, oout = _ref(oracle, raw, cap)
        assert (st, used) == (ost, oused), (name, tag, st, used, ost, oused)
        assert out == oout, (name, tag, len(out), len(oout), next((i for i, (a, b) in enumerate(zip(out, oout)) if a != b), None))
        if st == OK:
            assert adler == zlib.adler32(out), (name, tag)


@pytest.mark.parametrize("fam", sorted(FAMILIES))
def test_family(eng_ring, oracle, fam):
    cases = FAMILIES[fam]()
    res = eng_ring.inflate_many([c[1] for c in cases], [c[2] for c in cases])
    _check(oracle, cases, res)


def test_bounds(eng_ring, oracle):
    """all families in one batch, outputs back to back in a pattern-filled buffer: nothing outside
    [out_off, out_off + out_len) changes - H5's standing streams write until their room ends, and no further"""
    cases = [c for fam in sorted(FAMILIES) for c in FAMILIES[fam]()]
    _bounds_run(eng_ring, oracle, cases, raw=lambda r: r, check=_check)


def test_sizes(eng, oracle):
    """the size query (include/mdeflate.h): the status of the decode with room that never runs out; consumed 0 on
    failure; out_len = the bytes in front of the failing token.  The streams that stand still and write have no size:
    Unexpected_end_of_output and the bytes in front of the standing point."""
    uniq = {}
    for fam in sorted(FAMILIES):
        for name, raw, cap, tag in FAMILIES[fam]():
            uniq.setdefault(raw, (name, cap, tag))
    raws = list(uniq)
    res = _sizes(eng, DE, raws)
    seen = set()
    for raw, got in zip(raws, res):
        name, cap, tag = uniq[raw]
        if name in UNBOUNDED:
            assert got == (END_OF_OUTPUT, 0, UNBOUNDED[name]), (name, got)
            continue
        ost, oused, oout = _ref(oracle, raw, cap + 1024)
        assert ost != END_OF_OUTPUT, name
        assert got == (ost, oused if ost == OK else 0, len(oout)), (name, tag, got, ost, oused, len(oout))
        seen.add(ost)
    assert seen >= {0, 1, 4, 7}, seen


def test_zlib_frame(eng_ring, oracle):
    """H1 / H3 streams in a ZLIB frame with the right and a wrong Adler-32: a header's fault outranks the checksum"""
    pick = [c for c in FAMILIES["H1"]() if c[0].endswith(" /end")][::6] + [c for c in FAMILIES["H3"]() if c[0].endswith(" /end")][::5]
    assert len(pick) >= 12
    srcs, caps, names = [], [], []
    for name, raw, cap, tag in pick:
        plain = model.inflate(raw, 1 << 20).output
        for wrong in (0, 1):
            srcs.append(b"\x78\x9c" + raw + (zlib.adler32(plain) ^ wrong).to_bytes(4, "big"))
            caps.append(cap)
            names.append((name, tag, wrong))
    res = eng_ring.inflate_many(srcs, caps, fmt=ZL)
    seen = set()
    for src, cap, name, (st, used, out, _) in zip(srcs, caps, names, res):
        ost, oused, oout = oracle.zl_inflate(src, cap)
        assert (st, used, out) == (ost, oused, oout), (name, st, used, ost, oused)
        seen.add((st, name[2]))
    assert seen >= {(OK, 0), (CHECKSUM, 1), (DICTIONARY, 0), (DICTIONARY, 1)}, seen


def test_pieces(eng):
    """the streaming decoders (md_inf_*, md_inf_batch_*) with the input cut at every byte inside the header: the same
    ending and bytes as the uncut stream, which ends as the model says"""
    plans, owner = [], []
    streams = pieces_streams()
    for k, (name, raw, hdr_end) in enumerate(streams):
        plans.append([raw])
        owner.append(k)
        for cut in range(1, hdr_end + 1):
            plans.append([raw[:cut], raw[cut:]])
            owner.append(k)
    res, _, _, _ = run_batch(eng, DE, plans)
    whole = {}
    for plan, k, r in zip(plans, owner, res):
        name, raw, _ = streams[k]
        if len(plan) == 1:
            whole[k] = r
            want = model.inflate(raw, 1 << 20)
            assert run_single(eng, DE, plan) == r, name
            assert (r[0], r[1]) == ((END, 0) if want.status == OK else (MALFORMED, want.status)), (name, r[:3])
            assert r[3] == want.output and (want.status != OK or r[4] == zlib.adler32(want.output)), name
        else:
            assert r[:5] == whole[k][:5], (name, len(plan[0]), r[:3], whole[k][:3])
    for k in (1, len(plans) // 2, len(plans) - 1):
        assert run_single(eng, DE, plans[k]) == res[k], k
