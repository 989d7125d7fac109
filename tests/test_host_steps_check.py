"""md::running_offsets and md::adjacent_runs (csrc/host_util.hpp) under AddressSanitizer and UBSan, as a stand-alone host
program (host_steps_check.cpp, nothing preloaded, no device): the running sum of output offsets that md_zip_uncompress and
md_pack_read share, and the walk over the runs of ranges that leave by one copy at the end of md_inflate_index_read and
md_bgzf_read.  What the program prints is compared with the models below, written from the rules alone."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2 ** 64 - 1
OK, BAD = 0, -3


def _offsets(sizes):
    """[total, off_0 .. off_k]: a sum that does not fit 64 bits is 2^64 - 1 from there on."""
    offs, at = [], 0
    for s in sizes:
        offs.append(at)
        at = U64 if at + s > U64 else at + s
    return [at] + offs + [at]


def _runs(ranges):
    """(first, bytes) per longest run of consecutive ranges that succeeded, have bytes and are adjacent in dst."""
    runs, cur = [], None  # cur: [first, bytes, where the next range has to begin]
    for i, (status, length, dst) in enumerate(ranges):
        if status != OK or length == 0:
            cur = None
        elif cur is not None and dst == cur[2]:
            cur[1] += length
            cur[2] += length
        else:
            cur = [i, length, dst + length]
            runs.append(cur)
    return [(c[0], c[1]) for c in runs]


OFFSET_CASES = [
    [],                                  # k = 0
    [77],                                # one item
    [5, 0, 0, 9, 0, 1],                  # zero sizes among the others
    [U64 - 100, 50, 0, 49],              # reaches 2^64 - 2 exactly
    [U64 - 100, 50, 49, 2],              # overflows at the last item
    [1 << 63, 1 << 63, 5, 0, 1 << 63],   # overflows in the middle: the later offsets are the saturated value
]

RANGE_CASES = [
    [],                                                   # n = 0
    [(OK, 10, 3)],                                        # one good range
    [(BAD, 10, 0), (BAD, 4, 10), (1, 4, 14)],             # all failed
    [(OK, 10, 0), (OK, 6, 10)],                           # adjacent: one run
    [(OK, 10, 0), (OK, 6, 11)],                           # a gap
    [(OK, 10, 6), (OK, 6, 0)],                            # reverse order in dst
    [(OK, 10, 0), (BAD, 5, 10), (OK, 6, 10)],             # a failed range between two adjacent ones: two runs
    [(OK, 10, 0), (OK, 0, 10), (OK, 6, 10)],              # a range of no bytes between two adjacent ones: two runs
    [(OK, 0, 0), (OK, 10, 0), (OK, 6, 10), (OK, 0, 16)],  # a leading and a trailing range of no bytes
    [(OK, 0, 5), (BAD, 0, 5), (OK, 0, 5)],                # nothing but ranges of no bytes
    [(OK, 3, 3 * i) if i % 2 == 0 else (BAD, 3, 3 * i) for i in range(4099)],  # alternating good and failed
    [(OK, 3, 3 * i) for i in range(4099)],                # one long run
]


def test_models():
    """the models against answers worked out by hand"""
    assert _offsets([5, 0, 9]) == [14, 0, 5, 5, 14]
    assert _offsets(OFFSET_CASES[3])[0] == U64 - 1
    assert _offsets(OFFSET_CASES[4]) == [U64, 0, U64 - 100, U64 - 50, U64 - 1, U64]
    assert _offsets(OFFSET_CASES[5]) == [U64, 0, 1 << 63, U64, U64, U64, U64]
    assert _runs(RANGE_CASES[3]) == [(0, 16)]
    assert _runs(RANGE_CASES[5]) == [(0, 10), (1, 6)]
    assert _runs(RANGE_CASES[6]) == [(0, 10), (2, 6)]
    assert _runs(RANGE_CASES[7]) == [(0, 10), (2, 6)]
    assert _runs(RANGE_CASES[8]) == [(1, 16)]
    assert _runs(RANGE_CASES[10]) == [(i, 3) for i in range(0, 4099, 2)]
    assert _runs(RANGE_CASES[11]) == [(0, 3 * 4099)]


def test_host_steps_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    flags = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # an empty program first: only a compiler that cannot link the sanitizers at all is a reason to skip
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler cannot link the sanitizers")
    exe = tmp_path / "host_steps_check"
    cmd = [cxx] + flags + ["-I", os.path.join(ROOT, "decompress_amd", "csrc"), os.path.join(ROOT, "tests", "host_steps_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    path = tmp_path / "cases.txt"
    want = []
    with open(path, "w") as f:
        for sizes in OFFSET_CASES:
            f.write("O %d %s\n" % (len(sizes), " ".join(str(s) for s in sizes)))
            want.append(["O"] + [str(v) for v in _offsets(sizes)])
        for ranges in RANGE_CASES:
            f.write("R %d %s\n" % (len(ranges), " ".join("%d %d %d" % t for t in ranges)))
            want.append(["R"] + [str(v) for run in _runs(ranges) for v in run])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert [line.split() for line in r.stdout.splitlines()] == want
