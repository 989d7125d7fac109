"""csrc/sha1_host.hpp under AddressSanitizer and UBSan, as a stand-alone host program (sha1_check.cpp, nothing preloaded,
no device): the block step, the host SHA-1 and the formatter of a git object's header - the same text the kernel of
csrc/sha1_kernels.hip runs.  Yardsticks: the FIPS 180 vectors as printed in the standard's examples, hashlib, and Python's
own formatting of "<type> <size>\\0"."""
import hashlib
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPE_NAMES = {1: b"commit", 2: b"tree", 3: b"blob", 4: b"tag"}
FIPS = [
    (b"", "da39a3ee5e6b4b0d3255bfef95601890afd80709"),
    (b"abc", "a9993e364706816aba3e25717850c26c9cd0d89d"),
    (b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq", "84983e441c3bd26ebaae4aa1f95129e5e54670f1"),  # 448 bits
]
MILLION_A = "34aa973cd4c4daa4f61eeb2bdbad27316534016f"
# every digit count the device can meet: both sides of each power of ten, and the largest size the library takes
SIZES = [0, 9] + [v for k in range(1, 10) for v in (10 ** k - 1, 10 ** k)][1:] + [0xfffffff0]


def _message(n):
    return bytes((7 * i + n) & 0xff for i in range(n))


def _build(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "sha1_check"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "decompress_amd", "csrc"), os.path.join(ROOT, "tests", "sha1_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler cannot link the sanitizers")
    assert r.returncode == 0, r.stderr
    return exe


def test_host_sha1_under_sanitizers(tmp_path):
    exe = _build(tmp_path)
    lines, want = [], []
    for msg, digest in FIPS:
        lines.append("D 0 " + msg.hex())
        want.append(digest)
    lines.append("A 1000000")
    want.append(MILLION_A)
    for n in range(201):
        for t in range(5):
            msg = _message(n)
            lines.append("D %d %s" % (t, msg.hex()))
            head = TYPE_NAMES[t] + b" %d\0" % n if t else b""
            want.append(hashlib.sha1(head + msg).hexdigest())
    split = _message(130)
    lines.append("S " + split.hex())
    want += [hashlib.sha1(split).hexdigest()] * 131
    for t in range(1, 5):
        for size in SIZES:
            lines.append("H %d %d" % (t, size))
            head = TYPE_NAMES[t] + b" %d\0" % size
            want.append("%d %s" % (len(head), head.ljust(20, b"\0").hex()))
    lines.append("H 0 77")
    want.append("0 " + bytes(20).hex())
    lines.append("H 5 77")
    want.append("0 " + bytes(20).hex())
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want) > 1200
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, g, w)
    assert max(len(TYPE_NAMES[t]) + 1 + len(str(s)) + 1 for t in TYPE_NAMES for s in SIZES) == 18
    assert sorted({len(str(s)) for s in SIZES}) == list(range(1, 11))
