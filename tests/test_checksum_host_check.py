"""The host checksums of csrc/host_util.hpp - md::adler32_update, md::crc32_update, md::crc32_concat - under AddressSanitizer
and UBSan, as a stand-alone host program (checksum_check.cpp, nothing preloaded, no device), on the texts of
tests/checksum_cases.py.  The streaming shims, the gzip-member readers, the inflate index and the long-stream path compute
their checksums with these.

Yardsticks: zlib.adler32 and zlib.crc32 with the seed where there is one.  crc32_concat with a len_b no buffer can have is
checked three ways: against zlib on zero runs of up to 4 MiB, against the program's own crc32_update chained over as many
zero bytes, and by concat(concat(a, z1, n1), z2, n2) == concat(a, z12, n1 + n2) with the CRCs of zero runs doubled from a
zlib value - and against crc(A) x^(8 n) mod P xor crc(B) worked out here with Python integers (a reference that is itself
compared with zlib first)."""
import os
import random
import shutil
import subprocess
import zlib

import pytest

from tests import checksum_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POLY = 0x104c11db7
CONCAT_LENS = [0, 1] + [1 << k for k in range(1, 41)] + [(1 << 32) - 1, 65521]
MIB = 1 << 20


def _build(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "checksum_check"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "decompress_amd", "csrc"), os.path.join(ROOT, "tests", "checksum_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler cannot link the sanitizers")
    assert r.returncode == 0, r.stderr
    return exe


# ---- crc(A || B) with Python integers ---------------------------------------------------------------------------------------
def _rev32(v):
    return int(format(v, "032b")[::-1], 2)


def _mulmod(a, b):
    """a b mod P in GF(2)[x], bit k = x^k"""
    p = 0
    while b:
        if b & 1:
            p ^= a
        b >>= 1
        a <<= 1
        if a >> 32:
            a ^= POLY
    return p


def concat_ref(crc_a, crc_b, len_b):
    """a CRC-32 value read bit 31 = x^0 is a polynomial; crc(A || B) = crc(A) x^(8 |B|) mod P xor crc(B)"""
    r, sq, n = 1, 1 << 8, len_b
    while n:
        if n & 1:
            r = _mulmod(r, sq)
        sq = _mulmod(sq, sq)
        n >>= 1
    return _rev32(_mulmod(_rev32(crc_a), r)) ^ crc_b


def test_the_python_reference_is_zlibs():
    rng = random.Random(11)
    for n in (0, 1, 2, 3, 7, 8, 9, 255, 256, 65521, 100000):
        a, b = rng.randbytes(rng.randrange(0, 50)), rng.randbytes(n)
        assert concat_ref(zlib.crc32(a), zlib.crc32(b), n) == zlib.crc32(a + b)
    for n in (1, 65521, 65536, 4 * MIB):
        assert concat_ref(0xdeadbeef, zlib.crc32(bytes(n)), n) == zlib.crc32(bytes(n), 0xdeadbeef)


def _zero_crc(n):
    """the CRC-32 of n zero bytes, from zlib up to 4 MiB and by the reference beyond"""
    z, have = zlib.crc32(bytes(min(n, 4 * MIB))), min(n, 4 * MIB)
    while have < n:
        k = min(have, n - have)
        z = concat_ref(z, _zero_crc(k) if k != have else z, k)
        have += k
    return z


def test_host_checksums_under_sanitizers(tmp_path):
    exe = _build(tmp_path)
    blob, index, lines, want = bytearray(), {}, [], []

    def put(data):
        if data not in index:
            index[data] = len(blob)
            blob.extend(data)
        return index[data]

    def ask(line, *expect):
        lines.append(line)
        want.extend("%08x" % e for e in expect)

    # ---- adler32_update: every text, seeds, pieces
    texts = cc.top_texts() + [("slice-top", cc.slice_top())] + cc.unit_texts() + cc.one_hot() + cc.forged_texts()
    texts += [("lengths", cc.lengths_text()), ("random-65537", cc.long_random(65537)), ("zero-65537", cc.long_zero(65537)), ("empty", b"")]
    for name, t in texts:
        ask("A 1 %x %x 0" % (put(t), len(t)), zlib.adler32(t))
    ff = b"\xff" * max(cc.FF_RUNS)
    put(ff)
    for name, seed, d in cc.seeded():
        off = put(d) if len(d) == 70000 else index[ff]
        ask("A %x %x %x 0" % (seed, off, len(d)), zlib.adler32(d, seed))
    top = cc.top(70000)
    for piece in (1, 4095, 4096, 4097, 5552, 65536, 65537):  # the second piece of 65536 starts in state (65520, 65520)
        ask("P 1 %x %x %x" % (put(top), len(top), piece), zlib.adler32(top))
        ask("Q 0 %x %x %x" % (put(top), len(top), piece), zlib.crc32(top))
    for seed in cc.SEEDS:
        ask("P %x %x %x 1" % (seed, index[ff], 5553), zlib.adler32(ff[:5553], seed))
    # ---- crc32_update: every prefix of the 8400 bytes at shifts 0 .. 7 of its block, seeded, in pieces, every split point
    t = cc.lengths_text()
    _, crcs = cc.prefix_sums()
    for k in range(len(t) + 1):
        ask("C 0 %x %x %x" % (put(t), k, k % 8), crcs[k])
    for name, d in cc.forged_texts() + cc.forged_embedded_texts() + [("zero-65537", cc.long_zero(65537))]:
        ask("C 0 %x %x 3" % (put(d), len(d)), zlib.crc32(d))
        ask("C %x %x %x 5" % (0xffffffff, put(d), len(d)), zlib.crc32(d, 0xffffffff))
    msg = t[1000:1130]
    ask("S %x %x" % (index[t] + 1000, 130), *[zlib.crc32(msg)] * 131)
    # ---- crc32_concat
    rng = random.Random(12)
    a_bytes = rng.randbytes(77)
    crc_a = zlib.crc32(a_bytes)
    forged0 = cc.forged(1000, 0)
    for n in CONCAT_LENS:
        for ca in (crc_a, 0, 0xffffffff, zlib.crc32(forged0)):
            for cb in (0, 0x12345678):
                ask("K %x %x %x" % (ca, cb, n), concat_ref(ca, cb, n))
    for n in (0, 1, 2, 65521, 65536, 100000):  # real second halves
        b_bytes = rng.randbytes(n)
        ask("K %x %x %x" % (crc_a, zlib.crc32(b_bytes), n), zlib.crc32(a_bytes + b_bytes))
    # crc(A || 0^n) three ways: zlib, crc32_update chained over zero blocks, crc32_concat
    for n in (1, 65535, 65536, 65537, MIB - 1, MIB, MIB + 1, 4 * MIB):
        z = zlib.crc32(bytes(n))
        ask("Z %x %x" % (crc_a, n), zlib.crc32(bytes(n), crc_a))
        ask("K %x %x %x" % (crc_a, z, n), zlib.crc32(bytes(n), crc_a))
        ask("Z 0 %x" % n, z)
    # the CRC of a zero run, doubled from zlib's value of 1 MiB up to 2^40 bytes: 1 MiB 2^k, k = 1 .. 20
    z_mib = zlib.crc32(bytes(MIB))
    doubled = [_zero_crc(MIB << k) for k in range(1, 21)]
    assert doubled[0] == zlib.crc32(bytes(2 * MIB)) and doubled[1] == zlib.crc32(bytes(4 * MIB))
    ask("W %x %x %x" % (z_mib, MIB, 20), *doubled)
    # ... and associativity with them: n1 + n2 a power of two, across 2^32, and odd lengths
    z = {MIB << k: v for k, v in enumerate([z_mib] + doubled)}
    pairs = [(n, n) for n in (MIB, 1 << 31, 1 << 32, 1 << 39)] + [((1 << 32) - MIB, MIB), (MIB, (1 << 32) - MIB)]
    for n1, n2 in pairs:
        z1, z2 = z.get(n1, _zero_crc(n1)), z.get(n2, _zero_crc(n2))
        z12 = z.get(n1 + n2, _zero_crc(n1 + n2))
        for ca in (crc_a, 0xffffffff):
            both = concat_ref(ca, z12, n1 + n2)
            ask("J %x %x %x %x %x" % (ca, z1, n1, z2, n2), both)
            ask("K %x %x %x" % (ca, z12, n1 + n2), both)
    for n1, n2 in (((1 << 32) - 1, 1), (65521, (1 << 32) - 1), (65521, 65521)):
        z1, z2, z12 = _zero_crc(n1), _zero_crc(n2), _zero_crc(n1 + n2)
        ask("J %x %x %x %x %x" % (crc_a, z1, n1, z2, n2), concat_ref(crc_a, z12, n1 + n2))
        ask("K %x %x %x" % (crc_a, z12, n1 + n2), concat_ref(crc_a, z12, n1 + n2))

    cases, data = tmp_path / "cases.txt", tmp_path / "bytes.bin"
    cases.write_text("\n".join(lines) + "\n")
    data.write_bytes(bytes(blob))
    r = subprocess.run([str(exe), str(cases), str(data)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want) > 9000
    at = 0
    for line in lines:  # (a line has one answer, S and W more)
        k = 131 if line[0] == "S" else 20 if line[0] == "W" else 1
        assert got[at:at + k] == want[at:at + k], (line, got[at:at + k][:3], want[at:at + k][:3])
        at += k
