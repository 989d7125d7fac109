"""csrc/bgzf_index.hpp (md::bgzf::from_gzi / to_gzi, the .gzi loader of md_bgzf_index_from_gzi) under AddressSanitizer and
UBSan, as a stand-alone host program (bgzf_index_check.cpp, nothing preloaded, no device): the good blob of a file of twelve
members, every truncation of it, every other value of every byte of its count and of its first two entries, and the good
blob against every truncation of the file - each verdict, and the table behind every accepted blob, against a model of the
rules written here from mdeflate.h."""
import os
import shutil
import struct
import subprocess

import pytest

from tests import gz_members_util as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD = 0, 21
TEXT = b"".join(b"record %d\tsome fields\t%d\n" % (k, k * k) for k in range(120))


def _member_at(src, p):
    """length of the indexed member at src[p], 0 if none (BC anywhere in the extra field)"""
    if len(src) - p < 28 or src[p:p + 3] != b"\x1f\x8b\x08" or src[p + 3] & 0xe4 != 4:
        return 0
    xlen = struct.unpack_from("<H", src, p + 10)[0]
    if len(src) - p - 12 < xlen:
        return 0
    q = 0
    while q + 4 <= xlen:
        si, sl = src[p + 12 + q:p + 14 + q], struct.unpack_from("<H", src, p + 14 + q)[0]
        if q + 4 + sl > xlen:
            return 0
        if si == b"BC" and sl == 2:
            m = struct.unpack_from("<H", src, p + 16 + q)[0] + 1
            return 0 if m < 12 + xlen + 10 or m > len(src) - p else m
        q += 4 + sl
    return 0


def model(blob, src):
    """-> (status, [(c_off, u_off)] of M + 1 pairs or None)"""
    if len(blob) < 8:
        return BAD, None
    n = struct.unpack_from("<Q", blob)[0]
    if len(blob) != 8 + 16 * n:
        return BAD, None
    tab = [(0, 0)]
    for k in range(n):
        c, u = struct.unpack_from("<QQ", blob, 8 + 16 * k)
        if c <= tab[-1][0] or c >= len(src) or u < tab[-1][1] or (u - tab[-1][1]) // 1032 > c - tab[-1][0]:
            return BAD, None
        tab.append((c, u))
    p, u = tab[-1]
    walked = 0
    while p < len(src):
        if src[p] == 0 and walked:
            if src[p:].strip(b"\0"):
                return BAD, None
            break
        m = _member_at(src, p)
        if not m:
            return BAD, None
        if walked:
            tab.append((p, u))
        u += struct.unpack_from("<I", src, p + m - 4)[0]
        if u >> 64:
            return BAD, None
        p += m
        walked += 1
    if walked:
        tab.append((p, u))
    return OK, tab


def _gzi(pairs):
    return struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", c, u) for c, u in pairs)


def test_gzi_loader_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "bgzf_index_check"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "decompress_amd", "csrc"), os.path.join(ROOT, "tests", "bgzf_index_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler cannot link the sanitizers")
    assert r.returncode == 0, r.stderr
    f, idx = gu.bgzf_file(TEXT, block=300)
    assert len(idx) == 12
    blob = _gzi(idx[1:])
    assert model(blob, f) == (OK, idx + [(len(f), len(TEXT))])
    cases = [("T", 0, n, 0) for n in range(len(blob) + 1)]
    cases += [("M", 0, pos, v) for pos in range(8 + 32) for v in range(256) if v != blob[pos]]
    cases += [("C", n, 0, 0) for n in range(len(f) + 1)]
    path = tmp_path / "cases.txt"
    with open(path, "w") as out:
        out.write("S %s\nB %s\n" % (f.hex(), blob.hex()))
        for kind, a, b, v in cases:
            out.write({"T": "T %d %d\n" % (a, b), "M": "M %d %d %d\n" % (a, b, v), "C": "C %d\n" % a}[kind])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    counts = {OK: 0, BAD: 0}
    for (kind, a, b, v), line in zip(cases, lines):
        g = blob[:b] if kind == "T" else blob[:b] + bytes([v]) + blob[b + 1:] if kind == "M" else blob
        src = f[:a] if kind == "C" else f
        st, tab = model(g, src)
        got = line.split()
        assert int(got[0]) == st, (kind, a, b, v, line)
        counts[st] += 1
        if st == OK:
            assert (int(got[1]), int(got[2])) == (len(tab) - 1, tab[-1][1]), (kind, a, b, v, line)
            assert bytes.fromhex(got[3]) == _gzi(tab[1:-1]), (kind, a, b, v)
        else:
            assert got[1:] == ["0", "0", "-"]
    print(counts)
    # (both answers occur often: a loader that says one thing everywhere cannot pass)
    assert counts[OK] >= 50 and counts[BAD] >= 5000, counts
