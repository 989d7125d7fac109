"""csrc/gz_frame.hpp (md::gz::inf_header, Gz.Inf's header walk on the host) under AddressSanitizer and UBSan, as a stand-alone
host program (gz_frame_check.cpp, nothing preloaded, no device), against the CPU oracle's Gz.Inf: two frames of about 50
bytes - name, comment and header CRC; the same with an extra field, put in by hand as the reference reads it (XLEN
big-endian, the CRC over the fixed bytes, name and comment alone) - each cut at every length and with every byte in front of
its body set to every other value."""
import os
import shutil
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, END_OF_INPUT, BAD_HEADER, BAD_HEADER_CRC = 0, 1, 10, 11
DATA = b"some text, some text, some text"
EXTRA = b"\x01\x02extra"
FIELDS = ("st", "body", "extra_off", "extra_len", "name_off", "name_len", "comment_off", "comment_len", "flg", "mtime", "xfl", "os")


def _frames(oracle):
    a = oracle.gz_deflate(DATA, name=b"nm", comment=b"cm", hcrc=True)
    g = oracle.gz_deflate(DATA, name=b"nm", comment=b"cm", hcrc=False)
    assert g[3] == 8 | 16 and g[10:16] == b"nm\0cm\0" and len(EXTRA) == 7
    fixed = g[:3] + bytes([g[3] | 4 | 2]) + g[4:10]
    crc16 = (zlib.crc32(fixed + g[10:16]) >> 16).to_bytes(2, "big")
    b = fixed + len(EXTRA).to_bytes(2, "big") + EXTRA + g[10:16] + crc16 + g[16:]
    return (a, 18), (b, 27)


def _cases(frames):
    cases = []
    for k, (frame, body) in enumerate(frames):
        cases += [("T", k, n, 0) for n in range(len(frame) + 1)]
        cases += [("M", k, pos, v) for pos in range(body) for v in range(256) if v != frame[pos]]
    return cases


def test_header_walk_under_sanitizers_against_the_oracle(tmp_path, oracle):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "gz_frame_check"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "decompress_amd", "csrc"), os.path.join(ROOT, "tests", "gz_frame_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler cannot link the sanitizers")
    assert r.returncode == 0, r.stderr
    frames = _frames(oracle)
    cases = _cases(frames)
    for k, (frame, body) in enumerate(frames):
        assert sum(c[1] == k for c in cases) == len(frame) + 1 + 255 * body == (4633, 6937)[k]
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for frame, _ in frames:
            f.write("B %s\n" % frame.hex())
        for kind, k, a, v in cases:
            f.write("M %d %d %d\n" % (k, a, v) if kind == "M" else "T %d %d\n" % (k, a))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = [dict(zip(FIELDS, (int(x) for x in line.split()))) for line in r.stdout.splitlines()]
    assert len(got) == len(cases)
    counts = [{OK: 0, END_OF_INPUT: 0, BAD_HEADER: 0, BAD_HEADER_CRC: 0} for _ in frames]
    for (kind, k, a, v), h in zip(cases, got):
        frame = frames[k][0]
        src = frame[:a] if kind == "T" else frame[:a] + bytes([v]) + frame[a + 1:]
        ost, _, out, meta = oracle.gz_inflate(src, len(DATA) + 16)
        counts[k][h["st"]] += 1
        if h["st"] != OK:
            assert ost == h["st"], (kind, k, a, v, h, ost)
            continue
        assert ost not in (BAD_HEADER, BAD_HEADER_CRC), (kind, k, a, v, h, ost)
        if src == frame:  # the whole frame: every field, and the body begins where the walk says
            assert ost == OK and out == DATA
            assert oracle.de_inflate(src[h["body"]:])[2] == DATA
            assert h["body"] == frames[k][1]
            assert src[h["name_off"]:h["name_off"] + h["name_len"]] == meta["name"] == b"nm"
            assert src[h["comment_off"]:h["comment_off"] + h["comment_len"]] == meta["comment"] == b"cm"
            extra = src[h["extra_off"]:h["extra_off"] + h["extra_len"]]
            assert (extra, meta["extra"]) == ((EXTRA, EXTRA) if k else (b"", None))
            assert (h["flg"], h["os"], h["mtime"], h["xfl"]) == (meta["flg"], meta["os"], meta["mtime"], meta["xfl"])
    print(counts)
    for c in counts:  # (all four answers occur: a walk that says one thing everywhere cannot pass)
        assert all(n >= 50 for n in c.values()), c
