"""csrc/pack_write.hpp - the table's size, where the tables of a batch's bases go, the header and distance bytes, the keep rule, the walk over the offsets and the
bound - under AddressSanitizer and UBSan, as a stand-alone host program (pack_write_check.cpp, nothing preloaded, no
device), against the model's numbers (tests/pack_delta_model.py, tests/pack_writer.py) for the same inputs: the values at
which a varint grows, every pack of tests/pack_write_cases.py as the model laid it out, and keep rules over made-up chains."""
import os
import random
import shutil
import subprocess

import pytest

from tests import pack_delta_model as dm
from tests import pack_write_cases as wc
from tests import pack_writer as pw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lines():
    """[(line, expected output)]"""
    out = []
    for blocks in (0, 1, 511, 512, 513, 1024, 1025, 1 << 20, (1 << 20) + 1, (1 << 28) - 1):
        out.append(("T %d" % blocks, "%d" % dm.table_bits(blocks)))
    # the tables of a batch's distinct bases, in the order they are added: test_gpu_pack_write.test_one_plan_from_two_routes'
    # bases as the delta batch meets them and as the search does, and bases at which a table grows
    for lens in ([716, 716, 648, 15, 16], [716, 716, 648], [], [15], [16], [15, 31, 32, 0, 47], [8207, 8208, 15, 16400, 1 << 20, 0xFFFFFFF0, 16]):
        blocks = words = 0
        places = []
        for n in lens:
            nb = n // dm.BLOCK
            places.append(" %d:%d:%d" % ((words, blocks, dm.table_bits(nb)) if nb else (0, 0, 0)))
            blocks, words = blocks + nb, words + ((1 << dm.table_bits(nb)) if nb else 0)
        out.append(("P %d %s" % (len(lens), " ".join(map(str, lens))), "%d %d" % (blocks, words) + "".join(places)))
    sizes = [0, 1, 15, 16, 2047, 2048, (1 << 18) - 1, 1 << 18, (1 << 25) - 1, 1 << 25, 0xFFFFFFF0, (1 << 64) - 1]
    for t in (1, 2, 3, 4, 6):
        for s in sizes:
            out.append(("H %d %d" % (t, s), pw.object_header(t, s).hex()))
    for v in (1, 127, 128, 16511, 16512, 2113663, 2113664, (1 << 32) - 1, 1 << 32, (1 << 63), (1 << 64) - 1):
        out.append(("O %d" % v, pw.ofs_varint(v).hex()))
    for lens in ([], [0], [1, 7, 8, 9], [0xFFFFFFF0], [0xFFFFFFF0] * 3, [0xFFFFFFF1], [5, 0xFFFFFFF1]):
        want = 0 if any(n > 0xFFFFFFF0 for n in lens) else dm.write_bound(lens)
        out.append(("B %d %s" % (len(lens), " ".join(map(str, lens))), "%d" % want))
    rng = random.Random(7)
    rules = [([None, 0, 1, 2, 3], [0, 1, 1, 1, 1], [0, 1, 1, 1, 1], d) for d in (0, 1, 2, 3, 4, 5)]
    rules.append(([None, 0, 1, 2, 3], [0, 1, 1, 1, 1], [0, 1, 0, 1, 1], 2))
    rules.append(([], [], [], 3))
    for _ in range(200):
        n = rng.randrange(1, 40)
        bases = [None if i == 0 or rng.random() < 0.2 else rng.randrange(i) for i in range(n)]
        tried = [int(b is not None and rng.random() < 0.9) for b in bases]
        fitted = [int(t and rng.random() < 0.8) for t in tried]
        rules.append((bases, tried, fitted, rng.choice((0, 1, 2, 3, 50))))
    for bases, tried, fitted, max_depth in rules:
        keep, depth, c = dm.keep_rule(bases, tried, fitted, max_depth)
        line = "K %d %d %s" % (max_depth, len(bases), " ".join("%d %d %d" % (-1 if b is None else b, t, f) for b, t, f in zip(bases, tried, fitted)))
        want = "%d %d %d" % (c["kept"], c["dropped_size"], c["dropped_depth"]) + "".join(" %d:%d" % (k, d) for k, d in zip(keep, depth))
        out.append((line, want))
    for c in wc.pack_cases():
        for r in wc.pack_model(c["name"], 6):
            n = len(c["objects"])
            bases = c["bases"]
            offs = [e["offset"] for e in r["entries"]] + [len(r["pack"]) - 20]
            rows, heads = [], []
            for i in range(n):
                head = pw.object_header(6 if r["keep"][i] else c["objects"][i][0], len(r["payloads"][i]))
                if r["keep"][i]:
                    head += pw.ofs_varint(offs[i] - offs[bases[i]])
                assert r["pack"][offs[i]:offs[i] + len(head)] == head
                zlen = offs[i + 1] - offs[i] - len(head)
                rows.append("%d %d %d %d %d" % (c["objects"][i][0], len(r["payloads"][i]), -1 if bases[i] is None else bases[i], r["keep"][i], zlen))
                heads.append(" %d:%s" % (offs[i], head.hex()))
            out.append(("W %d %s" % (n, " ".join(rows)), "%d" % offs[n] + "".join(heads)))
    # a walk whose offsets pass 2^32 and whose distances need five bytes
    n, z = 6, (1 << 31) + 12345
    offs = [12]
    heads = []
    for i in range(n):
        head = pw.object_header(6 if i else 3, 1000 + i) + (pw.ofs_varint(offs[i] - offs[0]) if i else b"")
        heads.append(" %d:%s" % (offs[i], head.hex()))
        offs.append(offs[i] + len(head) + z)
    out.append(("W %d %s" % (n, " ".join("3 %d %d %d %d" % (1000 + i, 0 if i else -1, 1 if i else 0, z) for i in range(n))), "%d" % offs[n] + "".join(heads)))
    return out


def test_host_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "pack_write_check"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "decompress_amd", "csrc"), os.path.join(ROOT, "tests", "pack_write_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler cannot link the sanitizers")
    assert r.returncode == 0, r.stderr
    lines = _lines()
    path = tmp_path / "cases.txt"
    path.write_text("".join(line + "\n" for line, _ in lines))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = r.stdout.splitlines()
    assert len(got) == len(lines) > 300
    for (line, want), g in zip(lines, got):
        assert g == want, line[:200]
