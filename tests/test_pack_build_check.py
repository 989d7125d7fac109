"""csrc/pack_build.hpp - the walk over the candidates and the idx writer - under AddressSanitizer and UBSan, as a stand-alone
host program (pack_build_check.cpp, nothing preloaded, no device): every pack of tests/pack_build_cases.py with the
candidates' table as the model computes it, that table cut short at several lengths, and with single entries bent.  The
program must end clean and say of every walk what a walk written here in Python says of the same table; over the whole
table that is what the model found by decoding."""
import os
import shutil
import subprocess

import pytest

from tests import pack_build_cases as bc
from tests import pack_build_model as bm
from tests import pack_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_OFFSET = (1 << 64) - 1


def _walk(pack, table):
    """the forward merge of mdeflate.h over `table` [(z, consumed, out_len, status)] -> (rc, bad_offset, bad_status, n)"""
    end, count = len(pack) - 20, int.from_bytes(pack[8:12], "big")
    at, k, n = 12, 0, 0
    while at < end:
        if n == count:
            return pm.INVALID_PACK, at, 0, n
        h = bm.parse_header(pack, at, end)
        if h is None:
            return pm.INVALID_PACK, at, 0, n
        z = h[2]
        while k < len(table) and table[k][0] < z:
            k += 1
        if k == len(table) or table[k][0] != z:
            return pm.INVALID_PACK, at, 0, n
        if table[k][3] != 0:
            return pm.INVALID_PACK, at, table[k][3], n
        if table[k][1] > end - z:
            return pm.INVALID_PACK, at, 0, n
        n += 1
        at = z + table[k][1]
    if n != count:
        return pm.INVALID_PACK, end, 0, n
    return pm.OK, NO_OFFSET, 0, n


def _tables():
    """[(pack number, table)] and the packs"""
    packs, walks = [], []
    for c in bc.cases():
        pack = c["pack"]
        if len(pack) < 32 or pack[:4] != b"PACK":
            continue
        if len(pack) > 100000 and "random" not in c["name"]:
            continue  # (the long text blobs add nothing here: the walk sees two objects)
        b = len(packs)
        packs.append((c["name"], pack))
        table = bm.candidate_table(pack)
        walks.append((b, table, True))
        C = len(table)
        for cut in sorted({0, 1, C // 2, C - 1} & set(range(C))):
            walks.append((b, table[:cut], False))
        for k in sorted({0, 1, C // 2, C - 1} & set(range(C))):
            z, used, out, st = table[k]
            for bent in ((z + 1, used, out, st), (z, used + 1, out, st), (z, max(used - 1, 0), out, st), (z, 0, out, st), (z, 1 << 63, out, st),
                         (z, NO_OFFSET, out, st), (z, used, out + 1, st), (z, used, out, 1), (1 << 62, used, out, st), (0, used, out, st)):
                walks.append((b, table[:k] + [bent] + table[k + 1:], False))
    return packs, walks


def test_walk_and_writer_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    exe = tmp_path / "pack_build_check"
    cmd = [cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "decompress_amd", "csrc"), os.path.join(ROOT, "tests", "pack_build_check.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and ("asan" in r.stderr or "ubsan" in r.stderr or "sanitize" in r.stderr):
        pytest.skip("the compiler cannot link the sanitizers")
    assert r.returncode == 0, r.stderr
    packs, walks = _tables()
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for _, pack in packs:
            f.write("P %s\n" % pack.hex())
        for b, table, _ in walks:
            f.write("W %d %d %s\n" % (b, len(table), " ".join("%d %d %d %d" % e for e in table)))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(walks) > 1000
    seen = set()
    for (b, table, whole), g in zip(walks, got):
        name, pack = packs[b]
        want = _walk(pack, table)
        assert g[:4] == want, (name, len(table), g, want)
        assert g[4] == (8 + 1024 + 28 * want[3] + 40 if want[0] == pm.OK else 0), name
        seen.add(want[0])
        if whole:  # the model walked with zlib itself
            m = bm.BuildModel(pack, False)
            if m.rc == pm.UNSUPPORTED:
                continue  # (a call-level refusal: the walk is never asked)
            walked = not (m.rc == pm.INVALID_PACK and m.n == 0)  # (an object's own MD_INVALID_PACK comes with n objects)
            assert (want[0] == pm.OK) == walked, name
            if want[0] == pm.OK:
                assert want[3] == m.n, name
            else:
                assert (want[1], want[2] != 0) == (m.bad_offset, m.bad_status != 0), name
    assert seen == {pm.OK, pm.INVALID_PACK}
