"""The yardsticks of the packfile tests against git itself, on the CPU: the writer of tests/pack_writer.py writes what git
accepts, byte for byte down to the idx; the reader of tests/pack_model.py reads what git reads - types, bytes, depths - from
the writer's packs and from packs git pack-objects wrote; what the cases call malformed, git index-pack refuses; and the
list of cases holds every edge it is meant to hold.  Needs git (skipped where there is none); no device."""
import hashlib
import os
import shutil
import subprocess

import pytest

from tests import pack_cases as pc
from tests import pack_model as pm
from tests import pack_writer as pw

GIT = shutil.which("git")
needs_git = pytest.mark.skipif(GIT is None, reason="no git on this machine")
ENV = dict(os.environ, GIT_CONFIG_GLOBAL="/dev/null", GIT_CONFIG_SYSTEM="/dev/null", GIT_AUTHOR_NAME="a", GIT_AUTHOR_EMAIL="a@example.org",
           GIT_COMMITTER_NAME="a", GIT_COMMITTER_EMAIL="a@example.org", GIT_AUTHOR_DATE="1700000000 +0000", GIT_COMMITTER_DATE="1700000000 +0000")
TYPE_NAMES = {1: "commit", 2: "tree", 3: "blob", 4: "tag"}
# malformed cases that git index-pack accepts all the same, each with the reason (at most 3: the list must not hide a wrong model)
GIT_IS_MORE_LENIENT = {}


@pytest.fixture(scope="module")
def built():
    return [pc.build(c) for c in pc.cases()]


def _git(cwd, *args, **kw):
    return subprocess.run([GIT] + list(args), cwd=cwd, env=ENV, capture_output=True, **kw)


def _index_pack(tmp, pack):
    """git index-pack over a copy of the pack -> (the process, the idx it wrote or None)"""
    path = os.path.join(tmp, "t.pack")
    with open(path, "wb") as f:
        f.write(pack)
    idx = os.path.join(tmp, "t.idx")
    if os.path.exists(idx):
        os.remove(idx)
    r = _git(tmp, "index-pack", "-o", idx, path)
    return r, (open(idx, "rb").read() if r.returncode == 0 and os.path.exists(idx) else None)


def _repo_with(tmp, pack, idx):
    repo = os.path.join(tmp, "repo.git")
    shutil.rmtree(repo, ignore_errors=True)
    assert _git(tmp, "init", "-q", "--bare", repo).returncode == 0
    stem = os.path.join(repo, "objects", "pack", "pack-" + pack[-20:].hex())
    for ext, data in ((".pack", pack), (".idx", idx)):
        with open(stem + ext, "wb") as f:
            f.write(data)
    return repo, stem


def _cat_all(repo, names):
    """git cat-file --batch -> [(type name, bytes)]"""
    r = _git(repo, "cat-file", "--batch", input=b"".join(n.hex().encode() + b"\n" for n in names))
    assert r.returncode == 0, r.stderr
    out, at = [], 0
    for n in names:
        eol = r.stdout.index(b"\n", at)
        name, type_, size = r.stdout[at:eol].split(b" ")
        assert name == n.hex().encode()
        out.append((type_.decode(), r.stdout[eol + 1:eol + 1 + int(size)]))
        at = eol + 1 + int(size) + 1
    return out


def _verify_depths(repo, stem):
    r = _git(repo, "verify-pack", "-v", stem + ".idx")
    assert r.returncode == 0, r.stderr
    depth = {}
    for line in r.stdout.decode().split("\n"):
        w = line.split()
        if len(w) >= 5 and len(w[0]) == 40 and w[1] in TYPE_NAMES.values():
            depth[bytes.fromhex(w[0])] = int(w[5]) if len(w) >= 7 else 0
    return depth


def _model_equals_git(tmp, pack, idx, label):
    m = pm.Model(pack, idx)
    assert m.rc == pm.OK and m.info["failed"] == 0, label
    repo, stem = _repo_with(tmp, pack, idx)
    names = [o["name"] for o in m.objects]
    got = m.read()
    if names:
        depth = _verify_depths(repo, stem)
        for o, (st, data), (gt, gd) in zip(m.objects, got, _cat_all(repo, names)):
            assert st == pm.OK and (TYPE_NAMES[o["type"]], data) == (gt, gd), (label, o["name"].hex())
            assert o["depth"] == depth[o["name"]] and o["size"] == len(gd), (label, o["name"].hex())
            assert pw.object_name(o["type"], data) == o["name"], label
    return m


@needs_git
def test_well_formed_cases_are_gits_too(built, tmp_path):
    tmp = str(tmp_path)
    seen = unread = 0
    for c in built:
        if not c["well"]:
            continue
        r, idx = _index_pack(tmp, c["pack"])
        assert r.returncode == 0, (c["name"], r.stderr)
        assert idx == c["idx"], c["name"]  # byte for byte: names, CRC-32s, offsets, both checksums
        if c["git_reads"]:
            m = _model_equals_git(tmp, c["pack"], c["idx"], c["name"])
        else:
            unread += 1
            m = pm.Model(c["pack"], c["idx"])
            assert [(st, pw.object_name(o["type"], data)) for o, (st, data) in zip(m.objects, m.read())] == [(0, o["name"]) for o in m.objects]
        for k, lay in enumerate(c["layout"]):  # and the writer's own word on its entries
            o = m.objects[c["order"][k]]
            assert (o["name"], o["type"], o["offset"], o["packed_len"]) == (lay["name"], lay["type"], lay["offset"], lay["packed_len"]), c["name"]
        seen += 1
    assert seen >= 15 and unread <= 1


@needs_git
def test_malformed_cases_are_refused_by_git(built, tmp_path):
    assert len(GIT_IS_MORE_LENIENT) <= 3
    seen = 0
    for c in built:
        if c["well"] or c["idx_only"]:
            continue
        r, _ = _index_pack(str(tmp_path), c["pack"])
        assert (r.returncode != 0) == (c["name"] not in GIT_IS_MORE_LENIENT), (c["name"], r.stderr)
        seen += 1
    assert seen >= 25


def test_the_model_reads_every_case_as_the_case_says(built):
    for c in built:
        m = pm.Model(c["pack"], c["idx"])
        assert m.rc == c["rc"], c["name"]
        if m.rc != pm.OK:
            continue
        for verify in (False, True):
            got = m.read(None, verify)
            want = c.get("verify", c["expect"]) if verify else c["expect"]
            for k, lay in enumerate(c["layout"]):
                st, data = got[c["order"][k]]
                assert st == want.get(k, pm.OK), (c["name"], k, verify)
                if st == pm.OK:
                    assert lay["data"] is not None and data == lay["data"], (c["name"], k)
        assert (not c["well"]) == bool(c["expect"] or c.get("verify") or c["rc"] or c["idx_only"]), c["name"]
        assert pm.DECODER_ERROR not in [o["status"] for o in m.objects]


def test_the_cases_hold_every_edge():
    cases = pc.cases()
    assert len({c["name"] for c in cases}) == len(cases)
    held = set().union(*[c["edges"] for c in cases])
    assert pc.REQUIRED_EDGES <= held, pc.REQUIRED_EDGES - held
    for c in cases:
        if c["claim"]:
            assert c["claim"](pc.build(c)), c["name"]
    # edges the bytes themselves show
    b = {c["name"]: pc.build(c) for c in cases}
    m = pm.Model(b["a chain of 64, OFS and REF mixed"]["pack"], b["a chain of 64, OFS and REF mixed"]["idx"])
    assert sorted(o["depth"] for o in m.objects) == list(range(65))
    kinds = {(b["a chain of 64, OFS and REF mixed"]["pack"][o["offset"]] >> 4) & 7 for o in m.objects}
    assert kinds == {3, 6, 7}
    m = pm.Model(b["a fan of 1000"]["pack"], b["a fan of 1000"]["idx"])
    assert m.info["deltas"] == 1000 and m.info["max_depth"] == 1
    c = b["copy to the base's end"]
    assert c["entries"][1]["ins"][0][1] + c["entries"][1]["ins"][0][2] == len(pc.MID)
    c = b["copy one past the base's end"]
    assert c["entries"][1]["ins"][0][1] + c["entries"][1]["ins"][0][2] == len(pc.MID) + 1
    c = b["size varints of 1 to 5 bytes"]
    for k in range(1, 6):
        e = c["entries"][k]
        assert pw.leb128(100, e["size_bytes"]) == bytes([100 | 0x80] + [0x80] * (k - 2) + [0]) if k > 1 else pw.leb128(100, 1) == b"d"
    assert len(b["an empty pack"]["pack"]) == 32 and pm.Model(b["an empty pack"]["pack"], b["an empty pack"]["idx"]).info["n"] == 0
    ins = b["instruction counts around the window"]["entries"]
    assert pc.W == 64 and [len(e["ins"]) for e in ins[1:]] == [63, 64, 65, 127, 129]


def test_index_cases_in_the_model():
    cases, pack, layout = pc.index_cases()
    refusals = {label for label, _, want in cases if want != pm.OK}
    for word in ("fan-out that decreases", "do not ascend", "fan-out bucket", "escape outside", "too short", "left over", "version 1", "version 3"):
        assert any(word in r for r in refusals), word
    for label, blob, want in cases:
        st, ent, info = pm.read_idx(blob)
        assert st == want, label
        if st == pm.OK:
            assert info["has64"] == int("64-bit" in label) and info["pack_checksum"] == pack[-20:]
            assert [(n, o) for n, o, _ in ent] == sorted((x["name"], x["offset"]) for x in layout)


def _version_chains(repo, files, versions):
    import random
    rng = random.Random(5)
    cur = {f: ["line %d of %s %s" % (k, f, "".join(rng.choice("abcdef ") for _ in range(30))) for k in range(80)] for f in files}
    for v in range(versions):
        for f, lines in cur.items():
            lines[rng.randrange(len(lines))] = "edited in version %d" % v
            lines.insert(rng.randrange(len(lines)), "added in version %d" % v)
            with open(os.path.join(repo, f), "w") as g:
                g.write("\n".join(lines) + "\n")
        assert _git(repo, "add", "-A").returncode == 0
        assert _git(repo, "commit", "-q", "-m", "version %d" % v).returncode == 0


@needs_git
def test_the_model_reads_packs_git_wrote(tmp_path):
    repo = str(tmp_path / "work")
    os.mkdir(repo)
    assert _git(repo, "init", "-q", "-b", "main").returncode == 0
    _version_chains(repo, ["a.txt", "b.txt", "c.txt"], 8)
    names = _git(repo, "rev-list", "--objects", "--all").stdout.decode().split("\n")
    names = ("\n".join(n.split(" ")[0] for n in names if n) + "\n").encode()
    for label, flags in (("REF_DELTA", []), ("OFS_DELTA", ["--delta-base-offset"])):
        stem = str(tmp_path / label)
        r = _git(repo, "pack-objects", "--window=10", "--depth=6", *flags, stem, input=names)
        assert r.returncode == 0, r.stderr
        sha = r.stdout.decode().strip()
        pack = open("%s-%s.pack" % (stem, sha), "rb").read()
        idx = open("%s-%s.idx" % (stem, sha), "rb").read()
        m = _model_equals_git(str(tmp_path), pack, idx, label)
        assert m.info["n"] == 8 * (1 + 1 + 3)  # (a commit, a tree and three blobs a version)
        assert m.info["deltas"] >= 10 and m.info["max_depth"] >= 3
        kinds = {(pack[o["offset"]] >> 4) & 7 for o in m.objects if o["link"]}
        assert kinds == ({6} if flags else {7}), label
        assert hashlib.sha1(pack[:-20]).digest() == pack[-20:] and hashlib.sha1(idx[:-20]).digest() == idx[-20:]
