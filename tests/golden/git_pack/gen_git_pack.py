"""Writes the fixture beside it: a small pack that git itself wrote (git pack-objects, default options, so with REF_DELTA
entries), its idx, and objects.json: name -> type, size, depth (git verify-pack -v) and the SHA-1 of the content
(git cat-file).  Needs git; the tests that read the fixture do not.

    python tests/golden/git_pack/gen_git_pack.py
"""
import hashlib
import json
import os
import random
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ENV = dict(os.environ, GIT_AUTHOR_NAME="a", GIT_AUTHOR_EMAIL="a@example.org", GIT_COMMITTER_NAME="a", GIT_COMMITTER_EMAIL="a@example.org",
           GIT_AUTHOR_DATE="1700000000 +0000", GIT_COMMITTER_DATE="1700000000 +0000", GIT_CONFIG_GLOBAL="/dev/null", GIT_CONFIG_SYSTEM="/dev/null")


def git(repo, *args, **kw):
    return subprocess.run(["git", "-C", repo] + list(args), check=True, capture_output=True, env=ENV, **kw).stdout


def versions(seed, count, lines):
    """a file of `lines` lines and count - 1 later versions, each a small edit of the one before"""
    rng = random.Random(seed)
    cur = ["line %d of file %d: %s" % (k, seed, "".join(rng.choice("abcdefgh ") for _ in range(rng.randrange(10, 50)))) for k in range(lines)]
    out = []
    for v in range(count):
        out.append("\n".join(cur).encode() + b"\n")
        for _ in range(3):
            k = rng.randrange(len(cur))
            cur[k] = "edit %d.%d %s" % (v, k, "".join(rng.choice("xyz") for _ in range(20)))
        cur.insert(rng.randrange(len(cur)), "new line in version %d" % v)
    return out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        repo = os.path.join(tmp, "r")
        os.mkdir(repo)
        git(repo, "init", "-q", "-b", "main")
        files = {"f%d.txt" % s: versions(s, 6, 60) for s in range(3)}
        for v in range(6):
            for name, vs in files.items():
                with open(os.path.join(repo, name), "wb") as f:
                    f.write(vs[v])
            git(repo, "add", "-A")
            git(repo, "commit", "-q", "-m", "version %d" % v)
        git(repo, "tag", "-a", "-m", "a tag", "v1")
        revs = git(repo, "rev-list", "--objects", "--all").decode().split("\n")
        names = "\n".join([r.split(" ")[0] for r in revs if r] + [git(repo, "rev-parse", "v1").decode().strip()]) + "\n"
        base = os.path.join(tmp, "out")
        sha = git(repo, "pack-objects", "--depth=10", "--window=10", base, input=names.encode()).decode().strip()
        pack, idx = "%s-%s.pack" % (base, sha), "%s-%s.idx" % (base, sha)
        table = {}
        for line in git(repo, "verify-pack", "-v", idx).decode().split("\n"):
            w = line.split()
            if len(w) >= 5 and len(w[0]) == 40 and w[1] in ("commit", "tree", "blob", "tag"):
                data = git(repo, "cat-file", w[1], w[0])
                table[w[0]] = {"type": w[1], "size": len(data), "depth": int(w[5]) if len(w) >= 7 else 0, "sha1": hashlib.sha1(data).hexdigest()}
        for src, dst in ((pack, "git.pack"), (idx, "git.idx")):
            with open(src, "rb") as f, open(os.path.join(HERE, dst), "wb") as g:
                g.write(f.read())
        with open(os.path.join(HERE, "objects.json"), "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
        print(len(table), "objects,", sum(1 for o in table.values() if o["depth"]), "deltas, depth up to", max(o["depth"] for o in table.values()),
              os.path.getsize(pack) + os.path.getsize(idx), "bytes")


if __name__ == "__main__":
    main()
