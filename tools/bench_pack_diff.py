"""Trees diffed on one GPU, host to host, for DESIGN 4o.  The pack is tools/bench_pack_graph.py's: a linear history of
`--commits` commits over a tree of 16 x 16 x 16 files, every commit editing one file, all objects whole.

  changes        Pack.changes(): every commit against its first parent's tree (md_pack_diff over all pairs, records joined to paths)
  md_pack_diff   the same pairs through md_pack_diff and its getters alone: the records as one array, no paths joined
  one_pair       Pack.diff of the newest commit's tree against its parent's
  git diff-tree  `git diff-tree -r --stdin` fed the same commits, and `git log --raw --no-renames -m --first-parent` from the
                 newest commit, over the same pack, one CPU process each, if git is on the machine
and md_pack_diff_get's counts with the device time of the table and diff kernels (events).

    python tools/bench_pack_diff.py [--commits 20000] [--reps 7] [--warmup 1]

The legs are alternated in one process; every leg reports the median and the spread (min .. max) of its repeats, host to
host.  The pack is opened and its graph built once, outside the legs (DESIGN 4n measures those).  The changed paths of
`changes` are compared with git's lines."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import pack_writer as pw  # noqa: E402
from tools.bench_pack_graph import history  # noqa: E402


def stats(v):
    return {"median_ms": round(statistics.median(v) * 1e3, 3), "min_ms": round(min(v) * 1e3, 3), "max_ms": round(max(v) * 1e3, 3)}


class Git:
    def __init__(self, pack, idx):
        self.git = shutil.which("git")
        self.tmp = tempfile.TemporaryDirectory()
        self.env = dict(os.environ, GIT_CONFIG_GLOBAL="/dev/null", GIT_CONFIG_SYSTEM="/dev/null")
        if self.git:
            self.repo = os.path.join(self.tmp.name, "r.git")
            subprocess.run([self.git, "init", "-q", "--bare", self.repo], check=True, env=self.env)
            stem = os.path.join(self.repo, "objects", "pack", "pack-" + pack[-20:].hex())
            for ext, data in ((".pack", pack), (".idx", idx)):
                with open(stem + ext, "wb") as f:
                    f.write(data)

    def run(self, args, stdin=None):
        t0 = time.perf_counter()
        r = subprocess.run([self.git] + args, cwd=self.repo, env=self.env, capture_output=True, check=True, input=stdin)
        return time.perf_counter() - t0, r.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commits", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    from decompress_amd import pack as mp
    entries, heads = history(a.commits)
    pack, idx, _ = pw.write_pack(entries)
    res = {"commits": a.commits, "objects": len(entries), "pack_mib": round(len(pack) / 2**20, 2)}
    p = mp.Pack(pack, idx)
    g = p.graph()
    order = [p.find(h) for h in heads]
    newest = [k for k in g.edges_of(order[-1])]
    pair = [(g.edges_of(order[-2])[0][2], newest[0][2])]
    git = Git(pack, idx)
    feed = b"".join(h.hex().encode() + b"\n" for h in heads)
    trees = [g.edges_of(c)[0][2] for c in order]
    all_pairs = [(None, trees[0])] + list(zip(trees, trees[1:]))
    legs = {k: [] for k in ("changes", "md_pack_diff", "one_pair", "git_diff_tree_stdin", "git_log_raw")}
    got = lines = None
    for rep in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        _, got = p.changes(order, graph=g)
        t1 = time.perf_counter()
        res["changes_info"] = p.diff_last()
        t2 = time.perf_counter()
        one = p.diff(pair, graph=g)
        t3 = time.perf_counter()
        res["one_pair_info"] = p.diff_last()
        t4 = time.perf_counter()
        rc, recs, _, _, _ = p._diff_call(all_pairs, True, g)  # the C call and its getters alone: the records as one array, no paths
        t5 = time.perf_counter()
        assert rc == 0 and len(recs) == res["changes_info"]["changes"]
        took = [t1 - t0, t5 - t4, t3 - t2]
        if git.git:
            dt, lines = git.run(["diff-tree", "-r", "--root", "--no-renames", "--no-abbrev", "--stdin"], feed)
            took.append(dt)
            took.append(git.run(["log", "--raw", "--no-renames", "--no-abbrev", "-m", "--first-parent", "--format=%H", heads[-1].hex()])[0])
        if rep >= a.warmup:
            for k, v in zip(legs, took):
                legs[k].append(v)
        assert one[0][0] == "Ok" and len(one[0][1]) == 3
    # the same paths as git's lines, commit by commit
    if lines is not None:
        want, cur = {}, None
        for ln in lines.split(b"\n"):
            if ln.startswith(b":"):
                want[cur].append(ln.split(b"\t")[1])
            elif ln:
                cur = ln.decode()
                want[cur] = []
        for h, (tag, recs) in zip(heads, got):
            assert tag == "Ok" and sorted(r[5] for r in recs if not r[6] & mp.CHANGE_TREE) == sorted(want[h.hex()]), h.hex()
        res["git_lines"] = sum(len(v) for v in want.values())
    res["file_records"] = sum(1 for _, recs in got for r in recs if not r[6] & mp.CHANGE_TREE)
    res.update({k: stats(v) for k, v in legs.items() if v})
    g.close(), p.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
