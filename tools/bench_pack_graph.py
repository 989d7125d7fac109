"""The object graph of a pack on one GPU, host to host, for DESIGN 4n.  The pack is written by tests/pack_writer.py: a
linear history of `--commits` commits over a tree of 16 x 16 x 16 files, every commit editing one file - so a blob, three
trees and a commit each -, all objects whole.

  open          md_pack_open: the table the graph is built over
  graph         md_pack_graph_build: the commits, trees and tags decoded and their links read (blobs are not inflated)
  reach_all     md_pack_reachable from the newest commit
  reach_range   md_pack_reachable from the newest commit minus what the middle commit reaches (two walks)
  git rev-list  `git rev-list --objects <newest>` and `<newest> ^<middle>` over the same pack, one CPU process, if git is on the machine
and md_pack_graph_get's and md_pack_reach_last's counts with the device time of the link passes and of the steps.

    python tools/bench_pack_graph.py [--commits 20000] [--reps 7] [--warmup 1]

The legs are alternated in one process; every leg reports the median and the spread (min .. max) of its repeats, host to
host (perf_counter around a call that ends in a synchronise).  The marks of reach_all are compared with the whole pack."""
import argparse
import json
import os
import random
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import pack_graph_cases as gc  # noqa: E402
from tests import pack_writer as pw  # noqa: E402


def stats(v):
    return {"median_ms": round(statistics.median(v) * 1e3, 3), "min_ms": round(min(v) * 1e3, 3), "max_ms": round(max(v) * 1e3, 3)}


def history(commits):
    rng = random.Random(3)
    p = gc.Pack()
    files = [[[p.blob(b"file %d %d %d\n" % (a, b, c)) for c in range(16)] for b in range(16)] for a in range(16)]
    names = [b"%02d" % k for k in range(16)]
    low = [[p.add(gc.TREE, gc.tree([(b"100644", names[c], files[a][b][c]) for c in range(16)]))[1] for b in range(16)] for a in range(16)]
    mid = [p.add(gc.TREE, gc.tree([(b"40000", names[b], low[a][b]) for b in range(16)]))[1] for a in range(16)]
    heads, parents = [], []
    for k in range(commits):
        if k:  # (the first commit holds the tree as it was made)
            a, b, c = rng.randrange(16), rng.randrange(16), rng.randrange(16)
            files[a][b][c] = p.blob(b"file %d %d %d at commit %d\n" % (a, b, c, k))
            low[a][b] = p.add(gc.TREE, gc.tree([(b"100644", names[x], files[a][b][x]) for x in range(16)]))[1]
            mid[a] = p.add(gc.TREE, gc.tree([(b"40000", names[x], low[a][x]) for x in range(16)]))[1]
        top = p.add(gc.TREE, gc.tree([(b"40000", names[x], mid[x]) for x in range(16)]))[1]
        _, name = p.add(gc.COMMIT, gc.commit(top, parents, b"commit %d\n" % k))
        parents = [name]
        heads.append(name)
    return p.entries, heads


def time_git(pack, idx, revs, reps):
    git = shutil.which("git")
    if not git:
        return None
    with tempfile.TemporaryDirectory() as tmp:
        repo = os.path.join(tmp, "r.git")
        env = dict(os.environ, GIT_CONFIG_GLOBAL="/dev/null", GIT_CONFIG_SYSTEM="/dev/null")
        subprocess.run([git, "init", "-q", "--bare", repo], check=True, env=env)
        stem = os.path.join(repo, "objects", "pack", "pack-" + pack[-20:].hex())
        for ext, data in ((".pack", pack), (".idx", idx)):
            with open(stem + ext, "wb") as f:
                f.write(data)
        out, lines = [], 0
        for _ in range(reps):
            t0 = time.perf_counter()
            r = subprocess.run([git, "rev-list", "--objects"] + revs, cwd=repo, env=env, capture_output=True, check=True)
            out.append(time.perf_counter() - t0)
            lines = r.stdout.count(b"\n")
        return dict(stats(out), objects=lines)


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
    legs = {k: [] for k in ("open", "graph", "reach_all", "reach_range")}
    for rep in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        p = mp.Pack(pack, idx)
        t1 = time.perf_counter()
        g = p.graph()
        t2 = time.perf_counter()
        top, middle = p.find(heads[-1]), p.find(heads[len(heads) // 2])
        t3 = time.perf_counter()
        got = g.reachable([top])
        t4 = time.perf_counter()
        all_last = g.reach_last()
        t5 = time.perf_counter()
        cut = g.reachable([top], [middle])
        t6 = time.perf_counter()
        assert len(got) == len(entries) == g.info["n"] and g.connected() and 0 < len(cut) < len(got)
        if rep >= a.warmup:
            for k, v in zip(legs, (t1 - t0, t2 - t1, t4 - t3, t6 - t5)):
                legs[k].append(v)
        res["graph_info"], res["reach_all_last"], res["reach_range_last"], res["range_objects"] = g.info, all_last, g.reach_last(), len(cut)
        g.close(), p.close()
    res.update({k: stats(v) for k, v in legs.items()})
    res["git_rev_list_all"] = time_git(pack, idx, [heads[-1].hex()], a.reps)
    res["git_rev_list_range"] = time_git(pack, idx, [heads[-1].hex(), "^" + heads[len(heads) // 2].hex()], a.reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
