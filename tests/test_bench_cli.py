"""bench.py's launcher logic on CPU: `--gpus N` without a launcher re-executes under torch.distributed.run with N ranks
(`--gpus N` used to be ignored), and asks for more GPUs than the box has fail loudly.  With a GPU
(`pytest -m gpu`): what a plain run's line holds next to a --full one."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_single_gpu_needs_no_launcher(monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    assert bench.respawn_command(bench.parse(["--gpus", "1"]), ["--gpus", "1"], 8) is None


def test_gpus_n_spawns_n_ranks(monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    argv = ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    cmd = bench.respawn_command(bench.parse(argv), argv, 8)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-len(argv):] == argv and cmd[-len(argv) - 1].endswith("bench.py")


def test_a_rank_does_not_respawn(monkeypatch):
    monkeypatch.setenv("RANK", "2")
    assert bench.respawn_command(bench.parse(["--gpus", "4"]), ["--gpus", "4"], 8) is None


def test_too_few_devices_fails_loudly(monkeypatch):
    monkeypatch.delenv("RANK", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.respawn_command(bench.parse(["--gpus", "8"]), ["--gpus", "8"], 1)
    assert "only 1 gfx950" in str(e.value)


def test_steps_must_be_at_least_one():
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])
    assert bench.parse(["--steps", "3"]).steps == 3 and bench.parse([]).dump_outputs is None
    assert bench.parse(["--dump-outputs", "d"]).dump_outputs == "d"


def test_extra_legs_are_opt_in():
    """a plain run measures the headline only; --full adds the other legs and checks, and the --no-* options still apply"""
    assert bench.parse([]).full is False and bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"]).full is False
    a = bench.parse(["--full", "--no-deflate"])
    assert a.full is True and a.no_deflate is True and a.no_secondary is False


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True])
def test_plain_and_full_lines(tmp_path, full):
    """a plain run prints the headline with no extra legs; --full adds them (here the host path and the libz byte check)"""
    import json
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--streams", "64",
           "--stream-kib", "64", "--dump-outputs", str(tmp_path)]
    if full:
        cmd += ["--full", "--no-cpu-baseline", "--no-deflate", "--no-secondary"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["unit"] == "MiB/s" and d["higher_is_better"] is True and d["dtype"] == "u8" and d["value"] > 0
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["parity_ok"] is True and d["full"] is full
    assert d["roofline"]["kernel_ms"] > 0 and os.path.exists(os.path.join(str(tmp_path), "out_len.npy"))
    for leg in ("cpu_baseline", "deflate", "gzip", "lzo", "def_ns", "long_stream"):
        assert leg not in d, leg
    assert ("host_path" in d) is full
    if full:
        assert d["host_path"]["parity_ok"] is True


@pytest.mark.parametrize("n,nbytes", [(64, 64 * 1024), (2, 4 << 20)])
def test_dump_outputs_writes_exact_bounded_float_arrays(tmp_path, n, nbytes):
    """--dump-outputs on CPU tensors: float32 / float64 files under 64 MB, the same files for the same results, the sampled
    bytes where the offsets say, -1 beyond a stream's out_len"""
    import numpy as np
    import torch
    out_off = np.arange(n, dtype=np.int64) * nbytes
    d_out = torch.from_numpy(np.random.default_rng(1).integers(0, 256, n * nbytes, dtype=np.uint8))
    out_len = torch.full((n,), nbytes, dtype=torch.int64)
    out_len[1] = nbytes // 3
    res = (out_len, torch.arange(n, dtype=torch.int64) + 7, torch.zeros(n, dtype=torch.int32),
           torch.tensor([-1, 5] + [123456] * (n - 2), dtype=torch.int32))
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    sizes = [bench.dump_outputs(d, res, d_out, out_off, nbytes) for d in dirs]
    assert sizes[0] == sizes[1] and sum(sizes[0].values()) <= 64 * 10**6
    load = lambda d, k: np.load(os.path.join(d, k + ".npy"))
    for k in sizes[0]:
        a, b = load(dirs[0], k), load(dirs[1], k)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), k
    assert load(dirs[0], "checksum")[0] == 0xffffffff and list(load(dirs[0], "out_len")[:2]) == [nbytes, nbytes // 3]
    streams, cols = load(dirs[0], "sample_streams").astype(np.int64), load(dirs[0], "sample_offsets").astype(np.int64)
    s, raw = load(dirs[0], "out_sample"), d_out.numpy()
    assert s.shape == (len(streams), len(cols)) and cols.max() < nbytes
    for r, i in enumerate(streams):
        want = raw[i * nbytes + cols].astype(np.float32)
        want[cols >= int(out_len[i])] = -1
        assert np.array_equal(s[r], want)
