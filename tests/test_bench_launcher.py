"""`python bench.py --gpus N` must bring up its N ranks itself: the launcher, without a GPU (--dry-launch).
`--steps K` times exactly K steps, and `--dump-outputs DIR` writes what the last of them computed, the same on every run."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(args, env=None):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout     # ONE json line, from rank 0
    return json.loads(lines[0])


def test_plain_command_launches_two_ranks():
    d = run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--dry-launch"])
    assert d["dry_launch"] and d["n_gpus"] == 2
    assert d["ranks"] == [0, 1] and d["local_ranks"] == [0, 1] and d["pids"] == 2


def test_under_a_launcher_it_is_one_rank():
    # the driver's form: python -m torch.distributed.run ... bench.py --gpus N: no second level of launching
    import socket
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "3", "--dry-launch"],
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 3 and d["local_ranks"] == [0, 1, 2] and d["pids"] == 3


def test_single_rank_dry_launch():
    d = run(["--dry-launch"])
    assert d["n_gpus"] == 1 and d["ranks"] == [0]


import pytest


@pytest.mark.gpu
def test_two_ranks_on_one_device_rows_form_checks_itself():
    # VERDICT r3 "Next #3": the self-check runs the form the timed run uses (2 x 8192 chains: the rows form through the windows,
    # ns = 10000, 72 iterations), the timed run is wrapped (a p2p failure repeats it on the collective form), the shards' exchange
    # marks are compared across ranks after the run, and the line says how many ranks the process group really had
    d = run(["--gpus", "2", "--same-device", "--workload", "c3", "--chains", "8192", "--steps", "1", "--warmup", "1", "--no-cpu-baseline"])
    cfg = d["config"]
    assert d["n_gpus"] == 2 and cfg["world_seen"] == 2 and cfg["backend"]
    assert cfg["protocol"] == "p2p" and "8192 chains per rank" in cfg["protocol_check"] and "72 iterations" in cfg["protocol_check"]
    assert "0 inconsistent partner marks across 2 rank(s)" in cfg["cross_rank_check"]
    assert cfg["chains_total"] == 16384 and d["value"] > 0


@pytest.mark.gpu
def test_single_gpu_line_carries_the_persistent_kernel():
    d = run(["--steps", "1", "--warmup", "1", "--no-cpu-baseline"])
    r = d["roofline"]
    assert r["kernel"].startswith("k_chain_persist_loc") and r["persistent"]["launches"] >= 2 and r["persistent"]["repairs"] == 0
    assert r["one_launch_per_iteration"]["avg_kernel_us"] > r["avg_kernel_us"] > 0
    assert "0 inconsistent partner marks" in d["config"]["cross_rank_check"]


@pytest.mark.gpu
def test_two_ranks_on_one_device_take_the_persistent_form():
    # VERDICT r4 "Next #1" (iii): bench.py --gpus N: the self-check passes on the form the timed run uses, the timed run takes the
    # persistent form (2 x 2048 chains: all 256 tiles resident on the one GPU) and the line says which form ran
    d = run(["--gpus", "2", "--same-device", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"])
    cfg = d["config"]
    assert d["n_gpus"] == 2 and cfg["world_seen"] == 2 and cfg["protocol"] == "p2p"
    assert cfg["shard_form"].startswith("persistent"), cfg["shard_form"]
    assert d["roofline"]["kernel"] == "k_chain_persist_loc<2, false, true, false>" and d["roofline"]["persistent"]["repairs"] == 0
    assert "0 inconsistent partner marks across 2 rank(s)" in cfg["cross_rank_check"]


class _FakeContext:
    """history / state of N chains after `it` iterations, as a context hands them out (no device)"""

    def __init__(self, N, np_, nm, it):
        from smm_jl_amd import _abi as A
        self.A, self.N, self.np, self.nm, self.it, self.asked = A, N, np_, nm, it, None

    def _fill(self, b, seed):
        import numpy as np
        rng = np.random.default_rng(seed)
        for f in b.FIELDS:
            a = getattr(b, f)
            a[...] = rng.integers(0, 100, a.shape) if a.dtype.kind in "iu" else rng.standard_normal(a.shape)
        return b

    def state(self):
        s = self._fill(self.A.StateBuffers(self.N, self.np, self.nm), 1)
        s.iter = self.it
        return s

    def history(self, t0, t1):
        self.asked = (t0, t1)
        return self._fill(self.A.HistoryBuffers(t1 - t0, self.N, self.np, self.nm), 2)


def test_dump_outputs_writes_the_last_step_whole_or_a_seeded_sample_within_64_mb(tmp_path):
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from smm_jl_amd import _abi as A
    names = {"chains"} | {"history_" + f for f in A.HistoryBuffers.FIELDS} | {"state_" + f for f in A.StateBuffers.FIELDS}
    small = _FakeContext(64, 2, 2, 600)
    bench.dump_outputs(small, str(tmp_path / "small"))
    assert small.asked == (400, 600)     # the last step's 200 iterations
    got = {p.stem: np.load(p) for p in (tmp_path / "small").iterdir()}
    assert set(got) == names and all(a.dtype == np.float64 for a in got.values())
    h, s = small.history(400, 600), small.state()
    assert np.array_equal(got["chains"], np.arange(64))
    for f in A.HistoryBuffers.FIELDS:
        assert np.array_equal(got["history_" + f], getattr(h, f)), f
    for f in A.StateBuffers.FIELDS:
        assert np.array_equal(got["state_" + f], getattr(s, f)), f
    big = _FakeContext(4096, 50, 50, 400)     # c5's shape: 173 KB of history per chain, 708 MB in all
    for d in ("big1", "big2"):
        bench.dump_outputs(big, str(tmp_path / d))
    assert sum(p.stat().st_size for p in (tmp_path / "big1").iterdir()) <= 64e6
    c = np.load(tmp_path / "big1" / "chains.npy").astype(np.int64)
    assert 0 < len(c) < 4096 and np.all(np.diff(c) > 0)
    h = big.history(200, 400)
    assert np.array_equal(np.load(tmp_path / "big1" / "history_params.npy"), h.params[..., c])
    for p in (tmp_path / "big1").iterdir():      # the same sample every time
        assert np.array_equal(np.load(p), np.load(tmp_path / "big2" / p.name)), p.name


@pytest.mark.gpu
def test_steps_are_the_timed_steps_and_the_dumped_outputs_repeat(tmp_path):
    import numpy as np
    lines = [run(["--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-unfused", "--dump-outputs", str(tmp_path / d)]) for d in ("a", "b")]
    for d in lines:
        assert d["steps"] == 2 and d["repetitions"]["n"] == 1 and d["ms_per_step"] > 0
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert "history_value.npy" in files and sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 64e6
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f), equal_nan=True), f
