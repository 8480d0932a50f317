"""bench.py's N>1 entry: `python bench.py --gpus N` must start its own N ranks
(one process per GPU under torch.distributed.run) instead of demanding a
torchrun environment.  Host logic only — no GPU, no rendezvous."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _dry(*argv, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    e.update(env or {})
    r = subprocess.run([sys.executable, BENCH, *argv, "--dry-launch"], env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])["launch"]


def test_gpus_2_builds_the_torchrun_command():
    cmd = _dry("--gpus", "2", "--steps", "7", "--warmup", "3", "--master-port", "29712")
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd
    assert cmd[cmd.index("--nproc-per-node") + 1] == "2"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[cmd.index("--master-port") + 1] == "29712"
    at = cmd.index(BENCH)
    tail = cmd[at + 1:]
    assert tail[:6] == ["--gpus", "2", "--steps", "7", "--warmup", "3"]
    assert "--dry-launch" not in tail


def test_gpus_8_and_forced_world_1():
    cmd = _dry("--gpus", "8")
    assert cmd[cmd.index("--nproc-per-node") + 1] == "8"
    assert int(cmd[cmd.index("--master-port") + 1]) > 0          # a free port was picked
    cmd = _dry("--gpus", "1", env={"BENCH_FORCE_DIST": "1"})
    assert cmd[cmd.index("--nproc-per-node") + 1] == "1"


def test_world_size_mismatch_is_a_message_not_an_assert():
    env = dict(os.environ, WORLD_SIZE="4", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    assert "AssertionError" not in r.stderr
    assert "WORLD_SIZE=4" in r.stderr


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_default_line_options_and_the_t1_cpu_baseline_path(monkeypatch):
    """A plain command measures the headline alone (no per-kernel pass, strong scaling only, no dump); `--full` keeps the
    per-kernel pass, the weak sub-record, the CPU linearity check and the `other_configs` sub-records on; the full-batch
    CPU baseline of BASELINE configs[1] (oracle uniform replay + torch-CPU DQN step, bench.CpuPathT1) runs on a host
    without a GPU and reports every field the bench line quotes."""
    bench = _bench_module()
    monkeypatch.setattr(sys, "argv", [BENCH, "--gpus", "1", "--steps", "7", "--warmup", "3"])
    args = bench.parse()
    assert not args.full and args.profile_steps == 0 and args.scaling == "strong" and args.dump_outputs is None
    assert args.gpus == 1 and args.steps == 7 and args.warmup == 3
    monkeypatch.setattr(sys, "argv", [BENCH, "--full"])
    args = bench.parse()
    assert args.full and args.profile_steps == 3 and args.scaling == "both"
    assert args.cpu_linearity_check and not args.no_other_configs and args.gpus == 1 and args.other_steps == 200
    monkeypatch.setattr(sys, "argv", [BENCH, "--full", "--no-cpu-linearity-check", "--no-other-configs", "--profile-steps", "1",
                                      "--scaling", "weak", "--dump-outputs", "out"])
    args = bench.parse()
    assert not args.cpu_linearity_check and args.no_other_configs and args.profile_steps == 1 and args.scaling == "weak"
    assert args.dump_outputs == "out"
    cpu = bench.CpuPathT1("dqn_uniform", fill_steps=80)
    assert cpu.B == 256 and not cpu.per and not cpu.iqn
    parts = cpu.learner_step()
    assert len(parts) == 3 and all(p >= 0 for p in parts) and parts[1] > 0
    assert cpu.acting_rate(EA=8, reps=1) > 0
    assert bench.file_date(os.path.join(ROOT, "profiles", "gather_traffic.json")).startswith("2026-10-01")


def test_dump_outputs_files_dtypes_sampling_and_budget(tmp_path, monkeypatch):
    """--dump-outputs (bench.dump_outputs) on host tensors: one .npy per parameter / gradient / logged loss / the priority
    leaves, float32 or float64; an array above 2^20 elements becomes the same seeded sample of 2^20 in every run;
    more than the byte budget is an error, not a silent truncation."""
    import numpy as np
    import torch
    bench = _bench_module()

    class Hist:
        def tree_nodes(self):
            v = np.arange(16, dtype=np.float64)
            return v, np.zeros(16, np.uint8), np.zeros(16)

    class Trainer:
        policy = torch.nn.Module()

    g = torch.Generator().manual_seed(0)
    Trainer.policy.big = torch.nn.Parameter(torch.randn(1100, 1000, generator=g))
    Trainer.policy.small = torch.nn.Parameter(torch.randn(3, 4, generator=g))
    Trainer.policy.small.grad = torch.full((3, 4), 0.5)
    logged = {"qloss": torch.tensor(1.25)}
    first = bench.dump_outputs(str(tmp_path / "a"), Trainer, Hist(), True, logged)
    bench.dump_outputs(str(tmp_path / "b"), Trainer, Hist(), True, logged)
    assert sorted(first) == ["grad.small", "logged.qloss", "param.big", "param.small", "priorities"]
    big = np.load(tmp_path / "a" / "param.big.npy")
    assert big.dtype == np.float32 and big.shape == (bench.DUMP_MAX_ELEMENTS,)
    assert np.array_equal(big, np.load(tmp_path / "b" / "param.big.npy"))
    assert np.isin(big, Trainer.policy.big.detach().numpy().reshape(-1)).all()
    assert np.array_equal(np.load(tmp_path / "a" / "param.small.npy"), Trainer.policy.small.detach().numpy())
    assert np.array_equal(np.load(tmp_path / "a" / "grad.small.npy"), np.full((3, 4), 0.5, np.float32))
    assert np.load(tmp_path / "a" / "logged.qloss.npy").tolist() == [1.25]
    assert np.array_equal(np.load(tmp_path / "a" / "priorities.npy"), np.arange(8, 16, dtype=np.float64))
    assert sum(first.values()) <= bench.DUMP_MAX_BYTES
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1 << 20)
    with pytest.raises(RuntimeError, match="dump-outputs"):
        bench.dump_outputs(str(tmp_path / "c"), Trainer, Hist(), True, logged)
