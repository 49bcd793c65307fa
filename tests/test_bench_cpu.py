"""bench.py's multi-GPU launch contract on the CPU (no GPU call): ``--gpus N`` without a
launcher starts N ranks through torch.distributed.run as a child process; under a
launcher ``--gpus`` must equal WORLD_SIZE."""
import os
import subprocess
import sys

import pytest

from conftest import REPO


def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gpus_spawns_ranks(monkeypatch):
    bench = _bench()
    seen = {}
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    monkeypatch.setattr(subprocess, "call", lambda cmd: seen.setdefault("cmd", cmd) and 0)
    args = bench.parse()
    assert bench.launch_ranks(args) == 0
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert cmd[-4:] == ["--gpus", "4", "--steps", "3"]


def test_plain_run_is_the_headline_alone_and_full_restores_the_legs(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None and a.steps == 3 and a.warmup == 1
    assert a.no_cpu_baseline and a.no_kernel_timer and a.no_dice
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "somewhere"
    assert not (a.no_cpu_baseline or a.no_kernel_timer or a.no_dice)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-dice"])
    a = bench.parse()
    assert a.no_dice and not a.no_cpu_baseline and not a.no_kernel_timer


def test_dump_sample_is_fixed_and_bounded():
    import torch
    bench = _bench()
    flat = torch.arange(1000, dtype=torch.float32)
    a, b = bench._seeded_sample(flat, 64, seed=12), bench._seeded_sample(flat, 64, seed=12)
    assert a.numel() == 64 and torch.equal(a, b)
    assert torch.equal(a, a.sort().values) and a.unique().numel() == 64      # ascending positions, no repeats
    assert bench._seeded_sample(flat, 1000, seed=12) is flat
    # logits at the cap plus the parameter sample and the loss stay under 64 MB
    assert bench.DUMP_CAP_BYTES + 4 * bench.PARAM_SAMPLE + 4 < 64 * 10 ** 6


def test_gpus_one_and_launcher_consistency(monkeypatch):
    bench = _bench()
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    assert bench.launch_ranks(bench.parse()) is None           # N = 1: run in this process
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    assert bench.launch_ranks(bench.parse()) is None           # launched rank: run
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8"])
    with pytest.raises(SystemExit, match="WORLD_SIZE=2"):
        bench.launch_ranks(bench.parse())
