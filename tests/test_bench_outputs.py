"""bench.py --dump-outputs: what the timed step computed, written as .npy files (CPU tier: the writer, the size cap, the argument
checks; GPU tier: two runs with the same arguments write the same arrays, and the dumped loss is the line's).  And --full: a plain
run times the same steps as a --full run and leaves out what --full adds after them."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_steps_and_dump_arguments(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--workload", "S-cora", "--steps", "7", "--dump-outputs", "d"])
    args = bench.parse_args()
    assert args.steps == 7 and args.warmup == bench.DEFAULT_STEPS["S-cora"][1] and args.dump_outputs == "d"
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    assert bench.parse_args().dump_outputs is None
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + bad)
        with pytest.raises(SystemExit):
            bench.parse_args()


def test_full_is_off_by_default(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    assert bench.parse_args().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse_args().full is True


def test_step_outputs_hold_loss_parameters_and_moments(bench):
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(5, 4), torch.nn.ELU(), torch.nn.Linear(4, 3))
    opt = torch.optim.Adam(model.parameters(), lr=0.01)
    loss = model(torch.randn(8, 5)).square().mean()
    loss.backward()
    opt.step()
    out = bench.step_outputs(model, opt, loss)
    names = [n for n, _ in model.named_parameters()]
    assert set(out) == {"loss"} | {f"{k}.{n}" for k in ("param", "adam_exp_avg", "adam_exp_avg_sq") for n in names}
    assert out["loss"].shape == (1,) and out["loss"][0] == np.float32(loss.item())
    for n, p in model.named_parameters():
        assert out["param." + n].dtype == np.float32 and np.array_equal(out["param." + n], p.detach().numpy())
        assert np.array_equal(out["adam_exp_avg." + n], opt.state[p]["exp_avg"].numpy())
        assert np.array_equal(out["adam_exp_avg_sq." + n], opt.state[p]["exp_avg_sq"].numpy())


def test_write_outputs_keeps_small_arrays_whole_and_samples_large_ones_the_same_way(bench, tmp_path):
    arrays = {"a": np.arange(1000, dtype=np.float32).reshape(10, 100), "b": np.linspace(0, 1, 3000), "loss": np.ones(1, np.float32)}
    bench.write_outputs(str(tmp_path / "whole"), arrays)
    for k, v in arrays.items():
        got = np.load(tmp_path / "whole" / f"{k}.npy")
        assert got.dtype == v.dtype and np.array_equal(got, v)
    limit = 8000   # of 28 004 bytes
    for d in ("s1", "s2"):
        bench.write_outputs(str(tmp_path / d), arrays, limit=limit)
    total = 0
    for k, v in arrays.items():
        s1, s2 = np.load(tmp_path / "s1" / f"{k}.npy"), np.load(tmp_path / "s2" / f"{k}.npy")
        assert np.array_equal(s1, s2) and s1.dtype == v.dtype
        flat = v.reshape(-1)
        assert len(s1) == int(v.size * limit / 28004)
        # entries of the array, ascending flat positions, no repeats
        pos = np.searchsorted(flat, s1)
        assert np.array_equal(flat[pos], s1) and np.all(np.diff(pos) > 0)
        total += s1.nbytes
    assert total <= limit


@pytest.mark.gpu
def test_bench_dumps_the_same_outputs_for_the_same_arguments(tmp_path):
    """Two runs of `bench.py --dump-outputs` with the same arguments: the same files, the same values (the inputs are seeded, the
    step's kernels sum in a fixed order), under 64 MB, the dumped loss = the line's, and --steps = the number of timed steps."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    common = ["--workload", "S-cora", "--steps", "3", "--warmup", "1", "--gpu-warm-seconds", "0", "--no-cpu-baseline", "--no-bf16x3",
              "--no-all-rows", "--no-pruned"]
    lines = {}
    for d in ("a", "b"):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + common + ["--dump-outputs", str(tmp_path / d)], env=env,
                             cwd=tmp_path, check=True, timeout=600, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
        lines[d] = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    line = lines["a"]
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    assert "loss.npy" in files and any(f.startswith("param.") for f in files) and any(f.startswith("adam_exp_avg.") for f in files)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a)), f
        assert np.array_equal(a, b), f
    assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == line["loss"]


@pytest.mark.gpu
def test_plain_run_times_the_same_steps_and_full_adds_the_secondary_figures(tmp_path):
    """A plain run and a --full run with the same arguments: the same timed steps (the same loss and dumped arrays), the headline
    fields in both; only the --full line carries the re-timed variants, the GEMM kernels' events, the copy ceiling and the CPU
    baseline."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    common = ["--workload", "S-cora", "--steps", "3", "--warmup", "1", "--gpu-warm-seconds", "0"]
    lines = {}
    for d, extra in (("plain", []), ("full", ["--full"])):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + common + extra + ["--dump-outputs", str(tmp_path / d)],
                             env=env, cwd=tmp_path, check=True, timeout=600, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
        lines[d] = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("{")][-1])
    plain, full = lines["plain"], lines["full"]
    for line in (plain, full):
        assert line["metric"].startswith("edges aggregated/sec") and line["unit"] == "edges/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f32" and line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
        assert len(line["roofline"]["launches"]) > 0
    assert plain["full"] is False and full["full"] is True
    assert plain["loss"] == full["loss"]
    files = sorted(os.listdir(tmp_path / "plain"))
    assert files == sorted(os.listdir(tmp_path / "full"))
    for f in files:
        assert np.array_equal(np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)), f
    assert "cpu_baseline" not in plain and plain["gemm_kernels"] == {} and plain["gemm_ms_per_step"] is None
    assert plain["roofline"]["copy_ceiling_GBps"] is None
    assert all(plain[k] is None for k in ("ms_per_step_bf16x3", "ms_per_step_dense_on_all_rows", "ms_per_step_pruned"))
    assert full["cpu_baseline"]["value"] > 0 and full["gemm_kernels"] and full["gemm_ms_per_step"] > 0
    assert full["roofline"]["copy_ceiling_GBps"] > 0
    assert all(full[k] > 0 for k in ("ms_per_step_bf16x3", "ms_per_step_dense_on_all_rows", "ms_per_step_pruned"))
