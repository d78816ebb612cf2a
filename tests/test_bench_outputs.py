"""bench.py's result line and --dump-outputs: a plain run reports the headline figures only, --full adds the kernel / CPU
legs, and two runs with the same arguments write the same outputs (so two builds can be compared output for output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}
FULL_KEYS = {"roofline", "valu", "cpu_baseline", "parity"}
OUTPUTS = {"image", "plunger_images", "barrier_images", "obs_gate_voltages", "obs_barrier_voltages", "rewards",
           "terminated", "truncated"}


def test_full_and_dump_are_off_by_default():
    a = bench.build_parser().parse_args(["--gpus", "1", "--steps", "5", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 5


def test_zero_steps_is_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_dump_sample_is_fixed_sorted_and_within_budget():
    per_env = 491708                                           # 8-dot 64x64: all three images + the per-env vectors
    s = bench.dump_sample(4096, per_env, bench.DUMP_BYTES)
    assert len(s) * per_env <= bench.DUMP_BYTES < (len(s) + 1) * per_env
    assert np.all(np.diff(s) > 0) and s[0] >= 0 and s[-1] < 4096
    assert np.array_equal(s, bench.dump_sample(4096, per_env, bench.DUMP_BYTES))
    assert np.array_equal(bench.dump_sample(7, per_env, bench.DUMP_BYTES), np.arange(7))       # small batch: whole
    assert len(bench.dump_sample(4096, 10 ** 9, bench.DUMP_BYTES)) == 1                         # at least one env


def _fake_step(B, N, R, seed):
    """host tensors shaped like what VecQuantumDeviceEnv.step returns"""
    import torch
    g = torch.Generator().manual_seed(seed)
    v = torch.rand((B, 2 * N - 1), generator=g)
    obs = {"image": torch.rand((B, R, R, N - 1), generator=g), "obs_gate_voltages": v[:, :N],
           "obs_barrier_voltages": v[:, N:], "plunger_images": torch.rand((B, N, R, R, 2), generator=g),
           "barrier_images": torch.rand((B, N - 1, R, R, 1), generator=g)}
    return obs, torch.rand((B, 2 * N - 1), generator=g, dtype=torch.float64), torch.zeros(B, dtype=torch.bool), \
        torch.arange(B) % 2 == 0


def test_dump_outputs_writes_float_arrays_of_the_same_envs(tmp_path):
    obs, rew, term, trunc = _fake_step(300, 8, 64, 0)
    bench.dump_outputs(str(tmp_path / "one"), {8: (obs, rew, term, trunc)})
    files = {f[:-4]: np.load(tmp_path / "one" / f) for f in os.listdir(tmp_path / "one")}
    assert set(files) == OUTPUTS and sum(a.nbytes for a in files.values()) <= bench.DUMP_BYTES
    assert files["rewards"].dtype == np.float64 and all(files[k].dtype == np.float32 for k in OUTPUTS - {"rewards"})
    per_env = sum(a[0].nbytes for a in files.values())
    ids = bench.dump_sample(300, per_env, bench.DUMP_BYTES)
    assert len(ids) < 300
    assert np.array_equal(files["image"], obs["image"].numpy()[ids])
    assert np.array_equal(files["obs_barrier_voltages"], obs["obs_barrier_voltages"].numpy()[ids])
    assert np.array_equal(files["rewards"], rew.numpy()[ids])
    assert np.array_equal(files["truncated"], trunc.numpy()[ids].astype(np.float32))
    # a mixed batch: one set per dot count, the budget shared
    bench.dump_outputs(str(tmp_path / "mixed"), {n: _fake_step(100, n, 64, n) for n in (2, 4, 6, 8)})
    files = {f[:-4]: np.load(tmp_path / "mixed" / f) for f in os.listdir(tmp_path / "mixed")}
    assert set(files) == {f"{n}dot_{k}" for n in (2, 4, 6, 8) for k in OUTPUTS}
    assert sum(a.nbytes for a in files.values()) <= bench.DUMP_BYTES
    assert files["2dot_image"].shape == (100, 64, 64, 1) and files["8dot_plunger_images"].shape[1:] == (8, 64, 64, 2)


def _bench(*flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_line_and_repeatable_outputs(tmp_path):
    # 128 8-dot 64x64 envs are more than the dump budget holds: the seeded sample is exercised
    flags = ["--gpus", "1", "--dots", "8", "--envs", "128", "--resolution", "64", "--steps", "3", "--warmup", "1"]
    outs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        line = _bench(*flags, "--dump-outputs", str(d))
        assert LINE_KEYS <= set(line) and not FULL_KEYS & set(line)
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(128 * 1e3 / line["ms_per_step"], rel=1e-9)
        files = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
        assert set(files) == OUTPUTS
        assert all(a.dtype in (np.float32, np.float64) for a in files.values())
        assert sum(a.nbytes for a in files.values()) <= 64 * 10 ** 6
        n = {a.shape[0] for a in files.values()}
        assert len(n) == 1 and 1 <= n.pop() < 128
        assert files["image"].shape[1:] == (64, 64, 7) and files["rewards"].shape[1:] == (15,)
        assert np.isfinite(files["image"]).all() and np.isfinite(files["rewards"]).all()
        outs.append(files)
    for name in OUTPUTS:
        assert np.array_equal(outs[0][name], outs[1][name]), name


@pytest.mark.gpu
def test_full_adds_kernel_figures_and_cpu_baseline():
    line = _bench("--gpus", "1", "--config", "config1", "--steps", "2", "--warmup", "1", "--full", "--cpu-seconds", "1")
    assert LINE_KEYS <= set(line) and FULL_KEYS <= set(line) and line["steps"] == 2
    assert line["roofline"]["kernel_ms"] > 0 and line["cpu_baseline"]["value"] > 0
    assert line["parity"]["charge_state_list_mismatches"] == 0
