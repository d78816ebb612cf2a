"""Time of a full device-range map by probe scans against the route without them.

    python scripts/probe_rate.py [--dots 4,8] [--resolution 64] [--envs 64] [--repeats 3] [--only probe|old|select]

Workload per shape: the full-range map (qadapt_hip.device_map.map_full_device_range) of ONE device of an `--envs` handle:
nx * ny tiles from the device's sampled plunger range and its own window.  Each shape in a child process of its own.
  probe   one probe of all tiles + one compose on the GPU (the composite stays on the device), wall time, synchronised
  old     the same tiles through the route a handle without probes has: the device loaded into every env slot (untimed),
          then per batch of `--envs` tiles get_state / set_state / observe / raw(), stitched and normalised with NumPy
  select  the composite's exact percentile select at n = nx*ny*P alone (HIP events): spread over the grid against one
          block of the per-env percentile kernel
One JSON line per shape on stdout.  `--only probe` runs that route alone (for a kernel trace of its own)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-agent-for-qubit-array-tuning_amd"))


def run(N, args):
    import numpy as np
    import torch
    from qadapt_hip import _lib
    from qadapt_hip import device_map as M
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    R, B = args.resolution, args.envs
    env = VecQuantumDeviceEnv(B, num_dots=N, resolution=R, seed=1234, capacitance_model=lambda img: (None, None))
    env.load_new_devices(seed=1234)
    env.observe()
    L = env.L
    out = {"n_dots": N, "resolution": R, "envs": B, "chunk_envs": env.chunk_envs()}

    def sync():
        torch.cuda.synchronize()

    m = None
    if args.only in (None, "probe"):
        times = []
        for _ in range(args.repeats + 1):                       # the first run allocates the probe scratch: not counted
            sync(); t0 = time.perf_counter()
            m = M.map_full_device_range(env, 0, 0)
            sync(); times.append(time.perf_counter() - t0)
        out["probe_route_s"] = [round(t, 4) for t in times[1:]]
    else:
        m = M.map_full_device_range(env, 0, 0)
    nx, ny = m["n_scans_x"], m["n_scans_y"]
    nq = nx * ny
    out.update(n_scans_x=nx, n_scans_y=ny, tiles=nq)
    comp_probe = m["composite"].cpu().numpy()

    if args.only in (None, "select"):
        n = nq * R * R
        z = m["scans"].contiguous().reshape(-1)
        res = torch.empty(2, dtype=torch.float64, device=z.device)
        ms = ctypes.c_float(0)
        for key, single in (("select_grid_ms", 0), ("select_one_block_ms", 1)):
            for it in (1, args.repeats):                          # one warm-up call, then the timed ones
                _lib.check(env._h, env._lib.qd_time_select(env._h, z.data_ptr(), n, single, it, res.data_ptr(),
                                                           ctypes.byref(ms), env._stream()), "qd_time_select")
            out[key] = round(float(ms.value), 4)
            out[key.replace("_ms", "_plohi")] = res.cpu().tolist()
        out["select_values"] = n

    if args.only in (None, "old"):
        # every slot gets device 0 (untimed), then tiles go through the slots B at a time
        ids = np.arange(B, dtype=np.int32)
        st, steps = env.get_state()
        par = np.ascontiguousarray(np.tile(env._params_host[0], (B, 1)))
        st = np.ascontiguousarray(np.tile(st[0], (B, 1)))
        _lib.check(env._h, env._lib.qd_load_episodes(env._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), B,
                                                     par.ctypes.data, st.ctypes.data, 0, env._stream()), "qd_load_episodes")
        env.set_state(st, steps)
        gates = np.tile(m["gt_gates"], (nq, 1)); gates[:, 0] = m["centres"][:, 0]; gates[:, 1] = m["centres"][:, 1]
        times = []
        for _ in range(args.repeats):
            sync(); t0 = time.perf_counter()
            scans = np.empty((nq, R, R))
            for b0 in range(0, nq, B):
                n = min(B, nq - b0)
                s_, k_ = env.get_state()
                s_[:n, L.s_gate_v:L.s_gate_v + N] = gates[b0:b0 + n]
                s_[:n, L.s_barrier_v:L.s_barrier_v + N - 1] = m["gt_barriers"]
                s_[:n, L.s_sensor_gt] = 0.0
                env.set_state(s_, k_)
                env.observe()
                raw, _ = env.raw()
                scans[b0:b0 + n] = raw[:n, 0].reshape(n, R, R)
            comp = np.zeros((ny * R, nx * R))
            for idx in range(nq):
                i, j = idx // ny, idx % ny
                comp[j * R:(j + 1) * R, i * R:(i + 1) * R] = scans[idx]
            lo, hi = np.percentile(comp, 0.5), np.percentile(comp, 99.5)
            comp = np.clip((comp - lo) / (hi - lo), 0, 1) if hi > lo else np.zeros_like(comp)
            times.append(time.perf_counter() - t0)
        out["old_route_s"] = [round(t, 4) for t in times]
        out["routes_agree"] = bool(np.array_equal(comp.astype(np.float32), comp_probe))
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dots", default="4,8")
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, choices=("probe", "old", "select"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        print(json.dumps(run(int(args.child), args)), flush=True)
        return
    common = ["--resolution", str(args.resolution), "--envs", str(args.envs), "--repeats", str(args.repeats)]
    if args.only:
        common += ["--only", args.only]
    for N in args.dots.split(","):
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", N] + common)


if __name__ == "__main__":
    main()
