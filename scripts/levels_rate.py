"""Rate of the energy levels per point (qd_eval_points_ex, eval_points(levels=L)) beside the signal of the same points on the
same handle.

    python scripts/levels_rate.py [--dots 4,8] [--states 32,8] [--resolution 32] [--envs 16] [--repeats 3]
                                  [--out profiles/levels_rate.txt]

The handle and the points of scripts/closed_rate.py: per configuration (N dots, K = num_charge_states), on one handle of
`--envs` envs, each configuration in a child process of its own: one group per env of C * P random points within the scan window
of its ground truth (every slot full).  Open and closed (n_charge = N).  Wall time, synchronised, best of `--repeats`; the first
run of each route allocates its scratch and is not counted.
  signal    eval_points(outputs=("signal",)): search + ground-state stage, the deterministic point path
  levels2   eval_points(outputs=(), levels=2): search + levels kernel, no ground-state stage
  levels8   the same at levels=8
  both2/8   eval_points(outputs=("signal",), levels=L): all three
These are the routes a caller can take, each reported against `signal` of the same run; the search is in all of them.  The last
field is the share of env 0's points whose relative gap (levels[1] - levels[0]) / hnorm is at or below 1e-9.
One JSON line per configuration and regime on stdout; --out appends them to a file as well."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-agent-for-qubit-array-tuning_amd"))


def run(N, K, args):
    import torch
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    R, B = args.resolution, args.envs
    env = VecQuantumDeviceEnv(B, num_dots=N, resolution=R, seed=1234, num_charge_states=K, capacitance_model=lambda img: (None, None))
    env.load_new_devices(seed=1234)
    L, C, G = env.L, N - 1, N + 1
    CP = C * R * R
    st, _ = env.get_state()
    par = env._params_host
    rng = np.random.default_rng(5)
    vgm = st[:, L.s_vgm:L.s_vgm + G * G].reshape(B, G, G)
    win = par[:, L.scal + 2]

    def physical(e, virt):                                       # virtual plungers (n, N), sensor at its ground truth
        full = np.concatenate([virt, np.full((virt.shape[0], 1), st[e, L.s_sensor_gt])], axis=1)
        return full @ vgm[e].T + par[e, L.origin:L.origin + G]

    vg = np.stack([physical(e, st[e, L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-win[e], win[e], (CP, N))) for e in range(B)])
    vb = st[:, None, L.s_barrier_gt:L.s_barrier_gt + C] + rng.uniform(-1, 1, (B, CP, C))
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(env.device)      # noqa: E731
    vg_d, vb_d, ids = dev(vg), dev(vb), np.arange(B)

    def best(fn):
        times = []
        for _ in range(args.repeats + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
        return min(times[1:])

    lines = []
    for regime, kw in (("open", {}), ("closed", {"n_charge": N})):
        out = {"n_dots": N, "num_charge_states": K, "resolution": R, "envs": B, "points": B * CP, "regime": regime}
        routes = (("signal", dict(outputs=("signal",))), ("levels2", dict(outputs=(), levels=2)), ("levels8", dict(outputs=(), levels=8)),
                  ("both2", dict(outputs=("signal",), levels=2)), ("both8", dict(outputs=("signal",), levels=8)))
        for name, r in routes:
            t = best(lambda: env.eval_points(ids, vg_d, vb_d, **r, **kw))
            out[name + "_s"] = round(t, 4)
            out[name + "_points_per_s"] = round(B * CP / t)
        for name, _ in routes[1:]:
            out[name + "_over_signal"] = round(out[name + "_s"] / out["signal_s"], 3)
        lv = env.eval_points(ids[:1], vg_d[:1], vb_d[:1], outputs=(), levels=2, **kw)
        gap = ((lv["levels"][0, :, 1] - lv["levels"][0, :, 0]) / lv["hnorm"][0]).cpu().numpy()
        out["rel_gap_below_1e-9"] = round(float((gap <= 1e-9).mean()), 4)
        lines.append(out)
    env.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dots", default="4,8")
    ap.add_argument("--states", default="32,8")
    ap.add_argument("--resolution", type=int, default=32)
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        N, K = (int(v) for v in args.child.split(","))
        for line in run(N, K, args):
            print(json.dumps(line), flush=True)
        return
    common = ["--resolution", str(args.resolution), "--envs", str(args.envs), "--repeats", str(args.repeats)]
    lines = []
    for N in args.dots.split(","):
        for K in args.states.split(","):
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{N},{K}"] + common, check=True,
                                 stdout=subprocess.PIPE, text=True).stdout
            sys.stdout.write(res); sys.stdout.flush()
            lines.append(res)
    if args.out:
        with open(args.out, "a") as f:
            f.writelines(lines)


if __name__ == "__main__":
    main()
