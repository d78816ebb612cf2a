"""Rate of the charge response per point (qd_eval_points_response, eval_points(kT=..., response=True)) beside the thermal state
alone (eval_points(kT=...)) on the same handle and the same points.

    python scripts/response_rate.py [--dots 4,8] [--states 32] [--resolution 64] [--envs 64] [--repeats 5] [--calls 3]
                                    [--out profiles/response_rate.txt]

The handle and the points of scripts/thermal_rate.py: per configuration (N dots, K = num_charge_states), on one handle of `--envs`
envs, each configuration in a child process of its own: one group per env of C * P random points within the scan window of its
ground truth (every slot full), open regime, kT = 8.617333262145e-5 * 100.
  thermal    eval_points(kT=kT, outputs=("signal", "occupations", "variance", "ztail")): search + thermal kernel + write
  response   the same with response=True: search + thermal kernel with the response epilogue + write + dS/dv
Wall time around `--calls` calls ending in a device synchronise; the routes alternate inside every repeat; the first window of
each route allocates its scratch and is not counted.  Each route is reported by its best window in points/s, with the spread of
its windows, (worst - best) / best, which is the run-to-run spread a comparison with another commit has to exceed; and response
over thermal.  The thermal route launches what it launched before the response existed, so its figure is the one to hold against
the same script's run on the parent commit.
One JSON line per configuration on stdout; --out appends them to a file as well."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-agent-for-qubit-array-tuning_amd"))

KT = 8.617333262145e-5 * 100
ALL = ("signal", "occupations", "variance", "ztail")


def run(N, K, args):
    import torch
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    if not torch.cuda.is_available():
        raise SystemExit("response_rate.py measures on the GPU and found none")
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
    routes = (("thermal", dict(kT=KT, outputs=ALL)), ("response", dict(kT=KT, outputs=ALL, response=True)))
    if not args.with_response:                                   # (a commit without the argument: the thermal route alone)
        routes = routes[:1]
    best = {name: np.inf for name, _ in routes}
    worst = {name: 0.0 for name, _ in routes}
    for rep in range(args.repeats + 1):
        for name, kw in routes:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(args.calls):
                env.eval_points(ids, vg_d, vb_d, **kw)
            torch.cuda.synchronize(); t = (time.perf_counter() - t0) / args.calls
            if rep > 0:
                best[name] = min(best[name], t)
                worst[name] = max(worst[name], t)
    out = {"n_dots": N, "num_charge_states": K, "resolution": R, "envs": B, "points": B * CP, "kT": KT, "calls_per_window": args.calls}
    for name, _ in routes:
        out[name + "_s"] = round(best[name], 5)
        out[name + "_points_per_s"] = round(B * CP / best[name])
        out[name + "_spread"] = round((worst[name] - best[name]) / best[name], 4)
    if args.with_response:
        out["response_over_thermal"] = round(best["response"] / best["thermal"], 3)
        r = env.eval_points(ids[:1], vg_d[:1], vb_d[:1], kT=KT, outputs=("occupations",), response=True)
        out["max_abs_chi_kT"] = round(float(r["chi"].abs().max()) * KT, 4)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dots", default="4,8")
    ap.add_argument("--states", default="32")
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--thermal-only", dest="with_response", action="store_false",
                    help="measure the thermal route alone (for a commit whose eval_points has no response argument)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        N, K = (int(v) for v in args.child.split(","))
        print(json.dumps(run(N, K, args)), flush=True)
        return
    common = ["--resolution", str(args.resolution), "--envs", str(args.envs), "--repeats", str(args.repeats), "--calls", str(args.calls)]
    if not args.with_response:
        common.append("--thermal-only")
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
