"""Rate of charge-response grids (qd_scan_grid_response, scan_grid_response) beside the thermal grid they extend, the per-point
route that gave the same derivatives before, and the same kernel on the whole-block core and epilogue.

    python scripts/response_grid_rate.py [--dots 4,8] [--states 32] [--resolution 64] [--envs 64] [--repeats 5] [--calls 2]
                                         [--whole-lib FILE] [--parent-tree DIR] [--out profiles/response_grid_rate.txt]

Per configuration (N dots, K = num_charge_states) on the handle and grids of scripts/thermal_grid_rate.py: `--envs` envs at R x R,
one grid of R x R points per env in the physical frame, plungers 1 and 2 over the env's scan window around its working point, every
other control at the working point, kT = 8.617333262145e-5 * 100, open regime.  The routes:
  a  thermal   scan_grid_thermal(..., kT)
  b  default   scan_grid_response(..., kT) with the default outputs ("dsignal_axes", "docc_axes")
  c  all       scan_grid_response(..., kT, response=all five)
  d  points    eval_points(kT=kT, response=True) at the grid's voltages (built in NumPy, uploaded once, outside the windows), one
               group per grid
  e  whole     route b on a library built with -DQD_RSG_FORCE_WHOLE (--whole-lib, scripts/ab_build.sh): the open regime on
               QdResponseWs / qd_response_solve.  Measurement only
  p  parent    route a with the package and the library of the parent commit (--parent-tree, a checkout of it with its library
               built): the thermal grid before this kernel existed
Each route runs in a child process of its own; ONE SESSION: the children of a window run one after the other, the routes
alternated (a, b, c, d, e, p, a, b, ..), `--repeats` windows per route.  A child times `--calls` calls ending in a device
synchronise, after one uncounted call that allocates the scratch.  The figure of a route is the best of its windows; its spread
is (worst - best) / best of them, and the run-to-run spread the verdicts are judged against is the largest spread of the routes
compared.  One JSON line per configuration on stdout; --out appends them to a file as well."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KT = 8.617333262145e-5 * 100
ALL = ("chi", "jacobian", "dsignal", "docc_axes", "dsignal_axes")


def run(N, K, args):
    """one child: one window of one route; seconds per call"""
    sys.path.insert(0, os.path.join(args.tree or ROOT, "rl-agent-for-qubit-array-tuning_amd"))
    import torch
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    if not torch.cuda.is_available():
        raise SystemExit("response_grid_rate.py measures on the GPU and found none")
    R, B = args.resolution, args.envs
    env = VecQuantumDeviceEnv(B, num_dots=N, resolution=R, seed=1234, num_charge_states=K, capacitance_model=lambda img: (None, None))
    env.load_new_devices(seed=1234)
    L, C, G = env.L, N - 1, N + 1
    st, _ = env.get_state()
    par = env._params_host
    vgm = st[:, L.s_vgm:L.s_vgm + G * G].reshape(B, G, G)
    win = par[:, L.scal + 2]
    gt = np.concatenate([st[:, L.s_gate_gt:L.s_gate_gt + N], st[:, L.s_sensor_gt:L.s_sensor_gt + 1]], axis=1)
    phys = np.einsum("eij,ej->ei", vgm, gt) + par[:, L.origin:L.origin + G]
    bv = st[:, L.s_barrier_gt:L.s_barrier_gt + C]
    base = phys.copy(); base[:, 0] = 0.0; base[:, 1] = 0.0
    rgx = np.stack([phys[:, 0] - win, phys[:, 0] + win], axis=1)
    rgy = np.stack([phys[:, 1] - win, phys[:, 1] + win], axis=1)
    ids = np.arange(B)
    grid_args = (ids, 0, 1, rgx, rgy, R, R, base[:, :N], bv, KT, base[:, N])
    if args.route == "thermal":
        call = lambda: env.scan_grid_thermal(*grid_args, frame="physical")                            # noqa: E731
    elif args.route == "default":
        call = lambda: env.scan_grid_response(*grid_args, frame="physical")                           # noqa: E731
    elif args.route == "all":
        call = lambda: env.scan_grid_response(*grid_args, frame="physical", response=ALL)             # noqa: E731
    else:
        v = np.zeros((B, R, R, 2 * N))
        v[:, :, :, :G] = base[:, None, None, :]
        v[:, :, :, G:] = bv[:, None, None, :]
        for e in range(B):
            v[e, :, :, 0] = np.linspace(rgx[e, 0], rgx[e, 1], R)[None, :]
            v[e, :, :, 1] = np.linspace(rgy[e, 0], rgy[e, 1], R)[:, None]
        v = v.reshape(B, R * R, 2 * N)
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(env.device)      # noqa: E731
        vg_d, vb_d = dev(v[:, :, :G]), dev(v[:, :, G:])
        call = lambda: env.eval_points(ids, vg_d, vb_d, kT=KT, response=True)                         # noqa: E731
    call()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(args.calls):
        call()
    torch.cuda.synchronize(); t = (time.perf_counter() - t0) / args.calls
    env.close()
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dots", default="4,8")
    ap.add_argument("--states", default="32")
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--whole-lib", default=None)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--route", default="default", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        N, K = (int(x) for x in args.child.split(","))
        print(json.dumps(run(N, K, args)), flush=True)
        return
    common = ["--resolution", str(args.resolution), "--envs", str(args.envs), "--calls", str(args.calls)]
    routes = [("a", ["thermal"], {}), ("b", ["default"], {}), ("c", ["all"], {}), ("d", ["points"], {})]
    if args.whole_lib:
        routes.append(("e", ["default"], {"QDSIM_LIB": os.path.abspath(args.whole_lib)}))
    if args.parent_tree:
        routes.append(("p", ["thermal", "--tree", os.path.abspath(args.parent_tree)], {}))
    points = args.envs * args.resolution * args.resolution
    lines = []
    for N in args.dots.split(","):
        for K in args.states.split(","):
            t = {r: [] for r, _, _ in routes}
            for _ in range(args.repeats):
                for r, route, envv in routes:
                    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{N},{K}", "--route"] + route + common,
                                         check=True, stdout=subprocess.PIPE, text=True, env={**os.environ, **envv}).stdout
                    t[r].append(float(json.loads(res.strip().splitlines()[-1])))
            best = {r: min(x) for r, x in t.items()}
            spread = {r: (max(x) - min(x)) / min(x) for r, x in t.items()}
            out = {"n_dots": int(N), "num_charge_states": int(K), "points": points, "windows": args.repeats, "kT": KT}
            for r in t:
                out[r + "_s"] = round(best[r], 5)
                out[r + "_points_per_s"] = round(points / best[r])
                out[r + "_spread"] = round(spread[r], 3)
            out["b_over_a"] = round(best["b"] / best["a"], 3)
            out["c_over_a"] = round(best["c"] / best["a"], 3)
            out["d_over_b"] = round(best["d"] / best["b"], 3)
            if "e" in best:
                out["e_over_b"] = round(best["e"] / best["b"], 3)
                out["b_ahead_of_e"] = bool(best["e"] / best["b"] - 1.0 > max(spread["b"], spread["e"]))
            if "p" in best:
                out["a_over_p"] = round(best["a"] / best["p"], 3)
                out["a_within_spread_of_p"] = bool(abs(best["a"] / best["p"] - 1.0) <= max(spread["a"], spread["p"]))
            line = json.dumps(out)
            print(line, flush=True)
            lines.append(line + "\n")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.writelines(lines)


if __name__ == "__main__":
    main()
