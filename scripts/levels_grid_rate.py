"""Rate of energy-level grids (qd_scan_grid_levels, scan_grid_levels) beside the routes that gave the same levels and images before
it existed, and beside the same kernel on the whole-block core.

    python scripts/levels_grid_rate.py [--dots 4,8] [--states 32,8] [--levels 2,8] [--resolution 64] [--envs 64] [--repeats 3]
                                       [--rounds 3] [--calls 2] [--parent-tree DIR] [--whole-lib FILE]
                                       [--out profiles/levels_grid_rate.txt]

Per configuration (N dots, K = num_charge_states) on the handle of scripts/thermal_grid_rate.py: `--envs` envs at R x R, one grid
of R x R points per env in the physical frame, plungers 1 and 2 over the env's scan window around its working point, every other
control at the working point.  Open regime, and a closed series at n_charge = N.  The routes, each in child processes of its own:
  a  grid     scan_grid_levels(..., levels=L): search + qd_k_levels_grid + ground state, sensor, pack, percentiles, write
  b  points   eval_points(levels=L, outputs=()) at the grid's voltages (built in NumPy, uploaded once, outside the windows), one
              group per grid, plus scan_grid / scan_grid_closed: the routes that existed before, identical on the parent commit.
              With --parent-tree (a checkout of the parent commit with its library built) the children of this route import the
              package and load the library of THAT tree
  c  whole    route a on a library built with -DQD_LVG_FORCE_WHOLE (--whole-lib, scripts/ab_build.sh): the open regime through
              qd_k_levels_grid on the whole-block core.  Measurement only
Wall time around `--calls` calls ending in a device synchronise; inside a child the first window of each case allocates its
scratch and is not counted, the best of `--repeats` windows is the child's figure.  The routes are alternated `--rounds` times
(b, a, c, b, a, c, ..: a fresh process each); the figure of a route is the best over its rounds, and the SPREAD of route b over
its rounds, (worst - best) / best of the children's figures, is the run-to-run spread the verdicts are judged against:
  a_ahead_of_c   t_c / t_a - 1 > spread_b: the per-component core earns its place in this configuration (open regime)
  a_ahead_of_b   t_b / t_a - 1 > spread_b
One JSON line per configuration, L and regime on stdout; --out appends them to a file as well."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(N, K, args):
    """one child: every L and both regimes of one configuration through one route; {(L, regime): best seconds per call}"""
    tree = args.tree or ROOT
    sys.path.insert(0, os.path.join(tree, "rl-agent-for-qubit-array-tuning_amd"))
    import torch
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    if not torch.cuda.is_available():
        raise SystemExit("levels_grid_rate.py measures on the GPU and found none")
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
    v = np.zeros((B, R, R, 2 * N))
    v[:, :, :, :G] = base[:, None, None, :]
    v[:, :, :, G:] = bv[:, None, None, :]
    for e in range(B):
        v[e, :, :, 0] = np.linspace(rgx[e, 0], rgx[e, 1], R)[None, :]
        v[e, :, :, 1] = np.linspace(rgy[e, 0], rgy[e, 1], R)[:, None]
    v = v.reshape(B, R * R, 2 * N)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(env.device)      # noqa: E731
    vg_d, vb_d, ids = dev(v[:, :, :G]), dev(v[:, :, G:]), np.arange(B)
    grid_args = (ids, 0, 1, rgx, rgy, R, R, base[:, :N], bv)
    out = {}
    for nl in (int(x) for x in args.levels.split(",")):
        for regime in ("open", "closed"):
            q = None if regime == "open" else N
            if args.route == "points":
                def call():
                    env.eval_points(ids, vg_d, vb_d, n_charge=q, outputs=(), levels=nl)
                    if q is None:
                        env.scan_grid(*grid_args, base[:, N], frame="physical")
                    else:
                        env.scan_grid_closed(*grid_args, q, base[:, N], frame="physical")
            else:
                def call():
                    env.scan_grid_levels(*grid_args, base[:, N], levels=nl, n_charge=q, frame="physical")
            ts = []
            for rep in range(args.repeats + 1):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(args.calls):
                    call()
                torch.cuda.synchronize(); t = (time.perf_counter() - t0) / args.calls
                if rep > 0:
                    ts.append(t)
            out[f"{nl},{regime}"] = min(ts)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dots", default="4,8")
    ap.add_argument("--states", default="32,8")
    ap.add_argument("--levels", default="2,8")
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--whole-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--route", default="grid", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        N, K = (int(x) for x in args.child.split(","))
        print(json.dumps(run(N, K, args)), flush=True)
        return
    common = ["--levels", args.levels, "--resolution", str(args.resolution), "--envs", str(args.envs), "--repeats", str(args.repeats),
              "--calls", str(args.calls)]
    routes = [("b", ["--route", "points"] + (["--tree", os.path.abspath(args.parent_tree)] if args.parent_tree else []), {}),
              ("a", ["--route", "grid"], {})]
    if args.whole_lib:
        routes.append(("c", ["--route", "grid"], {"QDSIM_LIB": os.path.abspath(args.whole_lib)}))
    points = args.envs * args.resolution * args.resolution
    lines = []
    for N in args.dots.split(","):
        for K in args.states.split(","):
            figs = {r: [] for r, _, _ in routes}
            for _ in range(args.rounds):
                for r, extra, envv in routes:
                    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", f"{N},{K}"] + common + extra, check=True,
                                         stdout=subprocess.PIPE, text=True, env={**os.environ, **envv}).stdout
                    figs[r].append(json.loads(res.strip().splitlines()[-1]))
            for case in figs["a"][0]:
                nl, regime = case.split(",")
                t = {r: [f[case] for f in figs[r]] for r in figs}
                best = {r: min(x) for r, x in t.items()}
                spread = (max(t["b"]) - best["b"]) / best["b"]
                out = {"n_dots": int(N), "num_charge_states": int(K), "levels": int(nl), "regime": regime, "points": points,
                       "rounds": args.rounds, "b_on_parent_tree": bool(args.parent_tree), "spread_b": round(spread, 3)}
                for r in t:
                    out[r + "_s"] = round(best[r], 5)
                    out[r + "_points_per_s"] = round(points / best[r])
                    out[r + "_rounds_s"] = [round(x, 5) for x in t[r]]
                out["b_over_a"] = round(best["b"] / best["a"], 3)
                out["a_ahead_of_b"] = bool(best["b"] / best["a"] - 1.0 > spread)
                if "c" in best:
                    out["c_over_a"] = round(best["c"] / best["a"], 3)
                    out["a_ahead_of_c"] = bool(best["c"] / best["a"] - 1.0 > spread)
                line = json.dumps(out)
                print(line, flush=True)
                lines.append(line + "\n")
    if args.out:
        with open(args.out, "a") as f:
            f.writelines(lines)


if __name__ == "__main__":
    main()
