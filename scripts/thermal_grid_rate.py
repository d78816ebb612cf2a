"""Rate of finite-temperature grids (qd_scan_grid_thermal, scan_grid_thermal) beside the route that rendered the same points
before it existed and the same grid at T = 0.

    python scripts/thermal_grid_rate.py [--dots 4,8] [--states 32,8] [--resolution 64] [--envs 64] [--repeats 3] [--calls 2]
                                        [--census 256] [--out profiles/thermal_grid_rate.txt]

Per configuration (N dots, K = num_charge_states), each in a child process of its own, on one handle of `--envs` envs at R x R:
one grid of R x R points per env in the physical frame, plungers 1 and 2 over the env's scan window around its working point, every
other control at the working point, kT = 8.617333262145e-5 * 100.  Open regime, and a closed series at n_charge = N.
  grid      scan_grid_thermal(..., kT, occupations=True, variance=True, ztail=True): search + qd_k_thermal_grid + sensor, pack, percentiles, write
  points    eval_points(kT=kT, outputs=("signal", "occupations", "variance", "ztail")) at the grid's voltages (built in NumPy,
            uploaded once, outside the windows), one group per grid: search + qd_k_thermal + write -- the route before
  cold      scan_grid(occupations=True) at T = 0, for scale
Wall time around `--calls` calls ending in a device synchronise; the routes alternate inside every repeat, the first window of
each route allocates its scratch and is not counted, the best window of `--repeats` counts and the spread (worst - best) / best
of the counted windows is reported beside it.  grid_over_points is the ratio of the best times.
`--census n`: for n points of env 0's grid, from the oracle's kept lists alone (no device): the histogram of the LARGEST hop
component per point, and the sweeps per point of the host build of the core (tests/hosttest_thermal_blocks), when it is built.
One JSON line per configuration and regime on stdout; --out appends them to a file as well."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "rl-agent-for-qubit-array-tuning_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, _p)

KT = 8.617333262145e-5 * 100
ALL = ("signal", "occupations", "variance", "ztail")


def census(N, K, par, v_ext, n_points):
    """largest hop component per point and host sweeps per point, over n_points rows of v_ext spread evenly"""
    import helpers as H
    import qd_oracle as O
    pick = np.linspace(0, v_ext.shape[0] - 1, n_points).astype(int)
    v = v_ext[pick]
    dev = H.dev_view(N, par)
    vg, vb = v[:, :N + 1], v[:, N + 1:]
    states, n_cont = O.candidate_states(v, dev.cdd_inv_full, dev.cgd_full, N, k=K)
    nv = np.minimum(np.all(O._delta_table(N)[None] + np.floor(n_cont)[:, None, :] >= 0, axis=-1).sum(axis=1), K)
    with np.errstate(under="ignore"):
        tc = O.tunnel_couplings(O.effective_barrier_potential(vg, vb, dev.Cbg, dev.Cbb), dev.tc_base, dev.alpha)
    lib = None
    path = os.path.join(ROOT, "tests", "hosttest_thermal_blocks", "libqdsim_hosttest_thermal_blocks.so")
    if os.path.exists(path):
        lib = ctypes.CDLL(path)
    largest, sweeps = np.zeros(33, np.int64), []
    for p in range(n_points):
        k = int(nv[p])
        st = states[p:p + 1, :k].astype(np.int64)
        F = O.free_energy_states(v[p:p + 1], dev.cdd_inv_full, dev.cgd_full, st, N)[0]
        with np.errstate(under="ignore"):
            Hm = np.diag(F) + O.tunnel_hamiltonian(tc[p:p + 1], st)[0]
        lab = np.arange(k)
        link = (Hm != 0) & ~np.eye(k, dtype=bool)
        for _ in range(k):
            new = np.array([min(lab[i], lab[link[i]].min() if link[i].any() else lab[i]) for i in range(k)])
            if np.array_equal(new, lab):
                break
            lab = new
        largest[np.bincount(lab).max()] += 1
        if lib is not None:
            dp = ctypes.POINTER(ctypes.c_double)
            pk = np.ascontiguousarray(Hm[np.tril_indices(k)])
            o = [np.zeros(k), np.zeros(k), np.zeros((k, k)), np.zeros(1)]
            labs = np.zeros(k, np.int32)
            sweeps.append(lib.qdtb_thermal(k, pk.ctypes.data_as(dp), ctypes.c_double(KT), *[a.ctypes.data_as(dp) for a in o],
                                           labs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None))
    out = {"census_points": int(n_points), "largest_component": {str(s): int(c) for s, c in enumerate(largest) if c}}
    if sweeps:
        out["host_sweeps_mean"] = round(float(np.mean(sweeps)), 2)
        out["host_sweeps_max"] = int(np.max(sweeps))
    return out


def run(N, K, args):
    import torch
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    if not torch.cuda.is_available():
        raise SystemExit("thermal_grid_rate.py measures on the GPU and found none")
    R, B = args.resolution, args.envs
    env = VecQuantumDeviceEnv(B, num_dots=N, resolution=R, seed=1234, num_charge_states=K, capacitance_model=lambda img: (None, None))
    env.load_new_devices(seed=1234)
    L, C, G = env.L, N - 1, N + 1
    st, _ = env.get_state()
    par = env._params_host
    vgm = st[:, L.s_vgm:L.s_vgm + G * G].reshape(B, G, G)
    win = par[:, L.scal + 2]
    # the physical working point of every env; the swept plungers are 0 in the base point and carry it in their ranges, so
    # that NumPy's linspace builds the grid's voltages with the bits of the front end
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
    lines = []
    for regime in ("open", "closed"):
        q = None if regime == "open" else N
        if q is None:
            routes = (("grid", lambda: env.scan_grid_thermal(*grid_args, KT, base[:, N], frame="physical", occupations=True, variance=True,
                                                             ztail=True)),
                      ("points", lambda: env.eval_points(ids, vg_d, vb_d, kT=KT, outputs=ALL)),
                      ("cold", lambda: env.scan_grid(*grid_args, base[:, N], frame="physical", occupations=True)))
        else:
            routes = (("grid", lambda: env.scan_grid_thermal(*grid_args, KT, base[:, N], n_charge=q, frame="physical", occupations=True,
                                                             variance=True, ztail=True)),
                      ("points", lambda: env.eval_points(ids, vg_d, vb_d, n_charge=q, kT=KT, outputs=ALL)),
                      ("cold", lambda: env.scan_grid_closed(*grid_args, q, base[:, N], frame="physical", occupations=True)))
        times = {name: [] for name, _ in routes}
        for rep in range(args.repeats + 1):
            for name, call in routes:
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(args.calls):
                    call()
                torch.cuda.synchronize(); t = (time.perf_counter() - t0) / args.calls
                if rep > 0:
                    times[name].append(t)
        out = {"n_dots": N, "num_charge_states": K, "regime": regime, "resolution": R, "envs": B, "points": B * R * R, "kT": KT,
               "calls_per_window": args.calls}
        for name, _ in routes:
            best = min(times[name])
            out[name + "_s"] = round(best, 5)
            out[name + "_points_per_s"] = round(B * R * R / best)
            out[name + "_spread"] = round((max(times[name]) - best) / best, 3)
        out["grid_over_points"] = round(min(times["grid"]) / min(times["points"]), 3)
        out["grid_over_cold"] = round(min(times["grid"]) / min(times["cold"]), 3)
        a, b = routes[0][1](), routes[1][1]()
        d = (a["occupations"].reshape(B, R * R, N) - b["occupations"]).abs().max()
        out["max_occupation_difference_grid_points"] = float(d)
        out["ztail_above_1e-6"] = round(float((a["ztail"] > 1e-6).double().mean()), 4)
        if regime == "open" and args.census > 0:
            out.update(census(N, K, par[0], v[0], args.census))
        lines.append(json.dumps(out))
    env.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dots", default="4,8")
    ap.add_argument("--states", default="32,8")
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--census", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        N, K = (int(x) for x in args.child.split(","))
        for line in run(N, K, args):
            print(line, flush=True)
        return
    common = ["--resolution", str(args.resolution), "--envs", str(args.envs), "--repeats", str(args.repeats), "--calls", str(args.calls),
              "--census", str(args.census)]
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
