"""Rate of the affine axis scans (qd_scan_affine) against the route a handle had before them and against scan2d.

    python scripts/affine_rate.py [--dots 8,4] [--resolution 64] [--queries 64] [--repeats 5] [--out profiles/affine_rate.txt]

Workload per shape: `--queries` images of `--resolution`^2 pixels on a default handle of `--queries` envs, deterministic, as
detuning against on-site scans ("e1_2" x "U1_2", each over +-window around the env's voltages, near the ground truth as a
tuned device).  Each shape in a child process of its own; HIP events around every call, two warm-up calls per route (the
first allocates scratch), then `--repeats` rounds in which the three routes alternate; best and median per route.
  (a) affine   scan_affine
  (b) points   the same grids, built on the host by NumPy, through eval_points (signal only) on the same handle: the route
               combination axes had before; its code is that of the parent commit, so this is the baseline
  (c) scan2d   scan2d on the two plungers vP1, vP2 over ranges of equal span: what the affine front end and any extra redo
               work on diagonal axes cost
One JSON line per shape on stdout; a table in `--out`."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-agent-for-qubit-array-tuning_amd"))


def run(N, args):
    import numpy as np
    import torch
    from qadapt_hip.vec_env import VecQuantumDeviceEnv, scan_axis_vector
    R, nq = args.resolution, args.queries
    C, G, P = N - 1, N + 1, R * R
    env = VecQuantumDeviceEnv(nq, num_dots=N, resolution=R, seed=1234, capacitance_model=lambda img: (None, None))
    env.load_new_devices(seed=1234)
    L = env.L
    st, _ = env.get_state()
    par = env._params_host
    rng = np.random.default_rng(5)
    gv = st[:, L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-3, 3, (nq, N))         # near the ground truth, as a tuned device
    bv = st[:, L.s_barrier_gt:L.s_barrier_gt + C] + rng.uniform(-3, 3, (nq, C))
    sv = st[:, L.s_sensor_gt].copy()
    w = par[:, L.scal + 2]
    ids = np.arange(nq)
    dx, dy = scan_axis_vector("e1_2", N), scan_axis_vector("U1_2", N)
    rg = np.stack([-w, w], 1)
    # the physical voltages of every pixel, (nq, P, 2N), as the virtual frame forms them
    t = np.linspace(0.0, 1.0, R)
    s = rg[:, :1] + (rg[:, 1:] - rg[:, :1]) * t[None, :]                            # (nq, R): the same scalar on both axes
    W = np.concatenate([gv, sv[:, None], bv], axis=1)[:, None, None, :] + s[:, None, :, None] * dx + s[:, :, None, None] * dy
    vgm = st[:, L.s_vgm:L.s_vgm + G * G].reshape(nq, G, G)
    W[..., :G] = np.einsum("qij,q...j->q...i", vgm, W[..., :G]) + par[:, None, None, L.origin:L.origin + G]
    pts = W.reshape(nq, P, 2 * N)
    vg = torch.as_tensor(pts[..., :G]).cuda().contiguous(); vb = torch.as_tensor(pts[..., G:]).cuda().contiguous()
    gx = torch.as_tensor(gv).cuda(); bx = torch.as_tensor(bv).cuda(); sx = torch.as_tensor(sv).cuda()
    xr2, yr2 = np.stack([gv[:, 0] - w, gv[:, 0] + w], 1), np.stack([gv[:, 1] - w, gv[:, 1] + w], 1)
    routes = {"affine": lambda: env.scan_affine(ids, dx, dy, rg, rg, gx, bx, sensor_voltage=sx),
              "points": lambda: env.eval_points(ids, vg, vb, outputs=("signal",)),
              "scan2d": lambda: env.scan2d(ids, 0, 1, xr2, yr2, gx, bx, sensor_voltage=sx)}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    for fn in routes.values():
        fn(); fn()
    ts = {k: [] for k in routes}
    for _ in range(args.repeats):
        for k, fn in routes.items():
            ts[k].append(timed(fn))
    raw = routes["affine"]()["raw"].reshape(nq, P)
    sig = routes["points"]()["signal"]
    pix = nq * P
    out = {"n_dots": N, "resolution": R, "queries": nq, "chunk_envs": env.chunk_envs(), "repeats": args.repeats,
           "largest_difference_affine_points": float((raw - sig).abs().max())}
    for k in routes:
        out[k] = {"best_s": round(min(ts[k]), 6), "median_s": round(statistics.median(ts[k]), 6),
                  "pix_per_s": round(pix / min(ts[k])), "median_pix_per_s": round(pix / statistics.median(ts[k]))}
    out["affine_over_points"] = round(min(ts["points"]) / min(ts["affine"]), 3)
    out["affine_over_scan2d"] = round(min(ts["scan2d"]) / min(ts["affine"]), 3)
    env.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dots", default="8,4")
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affine_rate.txt"))
    ap.add_argument("--child", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        run(args.child, args)
        return
    rows = []
    for N in [int(x) for x in args.dots.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(N), "--resolution", str(args.resolution),
               "--queries", str(args.queries), "--repeats", str(args.repeats)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=300)
        if p.returncode != 0:
            raise SystemExit(f"shape {N} dots failed with status {p.returncode}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        rows.append(json.loads(line))
    with open(args.out, "w") as f:
        f.write("scan_affine (e1_2 x U1_2) against eval_points on the same grids and scan2d (vP1 x vP2, equal span): deterministic, "
                f"HIP events around a call, best of {args.repeats} alternated rounds, {args.queries} images of "
                f"{args.resolution}x{args.resolution}, default handle\n")
        f.write(f"{'dots':>4} {'affine pix/s':>14} {'points pix/s':>14} {'scan2d pix/s':>14} {'affine / points':>16} {'affine / scan2d':>16}\n")
        for r in rows:
            f.write(f"{r['n_dots']:>4} {r['affine']['pix_per_s']:>14} {r['points']['pix_per_s']:>14} {r['scan2d']['pix_per_s']:>14} "
                    f"{r['affine_over_points']:>16} {r['affine_over_scan2d']:>16}\n")
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
