"""Rate of the dense 1-D sweeps (qd_scan1d) against the two routes a line cut had before them.

    python scripts/line_rate.py [--dots 4,8] [--resolution 64] [--envs 64] [--repeats 5] [--out profiles/line_rate.txt]

Workload per shape: a default handle of `--envs` envs at `--resolution`^2; detuning lines ("e1_2" over +-window around the env's
voltages, near the ground truth as a tuned device), line q on env q % envs: 64 and 1024 lines of 64 points and 64 lines of 4096
points, deterministic and with sensor noise and latching.  Each shape in a child process of its own; HIP events around every
synchronised call, two warm-up calls per route (the first allocates scratch), then `--repeats` rounds in which the routes
alternate; best and median per route, in line points per second.
  (a) scan1d   scan1d
  (b) points   the same lines, built on the host by NumPy, through eval_points (signal only), one group per line: the route a
               line cut had before; its code is that of the parent commit, so this is the baseline.  Deterministic only
  (c) affine   scan_affine with dx = the line's direction and dy = 0: R rows, all equal, of which ONE is counted.  Only for
               lines of `--resolution` points (a row has that many); its latching and telegraph chains are those of an image
One JSON line per shape on stdout; a table in `--out`."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-agent-for-qubit-array-tuning_amd"))

CASES = [(64, 64), (1024, 64), (64, 4096)]           # (lines, points per line)
NOISE = ("sensor", "latch")


def run(N, args):
    import numpy as np
    import torch
    from qadapt_hip.vec_env import VecQuantumDeviceEnv, scan_axis_vector
    R, B = args.resolution, args.envs
    C, G = N - 1, N + 1
    env = VecQuantumDeviceEnv(B, num_dots=N, resolution=R, seed=1234, capacitance_model=lambda img: (None, None))
    env.load_new_devices(seed=1234)
    L = env.L
    st, _ = env.get_state()
    par = env._params_host
    rng = np.random.default_rng(5)
    gv0 = st[:, L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-3, 3, (B, N))         # near the ground truth, as a tuned device
    bv0 = st[:, L.s_barrier_gt:L.s_barrier_gt + C] + rng.uniform(-3, 3, (B, C))
    d = scan_axis_vector("e1_2", N)
    zero = np.zeros(2 * N)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    rows = []
    for nl, n in CASES:
        if n > R * R:
            continue
        ids = np.arange(nl) % B
        gv, bv, sv = gv0[ids], bv0[ids], st[ids, L.s_sensor_gt].copy()
        w = par[ids, L.scal + 2]
        rg = np.stack([-w, w], 1)
        # the physical voltages of every point, (nl, n, 2N), as the virtual frame forms them
        s = rg[:, :1] + (rg[:, 1:] - rg[:, :1]) * np.linspace(0.0, 1.0, n)[None, :]
        W = np.concatenate([gv, sv[:, None], bv], axis=1)[:, None, :] + s[:, :, None] * d
        vgm = st[ids, L.s_vgm:L.s_vgm + G * G].reshape(nl, G, G)
        W[..., :G] = np.einsum("qij,qtj->qti", vgm, W[..., :G]) + par[ids, None, L.origin:L.origin + G]
        vg = torch.as_tensor(W[..., :G]).cuda().contiguous(); vb = torch.as_tensor(W[..., G:]).cuda().contiguous()
        gx = torch.as_tensor(gv).cuda(); bx = torch.as_tensor(bv).cuda(); sx = torch.as_tensor(sv).cuda()
        for noisy in (False, True):
            kw = dict(noise=NOISE, serial=(1 << 63) | 9) if noisy else {}
            routes = {"scan1d": lambda: env.scan1d(ids, d, rg, n, gx, bx, sx, **kw)}
            if not noisy:
                routes["points"] = lambda: env.eval_points(ids, vg, vb, outputs=("signal",))
            if n == R:
                routes["affine"] = lambda: env.scan_affine(ids, d, zero, rg, (0.0, 0.0), gx, bx, sensor_voltage=sx, **kw)
            for fn in routes.values():
                fn(); fn()
            ts = {k: [] for k in routes}
            for _ in range(args.repeats):
                for k, fn in routes.items():
                    ts[k].append(timed(fn))
            row = {"lines": nl, "points_per_line": n, "noise": list(NOISE) if noisy else []}
            raw = routes["scan1d"]()["raw"]
            if "points" in routes:
                row["largest_difference_scan1d_points"] = float((raw - routes["points"]()["signal"]).abs().max())
            if "affine" in routes:
                row["largest_difference_scan1d_affine_row0"] = float((raw - routes["affine"]()["raw"][:, 0]).abs().max())
            for k in routes:
                row[k] = {"best_s": round(min(ts[k]), 6), "median_s": round(statistics.median(ts[k]), 6),
                          "points_per_s": round(nl * n / min(ts[k])), "median_points_per_s": round(nl * n / statistics.median(ts[k]))}
            for k in ("points", "affine"):
                if k in routes:
                    row[f"scan1d_over_{k}"] = round(min(ts[k]) / min(ts["scan1d"]), 2)
            rows.append(row)
    out = {"n_dots": N, "resolution": R, "envs": B, "chunk_envs": env.chunk_envs(), "repeats": args.repeats, "cases": rows}
    env.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dots", default="4,8")
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "line_rate.txt"))
    ap.add_argument("--child", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        run(args.child, args)
        return
    shapes = []
    for N in [int(x) for x in args.dots.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(N), "--resolution", str(args.resolution),
               "--envs", str(args.envs), "--repeats", str(args.repeats)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=400)
        if p.returncode != 0:
            raise SystemExit(f"shape {N} dots failed with status {p.returncode}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        shapes.append(json.loads(line))
    with open(args.out, "w") as f:
        f.write("scan1d (e1_2 lines) against eval_points with one group per line and scan_affine with dy = 0 (one row counted): HIP "
                f"events around a synchronised call, best of {args.repeats} alternated rounds after two warm-up calls, {args.envs} envs "
                f"at {args.resolution}x{args.resolution}, default handle; rates in line points per second\n")
        f.write(f"{'dots':>4} {'lines':>6} {'points':>6} {'noise':>13} {'scan1d':>12} {'points':>12} {'affine':>12} {'scan1d/points':>14} "
                f"{'scan1d/affine':>14} {'fastest':>8}\n")
        for sh in shapes:
            for r in sh["cases"]:
                rate = lambda k: r[k]["points_per_s"] if k in r else "-"      # noqa: E731
                best = max((k for k in ("scan1d", "points", "affine") if k in r), key=lambda k: r[k]["points_per_s"])
                f.write(f"{sh['n_dots']:>4} {r['lines']:>6} {r['points_per_line']:>6} {'+'.join(r['noise']) or 'none':>13} "
                        f"{rate('scan1d'):>12} {rate('points'):>12} {rate('affine'):>12} {r.get('scan1d_over_points', '-'):>14} "
                        f"{r.get('scan1d_over_affine', '-'):>14} {best:>8}\n")
        for sh in shapes:
            f.write(json.dumps(sh) + "\n")


if __name__ == "__main__":
    main()
