"""Rate of the nx x ny grids (qd_scan_grid) against the routes such a grid had before them.

    python scripts/grid_rate.py [--dots 4,8] [--resolution 64] [--envs 64] [--repeats 5] [--calls 10] [--out profiles/grid_rate.txt]

Per shape a default handle and a pixel_search handle of `--envs` envs at `--resolution`^2 with the same devices; grids of
detuning "e1_2" (columns) against the on-site axis "U1_2" (rows) over +-window around the env's voltages, near the ground truth
as a tuned device, grid q on env q % envs.  Each shape in a child process of its own; per route two warm-up calls (the first
allocates scratch), then `--repeats` rounds in which the routes alternate, each round HIP events around `--calls` calls in a
row; best and median time per call, in grid points per second.
  (a) 1024 grids of 64 x 16 on the default handle
      grid     scan_grid, deterministic; grid+noise with sensor noise and latching
      points   the same points, built on the host by NumPy, through eval_points (signal only), one group per grid: the route a
               rectangular grid had before (deterministic only, no normalisation)
  (b) 64 grids of `--resolution` x `--resolution`
      grid          scan_grid on the default handle (the per-pixel search on a slot of its own)
      affine        scan_affine on the default handle (the tile search)
      affine_pixel  scan_affine on the pixel_search handle (the per-pixel search: the kernels scan_grid runs)
      grid_pixel    scan_grid on the pixel_search handle
      affine / grid is what the missing tile search costs a square grid.
One JSON line per shape on stdout; a table in `--out`."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-agent-for-qubit-array-tuning_amd"))

NOISE = ("sensor", "latch")


def run(N, args):
    import numpy as np
    import torch
    from qadapt_hip.vec_env import VecQuantumDeviceEnv, scan_axis_vector
    R, B = args.resolution, args.envs
    C, G = N - 1, N + 1
    envs = {}
    for name, ps in (("default", False), ("pixel", True)):
        envs[name] = VecQuantumDeviceEnv(B, num_dots=N, resolution=R, seed=1234, capacitance_model=lambda img: (None, None),
                                         pixel_search=ps)
        envs[name].load_new_devices(seed=1234)
    env = envs["default"]
    L = env.L
    st, _ = env.get_state()
    par = env._params_host
    rng = np.random.default_rng(5)
    gv0 = st[:, L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-3, 3, (B, N))         # near the ground truth, as a tuned device
    bv0 = st[:, L.s_barrier_gt:L.s_barrier_gt + C] + rng.uniform(-3, 3, (B, C))
    dx, dy = scan_axis_vector("e1_2", N), scan_axis_vector("U1_2", N)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3 / args.calls

    def measure(routes, points):
        for fn in routes.values():
            fn(); fn()
        ts = {k: [] for k in routes}
        for _ in range(args.repeats):
            for k, fn in routes.items():
                ts[k].append(timed(fn))
        return {k: {"best_s": round(min(t), 6), "median_s": round(statistics.median(t), 6), "points_per_s": round(points / min(t)),
                    "median_points_per_s": round(points / statistics.median(t))} for k, t in ts.items()}

    def queries(nq):
        ids = np.arange(nq) % B
        gv, bv, sv = gv0[ids], bv0[ids], st[ids, L.s_sensor_gt].copy()
        w = par[ids, L.scal + 2]
        return ids, gv, bv, sv, np.stack([-w, w], 1)

    rows = []
    # (a) many rectangular grids against one eval_points group per grid
    nq, nx, ny = 1024, 64, 16
    if nx * ny <= R * R:
        ids, gv, bv, sv, rg = queries(nq)
        lin = lambda n: rg[:, :1] + (rg[:, 1:] - rg[:, :1]) * np.linspace(0.0, 1.0, n)[None, :]     # noqa: E731
        W = (np.concatenate([gv, sv[:, None], bv], axis=1)[:, None, None, :] + lin(nx)[:, None, :, None] * dx
             + lin(ny)[:, :, None, None] * dy).reshape(nq, nx * ny, 2 * N)
        vgm = st[ids, L.s_vgm:L.s_vgm + G * G].reshape(nq, G, G)
        W[..., :G] = np.einsum("qij,qtj->qti", vgm, W[..., :G]) + par[ids, None, L.origin:L.origin + G]
        vg = torch.as_tensor(W[..., :G]).cuda().contiguous(); vb = torch.as_tensor(W[..., G:]).cuda().contiguous()
        gx = torch.as_tensor(gv).cuda(); bx = torch.as_tensor(bv).cuda(); sx = torch.as_tensor(sv).cuda()
        noisy = dict(noise=NOISE, serial=(1 << 63) | 9)
        routes = {"grid": lambda: env.scan_grid(ids, dx, dy, rg, rg, nx, ny, gx, bx, sx),
                  "grid+noise": lambda: env.scan_grid(ids, dx, dy, rg, rg, nx, ny, gx, bx, sx, **noisy),
                  "points": lambda: env.eval_points(ids, vg, vb, outputs=("signal",))}
        row = {"workload": "a", "grids": nq, "nx": nx, "ny": ny, **measure(routes, nq * nx * ny)}
        row["largest_difference_grid_points"] = float((routes["grid"]()["raw"].reshape(nq, -1) - routes["points"]()["signal"]).abs().max())
        row["grid_over_points"] = round(row["points"]["best_s"] / row["grid"]["best_s"], 2)
        rows.append(row)
    # (b) square grids against the images of scan_affine, with and without the tile search
    nq = 64
    ids, gv, bv, sv, rg = queries(nq)
    gx = torch.as_tensor(gv).cuda(); bx = torch.as_tensor(bv).cuda(); sx = torch.as_tensor(sv).cuda()
    routes = {"grid": lambda: envs["default"].scan_grid(ids, dx, dy, rg, rg, R, R, gx, bx, sx),
              "affine": lambda: envs["default"].scan_affine(ids, dx, dy, rg, rg, gx, bx, sensor_voltage=sx, normalised=True),
              "affine_pixel": lambda: envs["pixel"].scan_affine(ids, dx, dy, rg, rg, gx, bx, sensor_voltage=sx, normalised=True),
              "grid_pixel": lambda: envs["pixel"].scan_grid(ids, dx, dy, rg, rg, R, R, gx, bx, sx)}
    row = {"workload": "b", "grids": nq, "nx": R, "ny": R, **measure(routes, nq * R * R)}
    row["grid_equals_affine_pixel"] = bool(torch.equal(routes["grid"]()["raw"], routes["affine_pixel"]()["raw"]))
    row["largest_difference_grid_affine"] = float((routes["grid"]()["raw"] - routes["affine"]()["raw"]).abs().max())
    row["affine_over_grid"] = round(row["grid"]["best_s"] / row["affine"]["best_s"], 2)
    row["affine_pixel_over_grid"] = round(row["grid"]["best_s"] / row["affine_pixel"]["best_s"], 2)
    rows.append(row)
    out = {"n_dots": N, "resolution": R, "envs": B, "chunk_envs": env.chunk_envs(), "repeats": args.repeats, "calls": args.calls,
           "cases": rows}
    for e in envs.values():
        e.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dots", default="4,8")
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_rate.txt"))
    ap.add_argument("--child", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        run(args.child, args)
        return
    shapes = []
    for N in [int(x) for x in args.dots.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(N), "--resolution", str(args.resolution),
               "--envs", str(args.envs), "--repeats", str(args.repeats), "--calls", str(args.calls)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=400)
        if p.returncode != 0:
            raise SystemExit(f"shape {N} dots failed with status {p.returncode}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        shapes.append(json.loads(line))
    with open(args.out, "w") as f:
        f.write("scan_grid (e1_2 x U1_2 grids) against eval_points with one group per grid (a) and against scan_affine on a default and "
                f"on a pixel_search handle (b): HIP events around {args.calls} calls in a row, best of {args.repeats} alternated rounds "
                f"after two warm-up calls, {args.envs} envs at {args.resolution}x{args.resolution}; rates in grid points per second\n")
        f.write(f"{'dots':>4} {'case':>4} {'grids':>6} {'shape':>7} {'route':>13} {'points/s':>12} {'median':>12} {'ms/call':>9}\n")
        for sh in shapes:
            for r in sh["cases"]:
                for k in ("grid", "grid+noise", "points", "affine", "affine_pixel", "grid_pixel"):
                    if k in r:
                        f.write(f"{sh['n_dots']:>4} {r['workload']:>4} {r['grids']:>6} {str(r['nx']) + 'x' + str(r['ny']):>7} {k:>13} "
                                f"{r[k]['points_per_s']:>12} {r[k]['median_points_per_s']:>12} {1e3 * r[k]['best_s']:>9.3f}\n")
                if r["workload"] == "a":
                    f.write(f"{'':>4} {'':>4} scan_grid is {r['grid_over_points']}x eval_points on the same points\n")
                else:
                    f.write(f"{'':>4} {'':>4} scan_affine with the tile search is {r['affine_over_grid']}x scan_grid, with the per-pixel "
                            f"search {r['affine_pixel_over_grid']}x; grid == affine_pixel bit for bit: {r['grid_equals_affine_pixel']}\n")
        for sh in shapes:
            f.write(json.dumps(sh) + "\n")


if __name__ == "__main__":
    main()
