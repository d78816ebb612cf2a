"""Rate of the axis scans (qd_scan2d) against the routes a handle had before them.

    python scripts/scan_rate.py [--dots 8,4] [--resolution 64] [--queries 64] [--repeats 3] [--out profiles/scan_rate.txt]

Workload per shape: `--queries` images of `--resolution`^2 pixels on a default handle of `--queries` envs, deterministic,
wall time of a synchronised call, best of `--repeats`; each shape in a child process of its own.
  scan2d   plunger-vs-barrier images (vP1 against B1) and adjacent-pair images (vP1 against vP2); the adjacent-pair images
           once more with sensor noise and latching on
  points   the same grids, built on the host by NumPy, through eval_points on the same handle
  probe    probes at the same voltages: pixels per second divided by C, the channels a probe renders for one image
Also the share of the tile search's tiles and pixels handed to the exact per-pixel search on the same voltages
(search_stats of a validate handle, for the adjacent pair: the env's own pattern; the barrier axis is not reachable by a
validate handle, which renders no scans).  One JSON line per shape on stdout; a table in `--out`."""
import argparse
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
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
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
    out = {"n_dots": N, "resolution": R, "queries": nq, "chunk_envs": env.chunk_envs()}

    def best(fn):
        ts = []
        for _ in range(args.repeats + 1):                         # the first run allocates scratch: not counted
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
        return min(ts[1:])

    def grid(ax, ay, xr, yr):
        """the physical voltages of every pixel, (nq, P, 2N), as scan2d's virtual frame forms them"""
        W = np.concatenate([gv, sv[:, None], bv], axis=1)
        Wg = np.broadcast_to(W[:, None, None, :], (nq, R, R, 2 * N)).copy()
        t = np.linspace(0.0, 1.0, R)
        Wg[:, :, :, ax] = (xr[:, :1] + (xr[:, 1:] - xr[:, :1]) * t[None, :])[:, None, :]
        Wg[:, :, :, ay] = (yr[:, :1] + (yr[:, 1:] - yr[:, :1]) * t[None, :])[:, :, None]
        vgm = st[:, L.s_vgm:L.s_vgm + G * G].reshape(nq, G, G)
        Wg[..., :G] = np.einsum("qij,q...j->q...i", vgm, Wg[..., :G]) + par[:, None, None, L.origin:L.origin + G]
        return Wg.reshape(nq, P, 2 * N)

    cases = {"plunger_barrier": (0, N + 1, np.stack([gv[:, 0] - w, gv[:, 0] + w], 1), np.stack([bv[:, 0] - 3, bv[:, 0] + 3], 1)),
             "adjacent_pair": (0, 1, np.stack([gv[:, 0] - w, gv[:, 0] + w], 1), np.stack([gv[:, 1] - w, gv[:, 1] + w], 1))}
    pix = nq * P
    for name, (ax, ay, xr, yr) in cases.items():
        gx = torch.as_tensor(gv).cuda(); bx = torch.as_tensor(bv).cuda(); sx = torch.as_tensor(sv).cuda()
        t_scan = best(lambda: env.scan2d(ids, ax, ay, xr, yr, gx, bx, sensor_voltage=sx))
        pts = grid(ax, ay, xr, yr)
        vg = torch.as_tensor(pts[..., :G]).cuda().contiguous(); vb = torch.as_tensor(pts[..., G:]).cuda().contiguous()
        t_pts = best(lambda: env.eval_points(ids, vg, vb, outputs=("signal",)))
        raw = env.scan2d(ids, ax, ay, xr, yr, gx, bx, sensor_voltage=sx)["raw"].reshape(nq, P)
        sig = env.eval_points(ids, vg, vb, outputs=("signal",))["signal"]
        out[name] = {"scan2d_s": round(t_scan, 5), "scan2d_pix_per_s": round(pix / t_scan), "points_s": round(t_pts, 5),
                     "points_pix_per_s": round(pix / t_pts), "scan_over_points": round(t_pts / t_scan, 3),
                     "largest_difference": float((raw - sig).abs().max())}
    t_probe = best(lambda: env.probe(ids, gx, bx, sensor_voltage=sx))
    out["probe"] = {"probe_s": round(t_probe, 5), "pix_per_s_over_C": round(pix * C / t_probe / C),
                    "scan_over_probe_per_image": round((t_probe / C) / out["adjacent_pair"]["scan2d_s"], 3)}
    ax, ay, xr, yr = cases["adjacent_pair"]
    t_noisy = best(lambda: env.scan2d(ids, ax, ay, xr, yr, gx, bx, sensor_voltage=sx, noise=("sensor", "latch"), serial=1 << 63))
    out["adjacent_pair_sensor_latch"] = {"scan2d_s": round(t_noisy, 5), "scan2d_pix_per_s": round(pix / t_noisy)}
    env.close()
    # what the tile search hands to the per-pixel search at these voltages (the env's own pattern; all channels)
    val = VecQuantumDeviceEnv(min(nq, 8), num_dots=N, resolution=R, seed=1234, validate=True, capacitance_model=lambda img: (None, None))
    val.load_new_devices(seed=1234)
    s2, steps = val.get_state()
    s2[:, L.s_gate_v:L.s_gate_v + N] = gv[:val.B]; s2[:, L.s_barrier_v:L.s_barrier_v + C] = bv[:val.B]
    val.set_state(s2, steps); val.observe()
    s = val.search_stats()
    out["search_stats_env_pattern"] = {k: int(v) for k, v in s.items() if isinstance(v, (int, np.integer))}
    val.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dots", default="8,4")
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_rate.txt"))
    ap.add_argument("--child", type=int, default=0)
    args = ap.parse_args()
    if args.child:
        run(args.child, args)
        return
    rows = []
    for N in [int(x) for x in args.dots.split(",")]:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(N), "--resolution", str(args.resolution),
               "--queries", str(args.queries), "--repeats", str(args.repeats)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=500)
        if p.returncode != 0:
            raise SystemExit(f"shape {N} dots failed with status {p.returncode}")
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
        print(line, flush=True)
        rows.append(json.loads(line))
    with open(args.out, "w") as f:
        f.write("scan2d against eval_points and probe: deterministic, wall time of a synchronised call, best of "
                f"{args.repeats}, {args.queries} images of {args.resolution}x{args.resolution}, default handle\n")
        f.write(f"{'dots':>4} {'image':<26} {'scan2d pix/s':>14} {'points pix/s':>14} {'probe pix/s / C':>16} {'scan / points':>14}\n")
        for r in rows:
            for name in ("plunger_barrier", "adjacent_pair"):
                c = r[name]
                pr = r["probe"]["pix_per_s_over_C"] if name == "adjacent_pair" else ""
                f.write(f"{r['n_dots']:>4} {name:<26} {c['scan2d_pix_per_s']:>14} {c['points_pix_per_s']:>14} {pr:>16} {c['scan_over_points']:>14}\n")
            c = r["adjacent_pair_sensor_latch"]
            f.write(f"{r['n_dots']:>4} {'adjacent_pair sensor+latch':<26} {c['scan2d_pix_per_s']:>14}\n")
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
