"""Rate of point evaluation (qd_eval_points) beside the closest existing path, probe scans on a per-pixel-search handle.

    python scripts/points_rate.py [--dots 4,8] [--resolution 64] [--envs 64] [--repeats 3] [--only probe|full|lines]
                                  [--out profiles/points_rate.txt]

Per shape, on one `pixel_search` handle of `--envs` envs (each shape in a child process of its own; wall time, synchronised,
the first run of each route allocates its scratch and is not counted):
  probe   one probe scan per env at its own voltages: envs * C * P pixels through the per-pixel search
  full    one group per env of C * P random points near its ground truth (every slot full): the same number of points;
          signal alone, as a probe gives, and signal with occupations (a second ground-state solve at K = 32)
  lines   the same number of points as 64-point line cuts through the ground truth, one group each (every slot holds 64
          points and C * P - 64 padding records)
One JSON line per shape on stdout; --out appends them to a file as well.  `--only` runs one route alone (for a kernel trace
of its own)."""
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
    R, B = args.resolution, args.envs
    env = VecQuantumDeviceEnv(B, num_dots=N, resolution=R, seed=1234, pixel_search=True, capacitance_model=lambda img: (None, None))
    env.load_new_devices(seed=1234)
    L, C, G = env.L, N - 1, N + 1
    CP = C * R * R
    st, _ = env.get_state()
    par = env._params_host
    rng = np.random.default_rng(5)
    out = {"n_dots": N, "resolution": R, "envs": B, "chunk_envs": env.chunk_envs(), "points": B * CP}
    vgm = st[:, L.s_vgm:L.s_vgm + G * G].reshape(B, G, G)
    origin = par[:, L.origin:L.origin + G]

    def physical(e, virt):                                       # virtual plungers (n, N), sensor at its ground truth
        full = np.concatenate([virt, np.full((virt.shape[0], 1), st[e, L.s_sensor_gt])], axis=1)
        return full @ vgm[e].T + origin[e]

    def timed(fn):
        times = []
        for _ in range(args.repeats + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
        return times[1:]

    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(env.device)      # noqa: E731
    # probe scans at the envs' ground truth
    ids = dev(np.arange(B, dtype=np.int32))
    gv, bv = dev(st[:, L.s_gate_gt:L.s_gate_gt + N]), dev(st[:, L.s_barrier_gt:L.s_barrier_gt + C])
    sv = dev(st[:, L.s_sensor_gt])
    if args.only in (None, "probe"):
        t = timed(lambda: env.probe(ids, gv, bv, sensor_voltage=sv))
        out["probe_s"] = [round(x, 4) for x in t]
        out["probe_pixels_per_s"] = round(B * CP / min(t))
    # full groups: C P random points per env within the scan window of the ground truth
    win = par[:, L.scal + 2]
    vg = np.stack([physical(e, st[e, L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-win[e], win[e], (CP, N))) for e in range(B)])
    vb = st[:, None, L.s_barrier_gt:L.s_barrier_gt + C] + rng.uniform(-1, 1, (B, CP, C))
    vg_d, vb_d = dev(vg), dev(vb)
    if args.only in (None, "full"):
        t = timed(lambda: env.eval_points(np.arange(B), vg_d, vb_d, outputs=("signal",)))
        out["full_groups_s"] = [round(x, 4) for x in t]
        out["full_points_per_s"] = round(B * CP / min(t))
        # signal and occupations: the occupations come from a second solve of the sorted records (K = 32)
        t = timed(lambda: env.eval_points(np.arange(B), vg_d, vb_d))
        out["full_groups_both_s"] = [round(x, 4) for x in t]
        out["full_points_both_per_s"] = round(B * CP / min(t))
    if args.only not in (None, "lines"):
        env.close()
        return out
    # 64-point line cuts through the ground truth along a random direction, as many points in all
    n_lines = B * CP // 64
    env_of = np.arange(n_lines) % B
    s = np.linspace(-1.0, 1.0, 64)[None, :, None]
    d = rng.normal(size=(n_lines, 1, N)); d /= np.linalg.norm(d, axis=-1, keepdims=True)
    virt = st[env_of, None, L.s_gate_gt:L.s_gate_gt + N] + s * d * win[env_of, None, None]
    lg = np.stack([physical(env_of[k], virt[k]) for k in range(n_lines)])
    lb = np.broadcast_to(st[env_of, None, L.s_barrier_gt:L.s_barrier_gt + C], (n_lines, 64, C))
    lg_d, lb_d = dev(lg), dev(lb)
    t = timed(lambda: env.eval_points(env_of, lg_d, lb_d, outputs=("signal",)))
    out["line_cuts"] = n_lines
    out["line_cuts_s"] = [round(x, 4) for x in t]
    out["line_points_per_s"] = round(n_lines * 64 / min(t))
    if args.only is None:
        out["full_over_probe"] = round(out["full_points_per_s"] / out["probe_pixels_per_s"], 3)
        out["lines_over_full"] = round(out["line_points_per_s"] / out["full_points_per_s"], 4)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dots", default="4,8")
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default=None, choices=("probe", "full", "lines"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        print(json.dumps(run(int(args.child), args)), flush=True)
        return
    common = ["--resolution", str(args.resolution), "--envs", str(args.envs), "--repeats", str(args.repeats)]
    if args.only:
        common += ["--only", args.only]
    lines = []
    for N in args.dots.split(","):
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", N] + common, check=True,
                             stdout=subprocess.PIPE, text=True).stdout
        sys.stdout.write(res); sys.stdout.flush()
        lines.append(res)
    if args.out:
        with open(args.out, "a") as f:
            f.writelines(lines)


if __name__ == "__main__":
    main()
