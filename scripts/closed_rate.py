"""Rate of closed point evaluation (qd_eval_points_closed) beside open point evaluation (qd_eval_points) on the same handle and
the same points.

    python scripts/closed_rate.py [--dots 4,8] [--states 32,8] [--resolution 32] [--envs 16] [--repeats 3]
                                  [--out profiles/closed_rate.txt]

Per configuration (N dots, K = num_charge_states), on one handle of `--envs` envs, each configuration in a child process of
its own: one group per env of C * P random points within the scan window of its ground truth (every slot full), signal and
occupations.  Wall time, synchronised; the first run of each route allocates its scratch and is not counted.
  open     eval_points(...): per-pixel search of the hand-over records, ground-state stage (twice at K = 32, 16, 8: the
           occupations come from the sorted records)
  closed   eval_points(..., n_charge=N): centre and sector search, ground-state stage once
solver_stats() counts on QD_FLAG_VALIDATE handles only, which evaluate no points; what it would say of the closed lists is
recounted here on the host from the kept states of a sample of points: the hop components (adjacent-dot hops between kept
states) of two or more states, by size ("tasks_by_size": 2..8 states, then 9..32) and the largest.
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


def components(states, nvalid):
    """sizes of the hop components of one kept list: states (K, N) ints, the first nvalid valid"""
    st = states[:nvalid]
    d = st[:, None, :] - st[None, :, :]
    hop = np.zeros((nvalid, nvalid), bool)
    for i in range(st.shape[1] - 1):
        e = np.zeros(st.shape[1], int); e[i], e[i + 1] = -1, 1
        hop |= (d == e).all(axis=2) | (d == -e).all(axis=2)
    seen, sizes = np.zeros(nvalid, bool), []
    for s in range(nvalid):
        if seen[s]:
            continue
        todo, n = [s], 0
        seen[s] = True
        while todo:
            a = todo.pop(); n += 1
            for b in np.nonzero(hop[a] & ~seen)[0]:
                seen[b] = True; todo.append(int(b))
        sizes.append(n)
    return sizes


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

    def timed(fn):
        times = []
        for _ in range(args.repeats + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
        return times[1:]

    out = {"n_dots": N, "num_charge_states": K, "resolution": R, "envs": B, "points": B * CP, "n_charge": N}
    t = timed(lambda: env.eval_points(ids, vg_d, vb_d))
    out["open_s"] = [round(x, 4) for x in t]
    out["open_points_per_s"] = round(B * CP / min(t))
    t = timed(lambda: env.eval_points(ids, vg_d, vb_d, n_charge=N))
    out["closed_s"] = [round(x, 4) for x in t]
    out["closed_points_per_s"] = round(B * CP / min(t))
    out["closed_over_open"] = round(out["closed_points_per_s"] / out["open_points_per_s"], 3)
    # the hop components of the closed lists of a sample of points
    m = min(args.sample, CP)
    kept = env.eval_points([0], vg_d[:1, :m], vb_d[:1, :m], n_charge=N, outputs=("occupations",), states=True)["states"][0].cpu().numpy()
    by_size, largest, tasks = [0] * 8, 0, 0
    for p in range(m):
        nv = int((kept[p].sum(axis=1) == N).sum())                # (zeros behind the candidates found; n_charge = N > 0)
        for s in components(kept[p], nv):
            largest = max(largest, s)
            if s >= 2:
                by_size[min(s, 9) - 2] += 1; tasks += 1
    out.update(sample_points=m, tasks=tasks, tasks_by_size=by_size, largest_component=largest)
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dots", default="4,8")
    ap.add_argument("--states", default="32,8")
    ap.add_argument("--resolution", type=int, default=32)
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sample", type=int, default=512)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        N, K = (int(v) for v in args.child.split(","))
        print(json.dumps(run(N, K, args)), flush=True)
        return
    common = ["--resolution", str(args.resolution), "--envs", str(args.envs), "--repeats", str(args.repeats), "--sample", str(args.sample)]
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
