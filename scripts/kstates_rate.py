"""Rate of the bench workload for several kept-state counts K (latched_model.num_charge_states).

    python scripts/kstates_rate.py [--ks 8,16,32] [--steps 10] [--warmup 3] [--envs 4096] [--dots 8] [--resolution 64]

The workload is bench.py's headline one: 8 dots, 4096 envs, 64x64, deterministic physics, synthetic capacitance model,
50-step episodes with staggered phases (1/50 of the batch auto-resets inside every step).  Every K runs in a child process
of its own (a handle created after others in the same process measured slower: K = 32 12 400 env-steps/s as the first
handle, 10 800 as the fourth): warm-up steps, then the driver-timed env-steps/s over the timed steps, then time_kernels()
(each hot kernel group by itself on one launch chunk, on the state the timed steps left).  One JSON line per K on stdout."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-agent-for-qubit-array-tuning_amd"))


def run(K, args):
    import torch
    from qadapt_hip.vec_env import VecQuantumDeviceEnv, SyntheticCapacitanceModel
    N, R, B = args.dots, args.resolution, args.envs
    env = VecQuantumDeviceEnv(B, num_dots=N, resolution=R, seed=1234, capacitance_model=SyntheticCapacitanceModel(99),
                              num_charge_states=K)
    gen = torch.Generator(device="cpu").manual_seed(99)
    env.reset()
    env.stagger_episodes()

    def step():
        env.step((torch.rand((B, 2 * N - 1), generator=gen) * 2 - 1).cuda(), auto_reset=True)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    kms = env.time_kernels(iters=2)
    out = {"num_charge_states": K, "env_steps_per_s": round(B * args.steps / dt, 1),
           "ms_per_step": round(dt / args.steps * 1e3, 3), "chunk_envs": env.chunk_envs(),
           "kernel_ms_per_chunk": {k: round(v, 4) for k, v in kms.items()},
           "workload": f"{N}-dot {R}x{R}, {B} envs, deterministic, staggered 50-step episodes, "
                       f"{args.warmup} warm-up + {args.steps} timed steps"}
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="8,16,32")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--dots", type=int, default=8)
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        print(json.dumps(run(args.child, args)), flush=True)
        return
    common = ["--steps", str(args.steps), "--warmup", str(args.warmup), "--envs", str(args.envs), "--dots", str(args.dots),
              "--resolution", str(args.resolution)]
    for K in (int(k) for k in args.ks.split(",")):
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", str(K)] + common)


if __name__ == "__main__":
    main()
