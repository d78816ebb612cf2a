"""Rate of the full charge-state space (latched_model.num_charge_states: null) against K = 32 on 2- and 3-dot arrays.

    python scripts/full_space_rate.py [--dots 2,3] [--modes 32,all] [--carriers M] [--steps 10] [--warmup 3] [--envs 4096]
                                      [--resolution 64]

Per (dots, mode): bench-style workload (R x R, deterministic physics, synthetic capacitance model, uniformly random actions,
50-step episodes with staggered phases, auto-reset inside the step), each in a child process of its own (as
scripts/kstates_rate.py: a handle created after others in the same process can measure slower): warm-up steps, then the
driver-timed env-steps/s over the timed steps, then time_kernels() (each hot kernel group by itself on one launch chunk;
the full space runs no tile search and no redo pass, reported as 0; the wave-per-block solve of 33..64-state sectors is part
of the qd_k_gs_solve group).  "all" uses the YAML's max_charge_carriers (4) unless --carriers gives another count, e.g.
--dots 4 --carriers 3, --dots 5 --carriers 2, --dots 7 --carriers 1.  One JSON line per run on stdout."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-agent-for-qubit-array-tuning_amd"))


def run(N, mode, args):
    import torch
    from qadapt_hip.vec_env import VecQuantumDeviceEnv, SyntheticCapacitanceModel
    R, B = args.resolution, args.envs
    K = "all" if mode == "all" else int(mode)
    qpath = None
    if args.carriers is not None:
        import yaml
        from qadapt_hip import device_model as DM
        q = DM.load_yaml(None, "qarray_config.yaml")
        q["simulator"]["model"]["max_charge_carriers"] = args.carriers
        fh = tempfile.NamedTemporaryFile("w", suffix=".yaml", delete=False)
        yaml.safe_dump(q, fh); fh.close()
        qpath = fh.name
    env = VecQuantumDeviceEnv(B, num_dots=N, resolution=R, seed=1234, capacitance_model=SyntheticCapacitanceModel(99),
                              num_charge_states=K, qarray_config_path=qpath)
    if qpath:
        os.unlink(qpath)
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
    out = {"n_dots": N, "num_charge_states": "null (all)" if env.num_charge_states is None else env.num_charge_states,
           "max_charge_carriers": env.max_charge_carriers,
           "env_steps_per_s": round(B * args.steps / dt, 1), "ms_per_step": round(dt / args.steps * 1e3, 3),
           "chunk_envs": env.chunk_envs(), "kernel_ms_per_chunk": {k: round(v, 4) for k, v in kms.items()},
           "workload": f"{N}-dot {R}x{R}, {B} envs, deterministic, random actions, staggered 50-step episodes, "
                       f"{args.warmup} warm-up + {args.steps} timed steps"}
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dots", default="2,3")
    ap.add_argument("--modes", default="32,all")
    ap.add_argument("--carriers", type=int, default=None, help="max_charge_carriers of the full space (default: the YAML's)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        N, mode = args.child.split(":")
        print(json.dumps(run(int(N), mode, args)), flush=True)
        return
    common = ["--steps", str(args.steps), "--warmup", str(args.warmup), "--envs", str(args.envs),
              "--resolution", str(args.resolution)]
    if args.carriers is not None:
        common += ["--carriers", str(args.carriers)]
    for N in args.dots.split(","):
        for mode in args.modes.split(","):
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", f"{N}:{mode}"] + common)


if __name__ == "__main__":
    main()
