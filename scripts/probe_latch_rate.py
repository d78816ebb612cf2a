"""HIP-event time of a one-query probe with all three stochastic stages (8 dots, 64x64 by default): what
`env.array._get_obs(noise=True)` and a GUI issue.  Run once with the product library (row-parallel latching,
qd_k_latch_rows) and once with a library built with -DQD_PROBE_SERIAL_LATCH (the one-thread walk qd_k_latch on the probe
buffers), selected through QDSIM_LIB, each in a process of its own:

    python scripts/probe_latch_rate.py
    QDSIM_LIB=/path/to/libqdsim_serial_latch.so python scripts/probe_latch_rate.py

Prints one JSON line.  Both builds render the same bits (`raw_crc`)."""
import argparse
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rl-agent-for-qubit-array-tuning_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dots", type=int, default=8)
    ap.add_argument("--resolution", type=int, default=64)
    ap.add_argument("--queries", type=int, default=1)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    from qadapt_hip import _lib
    from qadapt_hip.vec_env import VecQuantumDeviceEnv, SyntheticCapacitanceModel
    assert torch.cuda.is_available(), "needs the MI355X"
    N = a.dots
    env = VecQuantumDeviceEnv(max(a.queries, 1), num_dots=N, resolution=a.resolution, seed=11,
                              capacitance_model=SyntheticCapacitanceModel(3))
    env.reset()
    st, _ = env.get_state()
    L = env.L
    ids = np.arange(a.queries) % env.B
    gv = torch.as_tensor(st[ids, L.s_gate_gt:L.s_gate_gt + N] + 1.5).cuda()
    bv = torch.as_tensor(st[ids, L.s_barrier_gt:L.s_barrier_gt + N - 1]).cuda()
    idt = torch.as_tensor(ids, dtype=torch.int32).cuda()
    stages = ("sensor", "radial", "latch")
    res = {"dots": N, "resolution": a.resolution, "queries": a.queries, "iters": a.iters, "lib": os.path.basename(_lib.LIB_PATH)}
    for name, noise in (("clean", None), ("sensor_radial", stages[:2]), ("all_stages", stages)):
        kw = {} if noise is None else dict(noise=noise, serial=(1 << 63) | 5)
        for _ in range(a.warmup):
            out = env.probe(idt, gv, bv, **kw)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.iters):
            out = env.probe(idt, gv, bv, **kw)
        t1.record()
        torch.cuda.synchronize()
        res[name + "_ms"] = round(t0.elapsed_time(t1) / a.iters, 4)
        if noise == stages:
            res["raw_crc"] = zlib.crc32(out["raw"].cpu().numpy().tobytes())
    env.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
