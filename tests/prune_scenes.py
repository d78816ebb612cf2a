"""Scenes of the pruning tests of the ground-state stage (test_gs_prune_cpu.py, test_gpu_gs_prune.py), built on the host alone
with the product's sampler: the devices of seed 4286 + e, placed "mid" (helpers.place) or "wild" -- gates +-120 V and barriers
+-30 V around the ground truth, the regime of random actions where the tunnel couplings are large and many hop components
survive a Gershgorin test against the bound 0."""
import numpy as np

import helpers as H
from qadapt_hip.layout import layout

SEED = 4286


def place_wild(N, st, rng, vgm_noise=0.05):
    L = layout(N); G = N + 1; nb = N - 1
    st = st.copy()
    st[L.s_gate_v:L.s_gate_v + N] = st[L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-120, 120, N)
    st[L.s_barrier_v:L.s_barrier_v + nb] = st[L.s_barrier_gt:L.s_barrier_gt + nb] + rng.uniform(-30, 30, nb)
    st[L.s_vgm:L.s_vgm + G * G] += rng.normal(0, vgm_noise, G * G)
    return st


def placed(N, st, mode, rng):
    return place_wild(N, st, rng) if mode == "wild" else H.place(N, st, mode, rng)


def scene(N, modes, tc_base=None):
    """(parameter blocks, state blocks) of len(modes) envs: env e is the device of seed SEED + e placed modes[e];
    tc_base: overrides the devices' tunnel-coupling scale (0: the classical limit)"""
    eb = H.sample_blocks(N, [SEED + e for e in range(len(modes))])
    rng = np.random.default_rng(SEED + 100 * N)
    st = np.stack([placed(N, eb.state[e], modes[e], rng) for e in range(len(modes))])
    params = eb.params.copy()
    if tc_base is not None:
        params[:, layout(N).scal] = tc_base
    return params, st
