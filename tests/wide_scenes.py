"""Scenes shared by tests/test_wide_sectors.py (CPU) and tests/test_gpu_wide_sectors.py (GPU): the full charge-state
space with total-charge sectors of 33..64 states.  A scene is built on the host alone -- device blocks from
helpers.sample_blocks (what VecQuantumDeviceEnv.load_new_devices uploads for the same seed), voltages placed by
helpers.place or drawn over the action ranges -- so that the CPU tier can check, without a GPU, that the pixels the GPU
test compares one by one are resolvable."""
import numpy as np

import helpers as H
from qadapt_hip.layout import layout

SEED = 4321
# per case where the default draws a scene that tests/test_wide_sectors.py::test_gpu_scenes_are_resolvable refuses
# ((4, 3) at 4321: no pixel of the random-action env has rel_gap > GAP_MIN); chosen on the CPU, before any GPU run
SEEDS = {(4, 3): 200}
R = 16
# (dots, carriers) -> modes, one env each.  A 512-state eigh per pixel is what bounds R and the env count.
CASES = {(4, 3): ("near", "far", "random"), (5, 2): ("near", "far", "random"), (7, 1): ("near", "random"),
         (3, 7): ("near", "random")}


def random_action_state(N, par, st, rng):
    L = layout(N); st = st.copy(); nb = N - 1
    st[L.s_gate_v:L.s_gate_v + N] = par[L.pmin:L.pmin + N] + (par[L.pmax:L.pmax + N] - par[L.pmin:L.pmin + N]) * rng.random(N)
    st[L.s_barrier_v:L.s_barrier_v + nb] = par[L.bmin:L.bmin + nb] + (par[L.bmax:L.bmax + nb] - par[L.bmin:L.bmin + nb]) * rng.random(nb)
    return st


def seed_of(N, m):
    return SEEDS.get((N, m), SEED)


def scene(N, m, modes=None, seed=None):
    """(params (B, L.size), state (B, L.s_size)) of the case: env e is the device of seed + e, placed by modes[e]."""
    modes = CASES[(N, m)] if modes is None else modes
    seed = seed_of(N, m) if seed is None else seed
    eb = H.sample_blocks(N, [seed + e for e in range(len(modes))])
    rng = np.random.default_rng(10 * N + m)
    st = eb.state.copy()
    for e, mode in enumerate(modes):
        st[e] = random_action_state(N, eb.params[e], st[e], rng) if mode == "random" else H.place(N, st[e], mode, rng)
    return eb.params, st


def pre_kalman(N):
    """the part of a state block that load_new_devices uploads as sampled (everything before the Kalman block)"""
    return slice(0, layout(N).s_kmean)
