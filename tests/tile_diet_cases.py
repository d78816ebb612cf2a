"""Scenes shared by tests/test_gpu_tile_diet.py and tests/golden/make_golden_tile_digests.py: the smallest shapes that reach
the tile search (N >= 4, R >= 32), one per kept-set template (K = 8, 16, 32), with image edges that cut tiles."""
import hashlib

import numpy as np

import helpers as H

B = 2
# (N, R, K, mode): smallest shape; a 4-wide edge tile; one-pixel-wide tiles; the K = 16 template
CASES = [(4, 32, 32, "start"), (8, 36, 32, "mid"), (5, 33, 8, "near"), (6, 40, 16, "mid")]
STAT_KEYS = ("tiles", "tiles_redone", "pixels_redone")


def case_key(N, R, K, mode):
    return f"N{N}_R{R}_K{K}_{mode}"


def make_env(N, R, K, **kw):
    from qadapt_hip.vec_env import VecQuantumDeviceEnv, SyntheticCapacitanceModel
    env = VecQuantumDeviceEnv(B, num_dots=N, resolution=R, seed=6100 + N, num_charge_states=K,
                              capacitance_model=SyntheticCapacitanceModel(7), **kw)
    env.reset()
    return env


def placed_state(env, N, R, mode):
    """the state every handle of the case is set to: the reset state moved by helpers.place"""
    st, steps = env.get_state()
    rng = np.random.default_rng(53 * N + R)
    if mode != "start":
        for e in range(B):
            st[e] = H.place(N, st[e], mode, rng)
    return st, steps


def observe(env, st, steps):
    env.set_state(st, steps)
    env.observe()


def raw_digests(env):
    """sha256 of the raw signal per (env, channel)"""
    raw = np.ascontiguousarray(env.raw()[0])
    return [[hashlib.sha256(raw[e, c].tobytes()).hexdigest() for c in range(raw.shape[1])] for e in range(raw.shape[0])]
