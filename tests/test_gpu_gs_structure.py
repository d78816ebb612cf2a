"""The ground-state structure kernel's hop test on the MI355X (run with -m gpu): channels rendered in validate mode and in
product mode against the oracle, at the smallest shapes that reach every path of the exchange rounds
(csrc/qd_groundstate.h, qd_gs_hop_rounds: constant rotations of the half-wave, verdicts collected in the rotated frame).

Rules, per pixel, as everywhere in the suite: validate mode by `_check_channel` of test_gpu_parity (32 states, plain-C
oracle) or of test_gpu_num_charge_states (K < 32: the C oracle keeps 32 states, so the reference is the Python oracle's
k = K scan, with the same bars) -- kept states bit-exact, eigenvalue within 1e-12 ||H||, occupations and signal within 1e-6
except where the oracle's relative gap is below helpers.GAP_MIN; product mode by the rule of
test_config2_shape_in_product_mode_against_oracle -- raw signal within 1e-6 relative with the same exception.

Scenes: two envs per case, helpers.place "near" (env 0) and "mid" (env 1) on the devices of seed 4286.  Share of pixels
the rule excludes (oracle alone, relative gap <= GAP_MIN), counted on the CPU over all channels of both envs:
8 dots 0 of 896, 5 dots 0 of 72, 4 dots K = 5 0 of 384, 3 dots K = 2 0 of 36, 2 dots 0 of 128: every pixel is compared."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

SEED = 4286
# (dots, resolution, K):
#   8 dots, 32 states: partner distances 1..16 all occur, the round-16 pair is tested from both sides
#   5 dots, 3 x 3: nine pixels -- the last half-wave runs a clamped duplicate beside a live pixel
#   4 dots, K = 5: the lanes at and beyond K take no part
#   3 dots, K = 2; 2 dots: one pair, 16 candidates (the rest is |0..0> padding: equal codes)
CASES = [(8, 8, 32), (5, 3, 32), (4, 8, 5), (3, 3, 2), (2, 8, 32)]


def scene(N):
    """(parameter blocks, state blocks) of the case's two envs, built on the host alone"""
    eb = H.sample_blocks(N, [SEED + e for e in range(2)])
    rng = np.random.default_rng(SEED + 100 * N)
    st = np.stack([H.place(N, eb.state[e], ("near", "mid")[e], rng) for e in range(2)])
    return eb.params, st


def _env(N, R, K, validate):
    import torch
    from qadapt_hip.vec_env import VecQuantumDeviceEnv, SyntheticCapacitanceModel
    assert torch.cuda.is_available()
    return VecQuantumDeviceEnv(2, num_dots=N, resolution=R, seed=SEED, validate=validate, num_charge_states=K,
                               capacitance_model=SyntheticCapacitanceModel(7))


@pytest.mark.parametrize("N,R,K", CASES)
def test_structure_kernel_against_oracle_in_both_modes(N, R, K):
    import test_gpu_parity as P
    import test_gpu_num_charge_states as NK
    params, st = scene(N)
    # validate mode
    env = _env(N, R, K, True)
    env.reset()
    assert np.array_equal(env._params_host, params)          # the env drew the devices the scene was built for
    env.set_state(st, np.zeros(2, np.int32))
    env.observe()
    raw, _ = env.raw(); occ = env.occupations(); cand = env.candidates(); eig = env.eigen()
    env.close()
    z_ref = np.zeros((2, N - 1, R * R)); ok = np.zeros((2, N - 1, R * R), bool)
    for e in range(2):
        dev = H.dev_view(N, params[e]); sv = H.state_view(N, st[e])
        for ch in range(N - 1):
            tag = (N, R, K, e, ch)
            if K == 32:
                z_ref[e, ch], ok[e, ch], _, _ = P._check_channel(tag, dev, sv, ch, R, cand[e, ch], occ[e, ch], raw[e, ch], eig[e, ch])
            else:
                z_ref[e, ch], ok[e, ch] = NK._check_channel(tag, dev, sv, ch, R, K, cand[e, ch], occ[e, ch], raw[e, ch], eig[e, ch])
    print(f"[gs structure] N={N} R={R} K={K}: {int((~ok).sum())} of {ok.size} pixels excluded (relative gap <= {H.GAP_MIN})")
    # product mode (no validate flag: unsorted records, the benched kernels), same scene, same reference
    env = _env(N, R, K, False)
    env.reset()
    assert np.array_equal(env._params_host, params)
    env.set_state(st, np.zeros(2, np.int32))
    env.observe()
    praw, _ = env.raw()
    env.close()
    d = np.abs(praw - z_ref) / np.maximum(np.abs(z_ref), 1e-3)
    print(f"[gs structure] product mode: max relative signal error over compared pixels {d[ok].max() if ok.any() else 0.0:.2e}")
    assert np.all(d[ok] <= 1e-6), (N, R, K, float(d[ok].max()))
