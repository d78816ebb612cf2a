"""The pruning bound of the ground-state structure kernel on the MI355X (run with -m gpu): a handle with
QD_FLAG_GS_GERSHGORIN_ZERO (hop components pruned against the bound 0 alone, as before) against one without (the pair bound
of csrc/qd_groundstate.h, qd_gs_pair_bound), same build, same scene.  The results must agree BIT FOR BIT -- the pair bound only
drops components that cannot win the selection -- while the solved tasks (solver_stats) fall.

Scenes (prune_scenes.py): two envs on the devices of seed 4286, env 0 placed "mid", env 1 "wild"; 8 x 8 pixels.  Cases:
8 dots; 4 dots with K = 5 kept states (lanes beyond K); 2 dots (|0..0> padding); 8 dots with tc_base = 0 (the classical limit:
nothing couples, no task either way)."""
import ctypes

import numpy as np
import pytest

import prune_scenes as S

pytestmark = pytest.mark.gpu

R = 8
MODES = ("mid", "wild")
# (name, dots, K, tc_base)
CASES = [("8 dots", 8, 32, None), ("4 dots K=5", 4, 5, None), ("2 dots", 2, 32, None), ("8 dots tc_base=0", 8, 32, 0.0)]


def _env(N, K, validate, zero):
    import torch
    from qadapt_hip.vec_env import VecQuantumDeviceEnv, SyntheticCapacitanceModel
    assert torch.cuda.is_available()
    return VecQuantumDeviceEnv(len(MODES), num_dots=N, resolution=R, seed=S.SEED, validate=validate, num_charge_states=K,
                               capacitance_model=SyntheticCapacitanceModel(7), gs_gershgorin_zero=zero)


def _load(env, params, state):
    """these parameter and state blocks as the handle's devices"""
    from qadapt_hip import _lib
    ids = np.arange(env.B, dtype=np.int32)
    rc = env._lib.qd_load_episodes(env._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), env.B,
                                   np.ascontiguousarray(params).ctypes.data, np.ascontiguousarray(state).ctypes.data, 0,
                                   env._stream())
    _lib.check(env._h, rc, "qd_load_episodes")
    env._params_host[:] = params


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _render(N, K, tc_base, validate, zero):
    params, st = S.scene(N, MODES, tc_base=tc_base)
    env = _env(N, K, validate, zero)
    env.reset()
    _load(env, params, st)
    before = env.solver_stats()["tasks"] if validate else 0      # (the counters run on from the reset's own observation)
    env.observe()
    out = {"raw": env.raw()[0]}
    if validate:
        out["occ"] = env.occupations(); out["eig"] = env.eigen(); out["tasks"] = env.solver_stats()["tasks"] - before
    env.close()
    return out


@pytest.mark.parametrize("name,N,K,tc_base", CASES, ids=[c[0] for c in CASES])
def test_flag_and_default_agree_bit_for_bit(name, N, K, tc_base):
    zero = _render(N, K, tc_base, True, True)
    pair = _render(N, K, tc_base, True, False)
    for key in ("raw", "occ", "eig"):
        assert np.array_equal(_bits(zero[key]), _bits(pair[key])), (name, key)
    assert np.isfinite(pair["raw"]).all() and np.ptp(pair["raw"]) > 0.0
    pixels = len(MODES) * (N - 1) * R * R
    print(f"[gs prune] {name}: tasks per pixel {zero['tasks'] / pixels:.2f} (bound 0) -> {pair['tasks'] / pixels:.2f} (pair bound)")
    assert pair["tasks"] <= zero["tasks"], (name, pair["tasks"], zero["tasks"])
    if name == "8 dots":
        assert pair["tasks"] < zero["tasks"], (name, pair["tasks"], zero["tasks"])
    if tc_base == 0.0:
        assert zero["tasks"] == 0 and pair["tasks"] == 0
        assert np.array_equal(pair["occ"], np.round(pair["occ"]))           # the classical limit: integer occupations
    # product mode (no validate flag: unsorted records, the benched kernels)
    pzero = _render(N, K, tc_base, False, True)
    ppair = _render(N, K, tc_base, False, False)
    assert np.array_equal(_bits(pzero["raw"]), _bits(ppair["raw"])), (name, "product raw")
    assert np.isfinite(ppair["raw"]).all() and np.ptp(ppair["raw"]) > 0.0


def test_probe_and_points_agree_bit_for_bit():
    """qd_probe, qd_probe_ex and qd_eval_points run the same structure kernel: the 8-dot scene through all three"""
    import torch
    N = 8
    params, st = S.scene(N, MODES)
    L = S.layout(N); G = N + 1
    rng = np.random.default_rng(S.SEED)
    gv = np.stack([st[e, L.s_gate_v:L.s_gate_v + N] for e in range(2)]); bv = np.stack([st[e, L.s_barrier_v:L.s_barrier_v + N - 1] for e in range(2)])
    # points: 96 per env around its voltages, physical gate voltages with the sensor at its ground truth
    m = 96
    vg = np.zeros((2, m, G)); vb = np.zeros((2, m, N - 1))
    for e in range(2):
        virt = np.concatenate([gv[e] + rng.uniform(-20, 20, (m, N)), np.full((m, 1), st[e, L.s_sensor_gt])], axis=1)
        vgm = st[e, L.s_vgm:L.s_vgm + G * G].reshape(G, G)
        vg[e] = virt @ vgm.T + params[e, L.origin:L.origin + G]
        vb[e] = bv[e] + rng.uniform(-5, 5, (m, N - 1))
    got = []
    for zero in (True, False):
        env = _env(N, 32, False, zero)
        env.reset()
        _load(env, params, st)
        sens = np.array([st[e, L.s_sensor_gt] for e in range(2)])
        plain = env.probe([0, 1], gv, bv, sensor_voltage=sens)
        ex = env.probe([0, 1], gv, bv, sensor_voltage=sens, occupations=True)
        pts = env.eval_points([0, 1], vg, vb)
        torch.cuda.synchronize()
        got.append({"probe raw": plain["raw"].cpu().numpy(), "probe_ex raw": ex["raw"].cpu().numpy(),
                    "probe_ex occupations": ex["occupations"].cpu().numpy(), "points signal": pts["signal"].cpu().numpy(),
                    "points occupations": pts["occupations"].cpu().numpy()})
        env.close()
    for key in got[0]:
        assert np.isfinite(got[1][key]).all() and np.ptp(got[1][key]) > 0.0, key
        assert np.array_equal(_bits(got[0][key]), _bits(got[1][key])), key
