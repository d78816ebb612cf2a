"""The full charge-state space with sectors of 33..64 states on the MI355X (run with -m gpu): (4 dots, 3 carriers),
(5, 2), (7, 1), (3, 7).  Validate-mode parity by the rule of tests/test_gpu_full_charge_space.py against a dense eigh of
the whole M x M Hamiltonian, the use of the wave-per-block solver, the classical limit, a noisy env through an
automatic reset, and the independence of other handles.  The scenes are those of tests/wide_scenes.py, whose
resolvability tests/test_wide_sectors.py asserts on the CPU."""
import numpy as np
import pytest

import qd_oracle as O
import helpers as H
from qadapt_hip.layout import layout
from test_full_charge_space import full_states, pixel_inputs
from test_gpu_full_charge_space import _check_channel, _env, _place_all
import wide_scenes as WS

pytestmark = pytest.mark.gpu


def _load_scene(env, N, m, modes=None):
    """the host-built scene into the env: same devices (load_new_devices draws what sample_blocks draws), placed state"""
    params, st_host = WS.scene(N, m, modes)
    env.load_new_devices()
    assert np.array_equal(env._params_host, params)
    st, steps = env.get_state()
    pre = WS.pre_kalman(N)
    st[:, pre] = st_host[:, pre]
    env.set_state(st, steps)
    return st


@pytest.mark.parametrize("N,m", sorted(WS.CASES))
def test_validate_parity_and_wide_class_use(tmp_path, N, m):
    modes = WS.CASES[(N, m)]
    R = WS.R
    env = _env(len(modes), N, R, tmp_path, m=m, validate=True, seed=WS.seed_of(N, m))
    assert env.num_charge_states is None and env.max_charge_carriers == m
    st = _load_scene(env, N, m)
    env.observe()
    raw, _ = env.raw(); occ = env.occupations(); eig = env.eigen()
    img = env.global_image.cpu().numpy()
    stats = env.solver_stats()
    states = full_states(N, m)
    for e in range(len(modes)):
        dev = H.dev_view(N, env._params_host[e]); sv = H.state_view(N, st[e])
        for ch in range(N - 1):
            _check_channel((N, m, e, ch), dev, sv, ch, R, states, occ[e, ch], raw[e, ch], eig[e, ch])
        assert np.array_equal(img[e], O.normalise_image(raw[e].reshape(N - 1, R, R).transpose(1, 2, 0)))
    print(f"({N},{m}): worst residual {eig[..., 1].max():.2e}, solver stats {stats}")
    # sectors above 32 states went to the wave-per-block solver
    assert stats["wide_tasks"] > 0, stats
    env.close()


def test_three_dots_four_carriers_has_no_wide_task(tmp_path):
    env = _env(2, 3, 16, tmp_path, m=4, validate=True)
    env.reset()
    _place_all(env, 3, np.random.default_rng(34), ("near", "random"))
    env.observe()
    stats = env.solver_stats()
    assert stats["tasks"] > 0 and stats["wide_tasks"] == 0, stats
    env.close()


def test_zero_coupling_gives_integer_occupations(tmp_path):
    """tc_base = 0 at (4, 3): H is diagonal, the occupations are exact integers and the argmin of F over the 256 states."""
    N, m, R = 4, 3, 16
    modes = ("near", "far", "random")
    env = _env(len(modes), N, R, tmp_path, m=m, validate=True, seed=WS.seed_of(N, m))
    params, st_host = WS.scene(N, m, modes)
    env.load_new_devices()
    L = layout(N)
    par = env._params_host.copy()
    assert np.array_equal(par, params)
    par[:, L.scal] = 0.0                                              # tc_base
    ids = np.arange(len(modes), dtype=np.int32)
    import ctypes
    from qadapt_hip import _lib
    st, steps = env.get_state()
    pre = WS.pre_kalman(N)
    st[:, pre] = st_host[:, pre]
    rc = env._lib.qd_load_episodes(env._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(ids), par.ctypes.data,
                                   st.ctypes.data, 0, env._stream())
    _lib.check(env._h, rc, "qd_load_episodes")
    env.observe()
    occ = env.occupations()
    states = full_states(N, m)
    for e in range(len(modes)):
        dev = H.dev_view(N, par[e]); sv = H.state_view(N, st[e])
        assert dev.tc_base == 0.0
        for ch in range(N - 1):
            F, tc, _, _ = pixel_inputs(dev, sv, ch, R, states, vc=dev.vc)
            assert np.all(tc == 0.0)
            srt = np.sort(F, axis=1)
            clear = (srt[:, 1] - srt[:, 0]) > 1e-9 * np.abs(srt[:, 0]).clip(1.0)      # (an exact tie has no argmin)
            want = states[np.argmin(F, axis=1)].astype(np.float64)
            assert clear.any()
            assert np.array_equal(occ[e, ch], np.rint(occ[e, ch]))
            assert np.array_equal(occ[e, ch][clear], want[clear]), (e, ch)
    env.close()


def test_noisy_wide_env_steps_through_an_auto_reset(tmp_path):
    import torch
    from qadapt_hip.vec_env import SyntheticCapacitanceModel
    N, R, B = 4, 16, 4
    env = _env(B, N, R, tmp_path, m=3, noise=True, capacitance_model=SyntheticCapacitanceModel(11), seed=77)
    env.reset()
    st, steps = env.get_state()
    steps[1] = env.max_steps - 2                           # env 1 truncates on the second step and is reset in it
    env.set_state(st, steps)
    rng = np.random.default_rng(8)
    before = env.device_state()["gate_ground_truth"].copy()
    for k in range(3):
        act = torch.as_tensor(rng.uniform(-1, 1, (B, 2 * N - 1)).astype(np.float32)).cuda()
        obs, rew, term, trunc = env.step(act, auto_reset=True)
        img = obs["image"].cpu().numpy()
        assert np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 1.0
        r = rew.cpu().numpy()
        assert np.isfinite(r).all() and r.min() >= 0.0 and r.max() <= 1.0
        assert bool(trunc[1].item()) == (k == 1)
        for name in ("plunger_images", "barrier_images"):
            t = obs[name].cpu().numpy()
            assert np.isfinite(t).all() and t.min() >= 0.0 and t.max() <= 1.0
    after = env.device_state()["gate_ground_truth"]
    assert not np.array_equal(before[1], after[1])
    assert np.isfinite(env.raw()[0]).all()
    t = env.time_kernels(iters=1)
    assert t["qd_k_tile"] == 0.0 and t["qd_k_candidates"] == 0.0 and t["qd_k_gs_solve"] > 0.0
    env.close()


def test_mixed_batch_with_three_carriers_constructs_and_steps(tmp_path):
    import torch
    import yaml
    from qadapt_hip import device_model as DM
    from qadapt_hip.mixed import MixedVecQuantumDeviceEnv
    q = DM.load_yaml(None, "qarray_config.yaml")
    q["simulator"]["model"]["max_charge_carriers"] = 3
    p = tmp_path / "qarray_m3.yaml"
    p.write_text(yaml.safe_dump(q))
    from qadapt_hip.vec_env import SyntheticCapacitanceModel
    env = MixedVecQuantumDeviceEnv({2: 2, 4: 2}, resolution=16, num_charge_states="all", qarray_config_path=str(p),
                                   capacitance_model_factory=lambda n: SyntheticCapacitanceModel(3))
    obs = env.reset()
    rng = np.random.default_rng(3)
    acts = {n: torch.as_tensor(rng.uniform(-1, 1, (b, 2 * n - 1)).astype(np.float32)).cuda() for n, b in {2: 2, 4: 2}.items()}
    out = env.step(acts)
    for n in (2, 4):
        img = out[n][0]["image"].cpu().numpy()
        assert np.isfinite(img).all() and img.min() >= 0.0 and img.max() <= 1.0
    env.close()


def test_other_handles_are_unchanged_by_a_wide_handle(tmp_path):
    """A default K = 32 handle and a (3, 4) full-space handle built after a (4, 3) handle give the same raw images and
    global images as ones built before it."""
    from qadapt_hip.vec_env import VecQuantumDeviceEnv, SyntheticCapacitanceModel

    def default_out():
        env = VecQuantumDeviceEnv(3, num_dots=4, resolution=32, seed=99, capacitance_model=SyntheticCapacitanceModel(3))
        env.reset()
        _place_all(env, 4, np.random.default_rng(1), ("near", "mid", "far"))
        env.observe()
        out = (env.raw()[0], env.global_image.cpu().numpy())
        env.close()
        return out

    def full34_out():
        env = _env(3, 3, 32, tmp_path, m=4)
        env.reset()
        _place_all(env, 3, np.random.default_rng(2), ("near", "far", "random"))
        env.observe()
        out = (env.raw()[0], env.global_image.cpu().numpy())
        env.close()
        return out

    first = default_out(), full34_out()
    wide = _env(2, 4, 16, tmp_path, m=3)
    wide.reset(); wide.observe()
    second = default_out(), full34_out()
    wide.close()
    for a, b in zip(first, second):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
