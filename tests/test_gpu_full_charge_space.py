"""The full charge-state space (num_charge_states="all", the YAML's explicit null) on the MI355X (run with -m gpu), in
validate mode: per pixel the ground energy and residual against a dense eigh of the whole M x M Hamiltonian, the
occupations and raw signal against that solve, and the image against the reference's normalisation."""
import numpy as np
import pytest
import yaml

import qd_oracle as O
import helpers as H
from qadapt_hip import device_model as DM
from test_full_charge_space import full_states, full_hamiltonian, pixel_inputs

pytestmark = pytest.mark.gpu

RESID_MAX = 1e-13


def _qpath(tmp_path, m):
    q = DM.load_yaml(None, "qarray_config.yaml")
    q["simulator"]["model"]["max_charge_carriers"] = m
    p = tmp_path / f"qarray_m{m}.yaml"
    p.write_text(yaml.safe_dump(q))
    return str(p)


def _env(B, N, R, tmp_path, m=4, K="all", **kw):
    import torch
    from qadapt_hip.vec_env import VecQuantumDeviceEnv, SyntheticCapacitanceModel
    assert torch.cuda.is_available()
    kw.setdefault("capacitance_model", SyntheticCapacitanceModel(7))
    kw.setdefault("seed", 4321)
    return VecQuantumDeviceEnv(B, num_dots=N, resolution=R, num_charge_states=K,
                               qarray_config_path=_qpath(tmp_path, m), **kw)


def _random_action_state(N, par, st, rng):
    from qadapt_hip.layout import layout
    L = layout(N); st = st.copy(); nb = N - 1
    st[L.s_gate_v:L.s_gate_v + N] = par[L.pmin:L.pmin + N] + (par[L.pmax:L.pmax + N] - par[L.pmin:L.pmin + N]) * rng.random(N)
    st[L.s_barrier_v:L.s_barrier_v + nb] = par[L.bmin:L.bmin + nb] + (par[L.bmax:L.bmax + nb] - par[L.bmin:L.bmin + nb]) * rng.random(nb)
    return st


def _place_all(env, N, rng, modes):
    st, steps = env.get_state()
    for e, mode in enumerate(modes):
        st[e] = _random_action_state(N, env._params_host[e], st[e], rng) if mode == "random" else H.place(N, st[e], mode, rng)
    env.set_state(st, steps)
    return st


def _peak_width(dev, sv, ch):
    if dev.vpw_alpha is None:
        return dev.gamma
    w = dev.gamma - abs(dev.vpw_alpha * (abs(sv.gate_v[ch]) + abs(sv.gate_v[ch + 1])) / 2.0)
    return min(max(w, 0.0), 1.0)


def _check_channel(tag, dev, sv, ch, R, states, occ, raw, eig):
    F, tc, vg, vb = pixel_inputs(dev, sv, ch, R, states, vc=dev.vc)
    Hm = full_hamiltonian(F, tc, states)
    w, v = np.linalg.eigh(Hm)
    hn = np.abs(Hm).sum(axis=2).max(axis=1)
    rel_gap = (w[:, 1] - w[:, 0]) / hn
    assert eig[:, 1].max() <= RESID_MAX, (tag, eig[:, 1].max())
    assert np.all(np.abs(eig[:, 0] - w[:, 0]) <= 1e-12 * hn), (tag, np.abs(eig[:, 0] - w[:, 0]).max())
    n_ref = np.einsum("pm,md->pd", v[:, :, 0] ** 2, states.astype(np.float64))
    z_ref = O.charge_sensor_open(dev, vg, vb, n_open=n_ref, gamma=_peak_width(dev, sv, ch))[0].reshape(-1)
    d_occ = np.abs(occ - n_ref).max(axis=1)
    d_sig = np.abs(raw - z_ref) / np.maximum(np.abs(z_ref), 1e-3)
    ok = rel_gap > H.GAP_MIN
    assert np.all(rel_gap[d_occ > 1e-6] <= H.GAP_MIN), (tag, d_occ[ok].max())
    assert np.all(rel_gap[d_sig > 1e-6] <= H.GAP_MIN), (tag, d_sig[ok].max())
    return n_ref


def _run_case(tmp_path, N, m, R=32, modes=("near", "mid", "far", "random"), **kw):
    env = _env(len(modes), N, R, tmp_path, m=m, validate=True, **kw)
    assert env.num_charge_states is None and env.max_charge_carriers == m
    env.reset()
    st = _place_all(env, N, np.random.default_rng(10 * N + m), modes)
    env.observe()
    raw, _ = env.raw(); occ = env.occupations(); eig = env.eigen()
    img = env.global_image.cpu().numpy()
    states = full_states(N, m)
    for e in range(len(modes)):
        dev = H.dev_view(N, env._params_host[e]); sv = H.state_view(N, st[e])
        for ch in range(N - 1):
            _check_channel((N, m, e, ch), dev, sv, ch, R, states, occ[e, ch], raw[e, ch], eig[e, ch])
        assert np.array_equal(img[e], O.normalise_image(raw[e].reshape(N - 1, R, R).transpose(1, 2, 0)))
    from qadapt_hip._lib import QdError
    with pytest.raises(QdError, match="candidate"):
        env.candidates()
    env.close()


def test_two_dots(tmp_path):
    _run_case(tmp_path, 2, 4)


def test_three_dots(tmp_path):
    _run_case(tmp_path, 3, 4)


def test_four_dots_two_carriers(tmp_path):
    _run_case(tmp_path, 4, 2, modes=("near", "far", "random"))


def test_linear_capacitance_and_variable_peak_width(tmp_path):
    _run_case(tmp_path, 3, 4, modes=("near", "random"), voltage_capacitance_model="linear", vary_peak_width=True)


def test_four_dots_four_carriers_is_refused(tmp_path):
    with pytest.raises(NotImplementedError, match="625"):
        _env(1, 4, 16, tmp_path, m=4)


def test_random_action_differs_from_k32(tmp_path):
    """Same devices, same voltages: the full space and K = 32 give different occupations (the library used to run
    K = 32 for an explicit null)."""
    out = []
    for K in ("all", 32):
        env = _env(2, 2, 32, tmp_path, K=K, validate=True)
        env.reset()
        _place_all(env, 2, np.random.default_rng(5), ("random", "random"))
        env.observe()
        out.append(env.occupations())
        env.close()
    assert np.abs(out[0] - out[1]).max() > 0.5


def test_noisy_full_space_env_steps_through_an_auto_reset(tmp_path):
    import torch
    from qadapt_hip.vec_env import SyntheticCapacitanceModel
    N, R, B = 3, 32, 4
    env = _env(B, N, R, tmp_path, noise=True, capacitance_model=SyntheticCapacitanceModel(11), seed=77)
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
    assert t["qd_k_tile"] == 0.0 and t["qd_k_candidates"] == 0.0 and t["qd_k_gs_structure"] > 0.0
    env.close()


def test_default_handle_after_a_full_space_handle_is_unchanged(tmp_path):
    """A default K = 32 handle built after a full-space one in the same process gives the same images as one built
    before it (no state leaks between the modes)."""
    from qadapt_hip.vec_env import VecQuantumDeviceEnv, SyntheticCapacitanceModel

    def default_raw():
        env = VecQuantumDeviceEnv(3, num_dots=4, resolution=32, seed=99, capacitance_model=SyntheticCapacitanceModel(3))
        env.reset()
        _place_all(env, 4, np.random.default_rng(1), ("near", "mid", "far"))
        env.observe()
        out = (env.raw()[0], env.global_image.cpu().numpy())
        assert env.num_charge_states == 32
        env.close()
        return out

    first = default_raw()
    full = _env(2, 3, 32, tmp_path)
    full.reset(); full.observe()
    second = default_raw()
    full.close()
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
