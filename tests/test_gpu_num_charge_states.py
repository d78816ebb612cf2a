"""num_charge_states = K < 32 on the MI355X (run with -m gpu): the kept states, the K x K ground state and the images
against the oracle's k = K scan, in validate mode; K = 32 spelled out is the default; a noisy K = 16 env steps."""
import numpy as np
import pytest

import qd_oracle as O
import qd_oracle_c as OC
import helpers as H

pytestmark = pytest.mark.gpu

RESID_MAX = 1e-13


def _env(B, N, R, K, **kw):
    import torch
    from qadapt_hip.vec_env import VecQuantumDeviceEnv, SyntheticCapacitanceModel
    assert torch.cuda.is_available()
    kw.setdefault("capacitance_model", SyntheticCapacitanceModel(7))
    kw.setdefault("seed", 4321)
    return VecQuantumDeviceEnv(B, num_dots=N, resolution=R, num_charge_states=K, **kw)


def _random_action_state(N, par, st, rng):
    """The voltages a uniformly random action puts an env at (env.py:260-270): anywhere in its action ranges."""
    from qadapt_hip.layout import layout
    L = layout(N); st = st.copy()
    st[L.s_gate_v:L.s_gate_v + N] = par[L.pmin:L.pmin + N] + (par[L.pmax:L.pmax + N] - par[L.pmin:L.pmin + N]) * rng.random(N)
    nb = N - 1
    st[L.s_barrier_v:L.s_barrier_v + nb] = par[L.bmin:L.bmin + nb] + (par[L.bmax:L.bmax + nb] - par[L.bmin:L.bmin + nb]) * rng.random(nb)
    return st


def _ref_states(dev, v_ext, N, K, R, sv, ch):
    """The oracle's k = K kept states.  Up to 6 dots straight from candidate_states(k=K); for 8 dots (4^8 candidates per
    pixel) the plain-C 4^N scan's 32-list truncated to K -- the truncation argument test_num_charge_states pins -- and
    candidate_states(k=K) itself on every 16th pixel."""
    if N <= 6:
        return O.candidate_states(v_ext, dev.cdd_inv_full, dev.cgd_full, N, k=K)[0]
    ref = OC.csd_channel(dev, sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, sv.barrier_v, dev.window, ch, R)["states"][:, :K]
    sub = np.arange(0, R * R, 16)
    direct = O.candidate_states(v_ext[sub], dev.cdd_inv_full, dev.cgd_full, N, k=K)[0]
    assert np.array_equal(ref[sub], direct)
    return ref


def _check_channel(tag, dev, sv, ch, R, K, cand, occ, raw, eig):
    """One channel against the oracle's K-state pipeline; returns (oracle raw signal, resolvable mask)."""
    N = dev.n_dot
    vg = O.sweep_voltages(sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, ch, -dev.window, dev.window, R)
    vb = np.broadcast_to(np.asarray(sv.barrier_v, float), (R * R, N - 1))
    v_ext = np.concatenate([vg, vb], axis=1)
    ref = _ref_states(dev, v_ext, N, K, R, sv, ch)
    assert np.array_equal(cand[:, :K], ref), tag                       # kept states bit for bit
    assert np.all(cand[:, K:] == -1), tag                              # slots K..31: nothing
    F = O.free_energy_states(v_ext, dev.cdd_inv_full, dev.cgd_full, ref, N)
    if K >= 2:
        sp = H.pixel_spectrum(dev, sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, sv.barrier_v, dev.window, ch, R, states=ref)
    else:                                                              # H = [F]: no gap to resolve
        sp = dict(lam0=F[:, 0], hnorm=np.abs(F[:, 0]), rel_gap=np.full(R * R, np.inf))
    assert eig[:, 1].max() <= RESID_MAX, (tag, eig[:, 1].max())
    assert np.all(np.abs(eig[:, 0] - sp["lam0"]) <= 1e-12 * sp["hnorm"]), tag
    # the oracle's occupations of the K x K ground state and its sensor signal
    tc = O.tunnel_couplings(O.effective_barrier_potential(vg, vb, dev.Cbg, dev.Cbb), dev.tc_base, dev.alpha)
    Hm = F[:, :, None] * np.eye(K) + O.tunnel_hamiltonian(tc, ref)
    _, vecs = np.linalg.eigh(Hm)
    n_ref = np.einsum("pm,pmd->pd", vecs[:, :, 0] ** 2, ref.astype(np.float64))
    z_ref = O.charge_sensor_open(dev, vg, vb, n_open=n_ref)[0].reshape(-1)
    ok = sp["rel_gap"] > H.GAP_MIN
    d_occ = np.abs(occ - n_ref).max(axis=1)
    d_sig = np.abs(raw - z_ref) / np.maximum(np.abs(z_ref), 1e-3)
    assert np.all(sp["rel_gap"][d_occ > 1e-6] <= H.GAP_MIN), (tag, d_occ[ok].max())
    assert np.all(sp["rel_gap"][d_sig > 1e-6] <= H.GAP_MIN), (tag, d_sig[ok].max())
    return z_ref, ok


def _run_case(N, R, K, B, channels=None, pixel_search=False, seed=4321):
    env = _env(B, N, R, K, validate=True, pixel_search=pixel_search, seed=seed)
    env.reset()
    st, steps = env.get_state()
    rng = np.random.default_rng(100 * N + K)
    for e in range(B):
        if N == 8 and e == B - 1:
            st[e] = _random_action_state(N, env._params_host[e], st[e], rng)
        else:
            st[e] = H.place(N, st[e], ("near", "mid", "far")[e % 3], rng)
    env.set_state(st, steps)
    env.observe()
    raw, _ = env.raw(); occ = env.occupations(); cand = env.candidates(); eig = env.eigen()
    img = env.global_image.cpu().numpy()
    for e in range(B):
        dev = H.dev_view(N, env._params_host[e]); sv = H.state_view(N, st[e])
        chs = range(N - 1) if channels is None else channels
        ref_raw = np.zeros((N - 1, R * R)); comparable = np.zeros(N - 1, bool)
        for ch in chs:
            z, ok = _check_channel((N, R, K, e, ch), dev, sv, ch, R, K, cand[e, ch], occ[e, ch], raw[e, ch], eig[e, ch])
            ref_raw[ch] = z; comparable[ch] = ok.all()
        # the image is the reference's normalisation of the raw signal, and of the oracle's where every pixel resolves
        assert np.array_equal(img[e], O.normalise_image(raw[e].reshape(N - 1, R, R).transpose(1, 2, 0)))
        if channels is None and comparable.all():
            full = O.normalise_image(ref_raw.reshape(N - 1, R, R).transpose(1, 2, 0))
            assert np.abs(full - img[e]).max() <= 2e-6, np.abs(full - img[e]).max()
    env.close()


@pytest.mark.parametrize("K", [1, 8, 16, 24])
def test_two_dots_per_pixel_search(K):
    """Two dots: per-pixel search; K = 24 exceeds the 4^2 candidates, so every pixel pads with |0..0>."""
    _run_case(2, 32, K, B=3)


@pytest.mark.parametrize("K", [8, 16, 20])
def test_four_dots_tile_search(K):
    """Four dots, 32 x 32: the tile search with kept sets of KC = 8, 16 and 32 (K = 20 takes the first 20 of 32)."""
    _run_case(4, 32, K, B=3)


@pytest.mark.parametrize("K", [8, 16])
def test_eight_dots_tile_search(K):
    """Eight dots: two channels per env (the oracle's 4^8 scan bounds the CPU time), one env at a random action."""
    _run_case(8, 32, K, B=2, channels=(1, 5))


def test_four_dots_pixel_search_flag():
    _run_case(4, 32, 16, B=2, pixel_search=True)


def test_explicit_32_is_the_default():
    """K = 32 spelled out runs the same kernels as a handle built from the default config: raw images bit-identical."""
    out = []
    for K in (None, 32):
        env = _env(3, 6, 32, K)
        env.reset()
        st, steps = env.get_state()
        rng = np.random.default_rng(3)
        for e in range(3):
            st[e] = H.place(6, st[e], ("near", "mid", "far")[e], rng)
        env.set_state(st, steps); env.observe()
        out.append(env.raw()[0])
        assert env.num_charge_states == 32
        env.close()
    assert np.array_equal(out[0], out[1])


def test_noisy_k16_env_steps_through_an_auto_reset():
    import torch
    from qadapt_hip.vec_env import SyntheticCapacitanceModel
    N, R, B = 8, 32, 4
    env = _env(B, N, R, 16, noise=True, capacitance_model=SyntheticCapacitanceModel(11), seed=77)
    assert env.update_method == "kalman"
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
        v = obs["obs_gate_voltages"].cpu().numpy()
        assert np.isfinite(v).all() and np.abs(v).max() <= 1.0 + 1e-6
        r = rew.cpu().numpy()
        assert np.isfinite(r).all() and r.min() >= 0.0 and r.max() <= 1.0
        assert bool(trunc[1].item()) == (k == 1)
        for name in ("plunger_images", "barrier_images"):
            t = obs[name].cpu().numpy()
            assert np.isfinite(t).all() and t.min() >= 0.0 and t.max() <= 1.0
    after = env.device_state()["gate_ground_truth"]
    assert not np.array_equal(before[1], after[1])        # env 1 is a new device
    raw, _ = env.raw()
    assert np.isfinite(raw).all()
    env.close()
