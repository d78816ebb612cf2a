"""The untruncated charge-state space (latched_model.num_charge_states: null, the reference model's default): option
parsing, the qd_config encoding, and a restatement of the reference's full-space solve (ground_state.py:79-83, 149-162)
checked against known answers.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import qd_oracle as O
import helpers as H
from qadapt_hip import _lib
from qadapt_hip import device_model as DM


def _qconfig(k="absent", m=4):
    q = DM.load_yaml(None, "qarray_config.yaml")
    lm = q["simulator"]["latched_model"]
    if k == "absent":
        lm.pop("num_charge_states", None)
    else:
        lm["num_charge_states"] = k
    q["simulator"]["model"]["max_charge_carriers"] = m
    return q


# ---- the restatement of the reference --------------------------------------------------------------------------

def full_states(N, m):
    """create_full_charge_state_space (charge_states.py:5-34): all (m+1)^N states, base m+1, dot 0 most significant."""
    base = m + 1
    idx = np.arange(base ** N)
    powers = base ** np.arange(N - 1, -1, -1)
    return (idx[:, None] // powers[None, :]) % base


def full_hamiltonian(F, tc, states):
    """H = diag(F) + H_t over the fixed list, per pixel (unbatched_hamiltonian_build.py:20-80)."""
    P, M = F.shape
    st = np.broadcast_to(states, (P,) + states.shape)
    return F[:, :, None] * np.eye(M) + O.tunnel_hamiltonian(tc, st)


def full_ground(F, tc, states):
    """Dense eigh of the whole M x M matrix, column 0, n = sum_m |psi_m|^2 s_m; also the lowest eigenvalue."""
    w, v = np.linalg.eigh(full_hamiltonian(F, tc, states))
    return np.einsum("pm,md->pd", v[:, :, 0] ** 2, states.astype(np.float64)), w[:, 0]


def pixel_inputs(dev, sv, ch, R, states, vc=None):
    """F (P, M) and tc (P, N-1) of one CSD channel; vc = (alpha, beta): the linear voltage-dependent capacitance
    model, cdd_inv / (1 + alpha mean|v|) and cgd (1 + beta mean|v|) (voltage_dependent_capacitance.py:72-88)."""
    N = dev.n_dot
    vg = O.sweep_voltages(sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, ch, -dev.window, dev.window, R)
    vb = np.broadcast_to(np.asarray(sv.barrier_v, float), (R * R, N - 1))
    v_ext = np.concatenate([vg, vb], axis=1)
    st = np.broadcast_to(states, (R * R,) + states.shape)
    if vc is None:
        F = O.free_energy_states(v_ext, dev.cdd_inv_full, dev.cgd_full, st, N)
    else:
        mabs = np.abs(v_ext).mean(axis=1)
        sa, sb = 1.0 + vc[0] * mabs, 1.0 + vc[1] * mabs
        inner = states[None, :, :] - (sb[:, None] * (v_ext @ dev.cgd_full[:N, :].T))[:, None, :]
        F = np.einsum("pni,ij,pnj->pn", inner, dev.cdd_inv_full[:N, :N], inner) / sa[:, None]
    tc = O.tunnel_couplings(O.effective_barrier_potential(vg, vb, dev.Cbg, dev.Cbb), dev.tc_base, dev.alpha)
    return F, tc, vg, vb


def _scene(N, seed, mode):
    eb = H.sample_blocks(N, [seed])
    rng = np.random.default_rng(seed)
    return H.dev_view(N, eb.params[0]), H.state_view(N, H.place(N, eb.state[0], mode, rng))


# ---- option parsing ----------------------------------------------------------------------------------------------

def test_explicit_null_selects_the_full_space():
    assert DM.check_solver_options(_qconfig(None)) is None
    assert DM.check_solver_options(_qconfig(None), n_dot=3) is None
    assert DM.max_charge_carriers(_qconfig(None, m=4)) == 4


def test_missing_key_keeps_32():
    assert DM.check_solver_options(_qconfig("absent")) == 32
    assert DM.check_solver_options({}) == 32


@pytest.mark.parametrize("m", [0, -1, 2.5, "4", None, True])
def test_bad_max_charge_carriers_is_refused(m):
    with pytest.raises(ValueError, match="max_charge_carriers"):
        DM.check_solver_options(_qconfig(None, m=m))


def test_four_dots_with_four_carriers_is_refused_with_the_sizes():
    with pytest.raises(NotImplementedError, match=r"M = 625.*largest sector 85"):
        DM.check_solver_options(_qconfig(None, m=4), n_dot=4)


def test_four_dots_with_two_carriers_is_accepted():
    assert DM.check_solver_options(_qconfig(None, m=2), n_dot=4) is None


@pytest.mark.parametrize("N,m,M,sec", [(2, 4, 25, 5), (3, 4, 125, 19), (4, 4, 625, 85), (4, 2, 81, 19), (7, 1, 128, 35),
                                       (2, 10, 121, 11)])
def test_full_space_sizes(N, m, M, sec):
    assert DM.full_space_sizes(N, m) == (M, sec)
    st = full_states(N, m)
    assert len(st) == M and np.bincount(st.sum(axis=1)).max() == sec


def test_use_sparse_is_still_refused_in_the_full_space():
    q = _qconfig(None)
    q["simulator"]["latched_model"]["use_sparse"] = True
    with pytest.raises(NotImplementedError, match="use_sparse"):
        DM.check_solver_options(q, n_dot=2)


def test_mixed_batch_refuses_an_unsupported_bucket_at_construction():
    """The check runs for every bucket before any handle (or GPU) is touched."""
    from qadapt_hip.mixed import MixedVecQuantumDeviceEnv
    with pytest.raises(NotImplementedError, match="625"):
        MixedVecQuantumDeviceEnv({2: 2, 4: 2}, resolution=16, num_charge_states="all")


# ---- qd_config encoding ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,m", [(2, 4), (3, 4), (4, 2), (2, 1)])
def test_qd_config_encodes_minus_m(N, m):
    from qadapt_hip.vec_env import make_qd_config
    e = DM.load_yaml(None, "env_config.yaml")
    cfg = make_qd_config(e, _qconfig(None, m=m), N, 32, 2)
    assert cfg.num_charge_states == -m
    assert ctypes.sizeof(_lib.QdConfig) == 184 and cfg.struct_size == 184


def test_qd_config_refuses_an_unsupported_full_space():
    from qadapt_hip.vec_env import make_qd_config
    e = DM.load_yaml(None, "env_config.yaml")
    with pytest.raises(NotImplementedError, match="85"):
        make_qd_config(e, _qconfig(None, m=4), 4, 32, 2)


def test_header_documents_the_encoding():
    import os
    text = open(os.path.join(H.ROOT, "include", "qdsim.h")).read()
    assert "#define QD_ALL_CHARGE_STATES(m) (-(m))" in text


# ---- the restatement against known answers -------------------------------------------------------------------------

def test_state_list_is_the_reference_enumeration():
    st = full_states(3, 4)
    assert st[0].tolist() == [0, 0, 0] and st[1].tolist() == [0, 0, 1] and st[5].tolist() == [0, 1, 0]
    assert st[25].tolist() == [1, 0, 0] and st[-1].tolist() == [4, 4, 4]


@pytest.mark.parametrize("N", [2, 3])
def test_zero_coupling_gives_the_argmin_of_F(N):
    states = full_states(N, 4)
    for mode, seed in (("near", 3), ("far", 4)):
        dev, sv = _scene(N, seed, mode)
        F, tc, _, _ = pixel_inputs(dev, sv, 0, 8, states)
        n, lam = full_ground(F, np.zeros_like(tc), states)
        assert np.array_equal(n, states[np.argmin(F, axis=1)].astype(np.float64))
        assert np.array_equal(lam, F.min(axis=1))


def test_two_dot_single_carrier_closed_form():
    """The Q = 1 sector {|1,0>, |0,1>} alone at low energy: <n_0> = (1 - eps / sqrt(eps^2 + 4 t^2)) / 2."""
    states = full_states(2, 4)
    i10, i01 = 5, 1
    eps = np.array([-0.3, -0.01, 0.0, 0.02, 0.5])
    t = np.array([0.1, 0.05, 0.2, 0.01, 0.25])
    F = np.full((len(eps), len(states)), 50.0)
    F[:, i10], F[:, i01] = eps / 2, -eps / 2
    n, lam = full_ground(F, t[:, None], states)
    expect = 0.5 * (1.0 - eps / np.sqrt(eps ** 2 + 4 * t ** 2))
    assert np.allclose(n[:, 0], expect, rtol=0, atol=1e-12)
    assert np.allclose(n.sum(axis=1), 1.0, atol=1e-12)
    assert np.allclose(lam, -0.5 * np.sqrt(eps ** 2 + 4 * t ** 2), atol=1e-12)


@pytest.mark.parametrize("N,m", [(2, 4), (3, 4), (4, 2)])
def test_per_sector_solve_equals_the_dense_solve(N, m):
    """Hopping conserves the total charge: the lowest sector's ground vector is the dense ground vector."""
    states = full_states(N, m)
    Q = states.sum(axis=1)
    for mode, seed in (("near", 5), ("mid", 6), ("far", 7)):
        dev, sv = _scene(N, seed, mode)
        F, tc, _, _ = pixel_inputs(dev, sv, 0, 6, states)
        Hm = full_hamiltonian(F, tc, states)
        assert np.all(Hm[:, Q[:, None] != Q[None, :]] == 0.0)
        n_dense, lam_dense = full_ground(F, tc, states)
        w_all = np.linalg.eigvalsh(Hm)
        hn = np.abs(Hm).sum(axis=2).max(axis=1)
        best = np.full(len(F), np.inf); n_sec = np.zeros_like(n_dense)
        for q in np.unique(Q):
            sel = np.flatnonzero(Q == q)
            w, v = np.linalg.eigh(Hm[:, sel][:, :, sel])
            better = w[:, 0] < best
            best = np.where(better, w[:, 0], best)
            n_sec[better] = np.einsum("pm,md->pd", v[better][:, :, 0] ** 2, states[sel].astype(np.float64))
        assert np.all(np.abs(best - lam_dense) <= 1e-12 * hn)
        ok = (w_all[:, 1] - w_all[:, 0]) / hn > H.GAP_MIN
        assert np.abs(n_sec - n_dense)[ok].max() <= 1e-8


def test_full_space_differs_from_k32_at_random_actions():
    """Away from the ground truth the two modes give different integer occupations (the reason null is not 32)."""
    N, R = 2, 8
    states = full_states(N, 4)
    eb = H.sample_blocks(N, [21, 22, 23])
    rng = np.random.default_rng(0)
    from qadapt_hip.layout import layout
    L = layout(N)
    worst = 0.0
    for e in range(3):
        par, st = eb.params[e], eb.state[e].copy()
        st[L.s_gate_v:L.s_gate_v + N] = par[L.pmin:L.pmin + N] + (par[L.pmax:L.pmax + N] - par[L.pmin:L.pmin + N]) * rng.random(N)
        dev, sv = H.dev_view(N, par), H.state_view(N, st)
        F, tc, vg, vb = pixel_inputs(dev, sv, 0, R, states)
        n_full, _ = full_ground(F, tc, states)
        n_k = O.ground_state_open(dev, vg, vb)
        worst = max(worst, float(np.abs(n_full - n_k).max()))
    assert worst > 0.5, worst
