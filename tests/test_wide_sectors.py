"""The full charge-state space with total-charge sectors of 33..64 states (M <= 512): the option check, the qd_config
encoding, the restatement's sector decomposition at 256 / 243 states, and the resolvability of the scenes that
tests/test_gpu_wide_sectors.py compares pixel by pixel.  No GPU needed."""
import numpy as np
import pytest

import helpers as H
from qadapt_hip import device_model as DM
from test_full_charge_space import _qconfig, full_states, full_hamiltonian, full_ground, pixel_inputs, _scene
import wide_scenes as WS


@pytest.mark.parametrize("N,m,M,sec", [(4, 3, 256, 44), (5, 2, 243, 51), (7, 1, 128, 35), (3, 5, 216, 27), (3, 7, 512, 48),
                                       (2, 15, 256, 16)])
def test_wide_shapes_are_accepted(N, m, M, sec):
    assert DM.full_space_sizes(N, m) == (M, sec)
    assert DM.check_solver_options(_qconfig(None, m=m), n_dot=N) is None


@pytest.mark.parametrize("N,m,M,sec", [(4, 4, 625, 85), (8, 1, 256, 70), (6, 2, 729, 141), (2, 16, 289, 17)])
def test_shapes_beyond_one_wave_are_refused_with_the_sizes(N, m, M, sec):
    with pytest.raises(NotImplementedError, match=rf"M = {M} states, largest sector {sec}\b"):
        DM.check_solver_options(_qconfig(None, m=m), n_dot=N)


@pytest.mark.parametrize("N,m", [(4, 3), (5, 2), (7, 1), (3, 7), (2, 15)])
def test_qd_config_encodes_minus_m_for_the_wide_shapes(N, m):
    from qadapt_hip.vec_env import make_qd_config
    e = DM.load_yaml(None, "env_config.yaml")
    cfg = make_qd_config(e, _qconfig(None, m=m), N, 16, 2)
    assert cfg.num_charge_states == -m


def test_mixed_batch_accepts_three_carriers():
    """The shared check lets a mixed batch with a 4-dot bucket through once the YAML says 3 carriers (construction
    itself needs the GPU: only the check is exercised here)."""
    q = _qconfig(None, m=3)
    for n in (2, 4):
        assert DM.check_solver_options(q, n_dot=n) is None


@pytest.mark.parametrize("N,m", [(4, 3), (5, 2)])
def test_per_sector_solve_equals_the_dense_solve_at_wide_sizes(N, m):
    """Hopping conserves the total charge: the lowest sector's ground vector is the dense ground vector, also where
    sectors hold 44 / 51 of the 256 / 243 states."""
    states = full_states(N, m)
    Q = states.sum(axis=1)
    assert np.bincount(Q).max() > 32
    for mode, seed in (("near", 5), ("far", 7)):
        dev, sv = _scene(N, seed, mode)
        F, tc, _, _ = pixel_inputs(dev, sv, 0, 4, states)
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
        assert ok.any() and np.abs(n_sec - n_dense)[ok].max() <= 1e-8


@pytest.mark.parametrize("N,m", sorted(WS.CASES))
def test_gpu_scenes_are_resolvable(N, m):
    """A condition on the scenes of tests/test_gpu_wide_sectors.py, from the restatement alone: its per-pixel rule
    exempts pixels whose two lowest levels are closer than GAP_MIN, so at least half the pixels of every `near` env and
    some pixel of every env must not be exempt."""
    states = full_states(N, m)
    params, st = WS.scene(N, m)
    for e, mode in enumerate(WS.CASES[(N, m)]):
        dev = H.dev_view(N, params[e]); sv = H.state_view(N, st[e])
        ok = []
        for ch in range(N - 1):
            F, tc, _, _ = pixel_inputs(dev, sv, ch, WS.R, states, vc=dev.vc)
            Hm = full_hamiltonian(F, tc, states)
            w = np.linalg.eigvalsh(Hm)
            hn = np.abs(Hm).sum(axis=2).max(axis=1)
            ok.append((w[:, 1] - w[:, 0]) / hn > H.GAP_MIN)
        share = float(np.mean(ok))
        print(f"({N},{m}) env {e} {mode}: {share:.3f} of the pixels have rel_gap > GAP_MIN")
        assert share > 0.0, (N, m, e, mode)
        if mode == "near":
            assert share >= 0.5, (N, m, e, mode, share)
