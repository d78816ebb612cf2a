"""The pruning bound of the ground-state structure kernel (csrc/qd_groundstate.h: qd_gs_pair_bound, qd_gs_prune_margin,
qd_gs_is_task), compiled for the CPU (tests/hosttest_prune), on oracle Hamiltonians.  No GPU needed.

Per pixel: the oracle's kept states, free energies and tunnel Hamiltonian (as helpers.pixel_spectrum builds them), the hop
components from the non-zero pattern of the tunnel Hamiltonian, numpy.linalg.eigvalsh per component.  A component of >= 2
states is kept (becomes a task) iff its Gershgorin lower bound lb = min(F - radius) <= ub + margin.  Asserted, with
||H||_inf the norm in the frame of the lowest free energy (what the margin is a multiple of):
  * every component within 2e-14 ||H||_inf of the pixel's lowest eigenvalue is kept (the bar of the eigen-solvers,
    tests/test_eig_solver_cpu.py: whatever could win the selection, or tie for it, is solved);
  * every pruned component has lb - margin above the lowest eigenvalue;
  * ub >= lambda_min - 4 eps ||H||_inf (it is an upper bound, up to its own rounding).
Isolated states do not pass through the bound (they keep the rule F <= 0) and are no subject here beyond entering lambda_min.
Each case prints the tasks per pixel under the bound 0 and under the pair bound."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import prune_scenes as S
import qd_oracle as O

EPS = np.finfo(float).eps
_LIB = None


def prune_lib():
    global _LIB
    if _LIB is None:
        hdir = os.path.join(H.ROOT, "tests", "hosttest_prune")
        subprocess.check_call(["make", "-s", "-C", hdir, "libqdsim_hosttest_prune.so"])
        _LIB = ctypes.CDLL(os.path.join(hdir, "libqdsim_hosttest_prune.so"))
        _LIB.qdhp_pixel.restype = None
        _LIB.qdhp_is_task.restype = None
    return _LIB


def pixel_bounds(F, Ht):
    """the helpers on one pixel: (F - radius per state, ub, margin, lowest free energy)"""
    K = F.size
    F = np.ascontiguousarray(F, float); Ht = np.ascontiguousarray(Ht, float)
    lower = np.empty(K); ub = ctypes.c_double(); margin = ctypes.c_double(); fs = ctypes.c_double()
    prune_lib().qdhp_pixel(K, H._p(F, ctypes.c_double), H._p(Ht, ctypes.c_double), H._p(lower, ctypes.c_double),
                           ctypes.byref(ub), ctypes.byref(margin), ctypes.byref(fs))
    return lower, ub.value, margin.value, fs.value


def is_task(comp_lower, ub, margin):
    comp_lower = np.ascontiguousarray(comp_lower, float)
    out = np.empty(comp_lower.size, np.uint8)
    prune_lib().qdhp_is_task(ctypes.c_long(comp_lower.size), H._p(comp_lower, ctypes.c_double), ctypes.c_double(ub),
                             ctypes.c_double(margin), H._p(out, ctypes.c_uint8))
    return out.astype(bool)


def components(adj):
    """lists of member indices of the connected components of a symmetric boolean adjacency matrix"""
    K = adj.shape[0]
    reach = adj | np.eye(K, dtype=bool)
    while True:
        nxt = (reach.astype(np.int64) @ reach.astype(np.int64)) > 0
        if np.array_equal(nxt, reach):
            break
        reach = nxt
    label = reach.argmax(axis=1)                           # lowest member
    return [np.flatnonzero(label == r) for r in np.unique(label)]


_SCENES = {}
_PARTS = {}


def scene(N, modes, tc_base=None):
    key = (N, tuple(modes), tc_base)
    if key not in _SCENES:
        _SCENES[key] = S.scene(N, list(modes), tc_base=tc_base)
    return _SCENES[key]


def pixel_parts(N, modes, e, ch, R, K=32, tc_base=None):
    """per pixel of one channel of env e of a scene: free energies (P, K), tunnel couplings (P, N - 1) and the oracle's K kept
    states (P, K, N); computed once per session"""
    key = (N, tuple(modes), e, ch, R, K, tc_base)
    if key not in _PARTS:
        params, st = scene(N, modes, tc_base)
        dev = H.dev_view(N, params[e]); sv = H.state_view(N, st[e])
        vg = O.sweep_voltages(sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, ch, -dev.window, dev.window, R)
        vb = np.broadcast_to(np.asarray(sv.barrier_v, float), (R * R, N - 1))
        v_ext = np.concatenate([vg, vb], axis=1)
        states, _ = O.candidate_states(v_ext, dev.cdd_inv_full, dev.cgd_full, N, k=K)
        F = O.free_energy_states(v_ext, dev.cdd_inv_full, dev.cgd_full, states, N)
        tc = O.tunnel_couplings(O.effective_barrier_potential(vg, vb, dev.Cbg, dev.Cbb), dev.tc_base, dev.alpha)
        _PARTS[key] = (F, tc, states)
    return _PARTS[key]


def hamiltonians(N, modes, e, ch, R, K=32, tc_base=None):
    F, tc, states = pixel_parts(N, modes, e, ch, R, K, tc_base)
    return F, O.tunnel_hamiltonian(tc, states)


def check_pixels(tag, F, Ht):
    """the three assertions on every pixel; returns (pixels, tasks under the bound 0, tasks under the pair bound)"""
    P = F.shape[0]
    n_old = n_new = 0
    for p in range(P):
        lower, ub, margin, fs = pixel_bounds(F[p], Ht[p])
        Fs = F[p] - fs
        Hm = np.diag(Fs) + Ht[p]
        assert np.array_equal(Hm, Hm.T), tag
        hn = np.abs(Hm).sum(axis=1).max()
        assert ub <= 0.0 and abs(margin - 2.0 ** -40 * hn) <= 64 * EPS * margin, (tag, p, ub, margin, hn)    # (order of the row sums)
        comps = components(Ht[p] != 0.0)
        lam = np.array([np.linalg.eigvalsh(Hm[np.ix_(c, c)])[0] for c in comps])
        lam_min = lam.min()
        assert ub >= lam_min - 4 * EPS * hn, (tag, p, ub, lam_min, hn)
        multi = np.array([c.size >= 2 for c in comps])
        lb = np.array([lower[c].min() for c in comps])
        kept = is_task(lb, ub, margin) & multi
        old = (lb <= 0.0) & multi
        assert not (kept & ~old).any(), (tag, p)             # the pair bound never adds a task
        near = multi & (lam <= lam_min + 2e-14 * hn)
        assert kept[near].all(), (tag, p, lam[near], lb[near], ub, margin)
        pruned = multi & ~kept
        assert (lb[pruned] - margin > lam_min).all(), (tag, p, lb[pruned], margin, lam_min)
        n_old += int(old.sum()); n_new += int(kept.sum())
    print(f"[gs prune] {tag}: {P} pixels, tasks per pixel {n_old / P:.2f} (bound 0) -> {n_new / P:.2f} (pair bound)")
    return P, n_old, n_new


R = 8
THREE = {m: (m,) * 3 for m in ("mid", "wild")}


@pytest.mark.parametrize("mode", ["mid", "wild"])
def test_eight_dot_scenes(mode):
    """three devices, channels 0, 3 and 6"""
    N = 8
    tot = np.zeros(3, np.int64)
    for e in range(3):
        for ch in (0, 3, 6):
            F, Ht = hamiltonians(N, THREE[mode], e, ch, R)
            tot += check_pixels((mode, e, ch), F, Ht)
    print(f"[gs prune] 8 dots {mode}: tasks per pixel {tot[1] / tot[0]:.2f} (bound 0) -> {tot[2] / tot[0]:.2f} (pair bound)")
    assert tot[2] <= tot[1]
    if mode == "wild":
        assert tot[2] < tot[1]


def test_classical_limit_has_no_task():
    N = 8
    for e in range(2):
        F, Ht = hamiltonians(N, ("mid", "wild"), e, 3, R, tc_base=0.0)
        assert not Ht.any()
        assert check_pixels(("tc_base=0", e), F, Ht)[1:] == (0, 0)


@pytest.mark.parametrize("mode", ["mid", "wild"])
def test_couplings_of_very_different_scales(mode):
    """the coupling of one barrier scaled to 1e44 and of another to 1e-30 (the two pairs the kept states hop over most): the
    margin follows ||H||_inf, tiny couplings still link"""
    N = 8
    F, tc, states = pixel_parts(N, THREE[mode], 0, 0, R)
    hops = [np.count_nonzero(O.tunnel_hamiltonian(np.broadcast_to(np.eye(N - 1)[d], tc.shape), states)) for d in range(N - 1)]
    big, small = np.argsort(hops)[::-1][:2]
    assert hops[small] > 0
    tc = tc.copy()
    tc[:, big] *= 1e44 / tc[:, big].max(); tc[:, small] *= 1e-30 / tc[:, small].max()
    Ht = O.tunnel_hamiltonian(tc, states)
    assert np.abs(Ht).max() >= 1e43 and np.abs(Ht)[Ht != 0.0].min() <= 1e-28
    check_pixels(("scaled", mode), F, Ht)


def test_two_dots_with_padding():
    """16 valid candidates, the rest copies of |0..0>: equal states, never linked"""
    N = 2
    for e in range(2):
        F, Ht = hamiltonians(N, ("mid", "wild"), e, 0, R)
        assert not Ht[:, 16:, :].any()
        check_pixels(("2 dots", e), F, Ht)


def test_five_of_thirty_two_states():
    N, K = 4, 5
    for e in range(2):
        for ch in range(N - 1):
            F, Ht = hamiltonians(N, ("mid", "wild"), e, ch, R, K=K)
            assert F.shape[1] == K
            check_pixels(("K=5", e, ch), F, Ht)


def test_threshold_on_a_hand_made_pixel():
    """the helpers on five states: a component at lb = ub + margin is a task, one ulp above it is not"""
    F = np.array([0.0, 1.0, 3.0, 3.5, 10.0]); Ht = np.zeros((5, 5))
    Ht[0, 1] = Ht[1, 0] = -2.0; Ht[2, 3] = Ht[3, 2] = -0.25
    lower, ub, margin, fs = pixel_bounds(F, Ht)
    assert fs == 0.0 and ub == 0.5 * (0.0 + 1.0) - 2.0 and margin == 2.0 ** -40 * 10.0
    assert np.array_equal(lower, [-2.0, -1.0, 2.75, 3.25, 10.0])
    edge = ub + margin
    assert is_task(np.array([edge, np.nextafter(edge, np.inf), -2.0, 2.75]), ub, margin).tolist() == [True, False, True, False]
