"""The per-task dense eigen-solver of the ground-state kernel (csrc/qd_eig.h), compiled for the CPU, against
numpy.linalg.eigh (what the reference calls on the whole 32x32 matrix, ground_state.py:149-162): hop-type blocks
(non-negative diagonal, non-positive couplings, connected), every block size 2..32, couplings from 1e-22 to 1e44,
near-degenerate lowest pairs.  No GPU needed."""
import ctypes

import numpy as np
import pytest

import helpers as H
import eig_cases as EC
from eig_cases import hop_block  # noqa: F401  (scripts and older callers import it from here)


def solve(A):
    h = H.hosttest()
    s = A.shape[0]
    packed = np.ascontiguousarray(A[np.tril_indices(s)], dtype=np.float64)
    lam = ctypes.c_double(); res = ctypes.c_double(); it = ctypes.c_int()
    x = np.zeros(s)
    rc = h.qdh_eig_lowest(s, H._p(packed, ctypes.c_double), ctypes.byref(lam), H._p(x, ctypes.c_double),
                          ctypes.byref(res), ctypes.byref(it))
    assert rc == 0
    return lam.value, x, res.value, it.value


@pytest.mark.parametrize("s", EC.LANE_SIZES)
def test_lowest_pair_matches_eigh_over_scales(s):
    worst = 0.0
    for tscale, A in EC.scale_family(s):
        w, V = np.linalg.eigh(A)
        hn = np.abs(A).sum(axis=1).max()
        lam, x, res, it = solve(A)
        assert abs(lam - w[0]) <= 4e-15 * hn, (s, tscale, lam, w[0])
        assert abs(np.linalg.norm(x) - 1) < 1e-14
        assert res <= 4e-15 * hn, (s, tscale, res / hn)
        gap = (w[1] - w[0]) / hn
        if gap > 1e-9:
            # eigenvector error of any backward-stable solver ~ eps / gap
            err = min(np.abs(x - V[:, 0]).max(), np.abs(x + V[:, 0]).max())
            assert err <= 2e-7 + 1e-15 / gap, (s, tscale, err, gap)
            worst = max(worst, err)
        assert it <= 64
    print(f"s={s}: worst eigenvector difference vs eigh {worst:.1e}")


@pytest.mark.parametrize("s", EC.CLASSICAL_SIZES)
def test_classical_limit_and_tiny_couplings(s):
    """couplings of exactly zero or far below the diagonal's spread: the lowest diagonal entry wins"""
    A = EC.classical_block(s)
    lam, x, res, it = solve(A)
    k = int(np.argmin(np.diag(A)))
    assert lam == pytest.approx(A[k, k], abs=1e-15) and abs(abs(x[k]) - 1) < 1e-12


@pytest.mark.parametrize("s,sep", EC.NEAR_DEGENERATE)
def test_near_degenerate_lowest_pair_at_huge_coupling(s, sep):
    """The corner round 2 got wrong (plain Lanczos, no re-orthogonalisation): two weakly linked identical halves at
    tc ~ 1e14..1e20 give a lowest pair whose relative gap is `sep`; the vector must be the symmetric/positive one."""
    for tc, A, hn in EC.near_degenerate_family(s, sep):
        w, V = np.linalg.eigh(A)
        gap = (w[1] - w[0]) / hn
        lam, x, res, it = solve(A)
        assert abs(lam - w[0]) <= 4e-15 * hn
        assert res <= 2e-14 * hn
        err = min(np.abs(x - V[:, 0]).max(), np.abs(x + V[:, 0]).max())
        assert err <= 1e-6 * max(1.0, 1e-9 / gap) + 2e-15 / gap, (s, sep, tc, err, gap)


def test_laguerre_iteration_counts_are_bounded():
    its = np.array([solve(A)[3] for A in EC.iteration_count_family()])
    print("Laguerre iterations: mean %.2f max %d" % (its.mean(), its.max()))
    assert its.mean() < 8 and its.max() <= 40


def test_small_eigenvector_entries_regression():
    """A pixel of the 6-dot `mid` scene: well separated ground state whose vector has an entry of 3e-7.  Inverse iteration
    on the top-down LDL^T (round 2's scheme) returned it wrong by 5e-10 (eigen residual 6e-10); the twisted factorisation
    gives every entry to working accuracy."""
    A = EC.small_entry_block()
    lam, x, res, it = solve(A)
    w, V = np.linalg.eigh(A)
    v0 = V[:, 0] * np.sign(V[0, 0]) * np.sign(x[0])
    assert res <= 2e-15 and abs(lam - w[0]) <= 1e-15
    assert np.all(np.abs(x - v0) <= 1e-13 * np.abs(v0) + 1e-20), (x, v0)


@pytest.mark.parametrize("s", EC.MIXED_SIZES)
def test_mixed_coupling_scales_inside_one_block(s):
    """couplings of one block spread over many decades (tc_i = tc_base exp(-alpha_i vb_i) differs per barrier): the residual
    stays at round-off and small vector entries keep their relative accuracy"""
    for rep, A in enumerate(EC.mixed_scale_family(s)):
        hn = np.abs(A).sum(axis=1).max()
        lam, x, res, it = solve(A)
        w, V = np.linalg.eigh(A)
        assert abs(lam - w[0]) <= 4e-15 * hn and res <= 4e-15 * hn, (s, rep, res / hn)


def test_column_tail_far_below_the_pivot_regression():
    """A 10-state block of the random-action sweep (seed 1234, env 8, tc up to 2e45 next to couplings of 7e-5): after
    scaling, a Householder column had x0 ~ 1e-66 and a tail of ~1e-160; v0^2 underflowed and tau = 0 * (1 / denormal) = NaN.
    Negligible tails are dropped now."""
    A = EC.column_tail_block()
    hn = np.abs(A).sum(axis=1).max()
    lam, x, res, it = solve(A)
    w = np.linalg.eigvalsh(A)
    assert np.isfinite(res) and np.all(np.isfinite(x))
    assert abs(lam - w[0]) <= 4e-15 * hn and res <= 4e-15 * hn


@pytest.mark.parametrize("s", EC.EXTREME_SIZES)
def test_extreme_scale_mix_never_gives_nan(s):
    for rep, A in enumerate(EC.extreme_scale_family(s)):
        hn = np.abs(A).sum(axis=1).max()
        lam, x, res, it = solve(A)
        assert np.isfinite(lam) and np.isfinite(res) and np.all(np.isfinite(x)), (s, rep)
        assert res <= 1e-14 * hn, (s, rep, res / hn)
