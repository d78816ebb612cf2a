"""The wave-per-block dense eigen-solver of the 33..64-state sectors (csrc/qd_eig_wave.h), compiled for the CPU with the
64 lanes as a loop (tests/hosttest_wave), against numpy.linalg.eigh.  Bars: |lambda - lambda_eigh| <= 1e-12 ||A||_inf,
residual <= 1e-13 ||A||_inf, eigenvector entries within 1e-8 wherever the relative gap of the two lowest eigenvalues
exceeds helpers.GAP_MIN.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import eig_cases as EC

_LIB = None


def wave_lib():
    global _LIB
    if _LIB is None:
        hdir = os.path.join(H.ROOT, "tests", "hosttest_wave")
        subprocess.check_call(["make", "-s", "-C", hdir, "libqdsim_hosttest_wave.so"])
        _LIB = ctypes.CDLL(os.path.join(hdir, "libqdsim_hosttest_wave.so"))
    return _LIB


def solve(A):
    h = wave_lib()
    s = A.shape[0]
    packed = np.ascontiguousarray(A[np.tril_indices(s)], dtype=np.float64)
    lam = ctypes.c_double(); res = ctypes.c_double(); it = ctypes.c_int()
    x = np.zeros(s)
    rc = h.qdhw_eig_lowest(s, H._p(packed, ctypes.c_double), ctypes.byref(lam), H._p(x, ctypes.c_double),
                           ctypes.byref(res), ctypes.byref(it))
    assert rc == 0
    return lam.value, x, res.value, it.value


def check(A, tag):
    """the bars of the module docstring; returns the relative gap"""
    w, V = np.linalg.eigh(A)
    hn = np.abs(A).sum(axis=1).max()
    lam, x, res, it = solve(A)
    assert np.isfinite(x).all() and np.isfinite(lam), tag
    assert abs(lam - w[0]) <= 1e-12 * hn, (tag, lam, w[0], hn)
    assert res <= 1e-13 * hn, (tag, res / hn)
    assert abs(np.linalg.norm(x) - 1) < 1e-13, tag
    # the residual the solver reports is the residual of what it returns (each side is a 64-term float64 sum per row:
    # rounding of at most 64 eps ||A||_inf = 1.4e-14 ||A||_inf apiece)
    assert abs(np.linalg.norm(A @ x - lam * x) - res) <= 3e-14 * hn, tag
    gap = (w[1] - w[0]) / hn
    if gap > H.GAP_MIN:
        err = min(np.abs(x - V[:, 0]).max(), np.abs(x + V[:, 0]).max())
        assert err <= 1e-8, (tag, err, gap)
    assert 1 <= it <= 64, (tag, it)
    return gap


@pytest.mark.parametrize("s", EC.WIDE_SIZES)
def test_random_symmetric_blocks_of_every_wide_size(s):
    for tag, A in EC.wide_random_family(s):
        check(A, tag)


@pytest.mark.parametrize("s", EC.WIDE_HOP_SIZES)
def test_hop_type_blocks_over_coupling_scales(s):
    """non-negative diagonal of O(1), non-positive couplings from 1e-22 to 1e44 on a connected sparse graph"""
    for tag, A in EC.wide_hop_family(s):
        check(A, tag)


def test_small_sizes_run_too():
    for s, A in EC.wide_small_family():
        check(A, s)


def test_size_outside_one_wave_is_an_error():
    h = wave_lib()
    z = np.zeros(65 * 33)
    lam = ctypes.c_double(); res = ctypes.c_double(); it = ctypes.c_int()
    assert h.qdhw_eig_lowest(65, H._p(z, ctypes.c_double), ctypes.byref(lam), H._p(z, ctypes.c_double),
                             ctypes.byref(res), ctypes.byref(it)) == 1


@pytest.mark.parametrize("N,m", [(4, 3), (5, 2)])
def test_real_sector_blocks(N, m):
    """Every sector of more than 32 states, out of the scenes the GPU test runs (near / far / random actions: tunnel
    couplings up to ~1e45 occur) -- the blocks as the structure kernel hands them over, diagonal relative to the
    pixel's lowest free energy."""
    tcmax, n, resolved = 0.0, 0, 0
    for tag, A, tcmax in EC.wide_sector_family(N, m):
        resolved += check(A, tag) > H.GAP_MIN
        n += 1
    print(f"({N},{m}): {n} sector blocks, {resolved} with a resolved ground vector, largest coupling {tcmax:.1e}")
    assert resolved > 0


def test_nearly_degenerate_lowest_pair():
    """two weakly coupled copies of the same block: the two lowest levels split by ~1e-11 ||A|| and by ~1e-6 ||A||"""
    for tag, A in EC.wide_degenerate_family():
        check(A, tag)


def test_householder_tail_that_underflows():
    """couplings 60 decades apart inside one block: the reflector of a column whose tail is ~1e-160 of its head would
    need v0^2 ~ 1e-320 (the NaN case of the per-lane solver at tc ~ 2e45); the tail is dropped instead"""
    for tag, A in EC.wide_underflow_family():
        check(A, tag)
