"""Shared by the affine-scan tests (test_affine_cpu.py, test_gpu_scan_affine.py): the CPU build of the affine front end
(tests/hosttest_affine: qd_affine_voltages behind QdFrontAffine) and a NumPy statement of the grids an affine scan renders."""
import ctypes
import os
import subprocess

import numpy as np

import helpers as H
from qadapt_hip.layout import layout

VIRTUAL, PHYSICAL = 0, 1
_LIB = None


def affine_lib():
    global _LIB
    if _LIB is None:
        hdir = os.path.join(H.ROOT, "tests", "hosttest_affine")
        subprocess.check_call(["make", "-s", "-C", hdir, "libqdsim_hosttest_affine.so"])
        _LIB = ctypes.CDLL(os.path.join(hdir, "libqdsim_hosttest_affine.so"))
    return _LIB


def _d(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def affine_voltages(N, par, st, dx, dy, ranges, R, frame=VIRTUAL):
    """qd_affine_voltages of every pixel (row-major, p = y R + x): v_ext (P, 2N), vpp (P, N+1), tc (P, N-1)"""
    par = np.ascontiguousarray(par, np.float64); st = np.ascontiguousarray(st, np.float64)
    rg = np.ascontiguousarray(ranges, np.float64).reshape(4)
    dirs = np.ascontiguousarray(np.stack([np.asarray(dx, np.float64), np.asarray(dy, np.float64)]))
    assert dirs.shape == (2, 2 * N)
    P = R * R
    v_ext = np.zeros((P, 2 * N)); vpp = np.zeros((P, N + 1)); tc = np.zeros((P, N - 1))
    rc = affine_lib().qdha_affine_voltages(N, _d(par), _d(st), _d(dirs), int(frame), _d(rg), int(R), _d(v_ext), _d(vpp), _d(tc))
    assert rc == 0, rc
    return v_ext, vpp, tc


def unit(N, i):
    v = np.zeros(2 * N)
    v[i] = 1.0
    return v


def base_point(N, st):
    """W0 = [gate_v, sensor_v, barrier_v] of a state block"""
    L = layout(N)
    return np.concatenate([st[L.s_gate_v:L.s_gate_v + N], [st[L.s_sensor_gt]], st[L.s_barrier_v:L.s_barrier_v + N - 1]])


def numpy_w(W0, dx, dy, ranges, R):
    """NumPy statement of W (R, R, 2N), rows y, columns x: W0 + sx dx + sy dy (rounded as NumPy rounds it)"""
    sx = np.linspace(ranges[0], ranges[1], R)[None, :, None]
    sy = np.linspace(ranges[2], ranges[3], R)[:, None, None]
    return np.asarray(W0, np.float64) + sx * np.asarray(dx, np.float64) + sy * np.asarray(dy, np.float64)


def numpy_grid(N, st, origin, dx, dy, ranges, R, frame=VIRTUAL):
    """NumPy statement of the affine scan's v_ext (R, R, 2N)"""
    L = layout(N); G = N + 1
    W = numpy_w(base_point(N, st), dx, dy, ranges, R)
    if frame == PHYSICAL:
        return W
    vgm = st[L.s_vgm:L.s_vgm + G * G].reshape(G, G)
    out = W.copy()
    out[:, :, :G] = np.einsum("ij,...j->...i", vgm, W[:, :, :G]) + origin
    return out
