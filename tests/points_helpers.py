"""Shared by the point-evaluation tests (test_points_cpu.py, test_gpu_points.py): the CPU build of the point front end
(tests/hosttest_points) and the scan pixels' physical voltages, which are the points of the bit-for-bit tests."""
import ctypes
import os
import subprocess

import numpy as np

import helpers as H
from qadapt_hip import device_model as DM

_LIB = None


def points_lib():
    global _LIB
    if _LIB is None:
        hdir = os.path.join(H.ROOT, "tests", "hosttest_points")
        subprocess.check_call(["make", "-s", "-C", hdir, "libqdsim_hosttest_points.so"])
        _LIB = ctypes.CDLL(os.path.join(hdir, "libqdsim_hosttest_points.so"))
    return _LIB


def _d(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def scan_voltages(N, par, st, ch, R):
    """qd_pixel_voltages of every pixel of channel ch: v_ext (P, 2N), vpp (P, N+1), tc (P, N-1)"""
    par = np.ascontiguousarray(par, np.float64); st = np.ascontiguousarray(st, np.float64)
    P = R * R
    v_ext = np.zeros((P, 2 * N)); vpp = np.zeros((P, N + 1)); tc = np.zeros((P, N - 1))
    assert points_lib().qdhp_scan_voltages(N, _d(par), _d(st), int(ch), int(R), _d(v_ext), _d(vpp), _d(tc)) == 0
    return v_ext, vpp, tc


def scan_points(N, par, st, R):
    """the v_ext of every pixel of every channel, in the order of the raw signal: (C * P, 2N)"""
    return np.concatenate([scan_voltages(N, par, st, ch, R)[0] for ch in range(N - 1)])


def point_front(N, par, v_ext):
    """qd_point_front at the rows of v_ext (n, 2N): dict of vpp (n, N+1), tc (n, N-1), vd (n, N), ncont (n, N), isa (n,)"""
    par = np.ascontiguousarray(par, np.float64); v_ext = np.ascontiguousarray(v_ext, np.float64)
    n = v_ext.shape[0]
    out = dict(vpp=np.zeros((n, N + 1)), tc=np.zeros((n, N - 1)), vd=np.zeros((n, N)), ncont=np.zeros((n, N)), isa=np.zeros(n))
    rc = points_lib().qdhp_point_front(N, _d(par), ctypes.c_long(n), _d(v_ext), _d(out["vpp"]), _d(out["tc"]), _d(out["vd"]),
                                       _d(out["ncont"]), _d(out["isa"]))
    assert rc == 0
    return out


def blocks(N, seeds, linear=False):
    """helpers.sample_blocks, or the same draws with the linear voltage-dependent capacitance model on"""
    if not linear:
        return H.sample_blocks(N, seeds)
    q, e = H.configs()
    q["simulator"]["voltage_capacitance_model"]["type"] = "linear"
    s = DM.DeviceSampler(N, q, e)
    return s.build(np.stack([np.random.default_rng(int(sd)).random(s.n_draws) for sd in seeds]))


def bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)
