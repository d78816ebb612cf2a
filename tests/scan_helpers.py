"""Shared by the axis-scan tests (test_scan_cpu.py, test_gpu_scan2d.py): the CPU build of the scan front end
(tests/hosttest_scan: qd_scan_voltages beside qd_pixel_voltages and qd_point_front) and a NumPy statement of the grids a
scan renders."""
import ctypes
import os
import subprocess

import numpy as np

import helpers as H
from qadapt_hip.layout import layout

VIRTUAL, PHYSICAL = 0, 1
_LIB = None


def scan_lib():
    global _LIB
    if _LIB is None:
        hdir = os.path.join(H.ROOT, "tests", "hosttest_scan")
        subprocess.check_call(["make", "-s", "-C", hdir, "libqdsim_hosttest_scan.so"])
        _LIB = ctypes.CDLL(os.path.join(hdir, "libqdsim_hosttest_scan.so"))
        _LIB.qdhs_peak_width_pair.restype = ctypes.c_double
        _LIB.qdhs_peak_width.restype = ctypes.c_double
    return _LIB


def _d(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def query_state(N, st, gate_v, barrier_v, sensor_v=0.0, vgm=None):
    """the state block a scan query renders: the env's, with the query's voltages (and matrix)"""
    L = layout(N); G = N + 1
    st = np.array(st, np.float64)
    st[L.s_gate_v:L.s_gate_v + N] = gate_v
    st[L.s_barrier_v:L.s_barrier_v + N - 1] = barrier_v
    st[L.s_sensor_gt] = sensor_v
    if vgm is not None:
        st[L.s_vgm:L.s_vgm + G * G] = np.asarray(vgm, np.float64).reshape(-1)
    return st


def scan_voltages(N, par, st, ax, ay, ranges, R, frame=VIRTUAL):
    """qd_scan_voltages of every pixel (row-major, p = y R + x): v_ext (P, 2N), vpp (P, N+1), tc (P, N-1)"""
    par = np.ascontiguousarray(par, np.float64); st = np.ascontiguousarray(st, np.float64)
    rg = np.ascontiguousarray(ranges, np.float64).reshape(4)
    P = R * R
    v_ext = np.zeros((P, 2 * N)); vpp = np.zeros((P, N + 1)); tc = np.zeros((P, N - 1))
    rc = scan_lib().qdhs_scan_voltages(N, _d(par), _d(st), int(ax), int(ay), int(frame), _d(rg), int(R), _d(v_ext), _d(vpp), _d(tc))
    assert rc == 0, rc
    return v_ext, vpp, tc


def pixel_voltages(N, par, st, ch, R):
    par = np.ascontiguousarray(par, np.float64); st = np.ascontiguousarray(st, np.float64)
    P = R * R
    v_ext = np.zeros((P, 2 * N)); vpp = np.zeros((P, N + 1)); tc = np.zeros((P, N - 1))
    assert scan_lib().qdhs_pixel_voltages(N, _d(par), _d(st), int(ch), int(R), _d(v_ext), _d(vpp), _d(tc)) == 0
    return v_ext, vpp, tc


def point_front(N, par, v_ext):
    par = np.ascontiguousarray(par, np.float64); v_ext = np.ascontiguousarray(v_ext, np.float64)
    n = v_ext.shape[0]
    vpp = np.zeros((n, N + 1)); tc = np.zeros((n, N - 1))
    assert scan_lib().qdhs_point_front(N, _d(par), ctypes.c_long(n), _d(v_ext), _d(vpp), _d(tc)) == 0
    return vpp, tc


def peak_width_pair(N, par, st, i, j):
    par = np.ascontiguousarray(par, np.float64); st = np.ascontiguousarray(st, np.float64)
    return scan_lib().qdhs_peak_width_pair(N, _d(par), _d(st), int(i), int(j))


def peak_width(N, par, st, ch):
    par = np.ascontiguousarray(par, np.float64); st = np.ascontiguousarray(st, np.float64)
    return scan_lib().qdhs_peak_width(N, _d(par), _d(st), int(ch))


def adjacent_ranges(gate_v, c, w):
    """the ranges that make scan (c, c+1) the probe's channel c: fl(v + (-w)), fl(v + w), as qd_pixel_voltages forms them"""
    v1, v2 = np.float64(gate_v[c]), np.float64(gate_v[c + 1])
    w = np.float64(w)
    return np.array([v1 + (-w), v1 + w, v2 + (-w), v2 + w], np.float64)


def numpy_grid(N, st, origin, ax, ay, ranges, R, frame=VIRTUAL):
    """NumPy statement of the scan's v_ext (R, R, 2N): rows y, columns x"""
    L = layout(N); G = N + 1
    W = np.concatenate([st[L.s_gate_v:L.s_gate_v + N], [st[L.s_sensor_gt]], st[L.s_barrier_v:L.s_barrier_v + N - 1]])
    Wg = np.broadcast_to(W, (R, R, 2 * N)).copy()
    Wg[:, :, ax] = np.linspace(ranges[0], ranges[1], R)[None, :]
    Wg[:, :, ay] = np.linspace(ranges[2], ranges[3], R)[:, None]
    if frame == PHYSICAL:
        return Wg
    vgm = st[L.s_vgm:L.s_vgm + G * G].reshape(G, G)
    out = Wg.copy()
    out[:, :, :G] = np.einsum("ij,...j->...i", vgm, Wg[:, :, :G]) + origin
    return out
