"""Shared by the line tests (test_line_cpu.py, test_gpu_scan1d.py): the CPU build of the line front end (tests/hosttest_line:
qd_line_voltages, qd_line_record and the slot arithmetic of csrc/qd_line.h) and a NumPy statement of the points a line visits."""
import ctypes
import os
import subprocess

import numpy as np

import affine_helpers as AH
import helpers as H
from qadapt_hip.layout import layout

VIRTUAL, PHYSICAL = 0, 1
_LIB = None


def line_lib():
    global _LIB
    if _LIB is None:
        hdir = os.path.join(H.ROOT, "tests", "hosttest_line")
        subprocess.check_call(["make", "-s", "-C", hdir, "libqdsim_hosttest_line.so"])
        _LIB = ctypes.CDLL(os.path.join(hdir, "libqdsim_hosttest_line.so"))
    return _LIB


def _d(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def line_voltages(N, par, st, d, s_range, n, frame=VIRTUAL):
    """qd_line_voltages of every point: v_ext (n, 2N), vpp (n, N+1), tc (n, N-1)"""
    par = np.ascontiguousarray(par, np.float64); st = np.ascontiguousarray(st, np.float64)
    rg = np.ascontiguousarray(s_range, np.float64).reshape(2)
    d = np.ascontiguousarray(d, np.float64)
    assert d.shape == (2 * N,)
    v_ext = np.zeros((n, 2 * N)); vpp = np.zeros((n, N + 1)); tc = np.zeros((n, N - 1))
    rc = line_lib().qdhl_line_voltages(N, _d(par), _d(st), _d(d), int(frame), _d(rg), int(n), _d(v_ext), _d(vpp), _d(tc))
    assert rc == 0, rc
    return v_ext, vpp, tc


def slot(n, ppb=256):
    """(side, tail records, ground-state batches) of the slot of a line of n points"""
    out = np.zeros(3, np.int32)
    assert line_lib().qdhl_slot(int(n), int(ppb), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int))) == 0
    return tuple(int(v) for v in out)


def line_records(N, par, st, d, s_range, n, frame=VIRTUAL, fill=0xA5):
    """The side*side records of the line's slot as qd_line_record leaves them, over a buffer pre-filled with `fill`:
    (bytes (SP, record size) uint8, live (SP,) bool)"""
    par = np.ascontiguousarray(par, np.float64); st = np.ascontiguousarray(st, np.float64)
    rg = np.ascontiguousarray(s_range, np.float64).reshape(2)
    d = np.ascontiguousarray(d, np.float64)
    side = slot(n)[0]
    SP, size = side * side, int(line_lib().qdhl_record_bytes())
    recs = np.full((SP, size), fill, np.uint8)
    live = np.zeros(SP, np.int32)
    rc = line_lib().qdhl_line_records(N, _d(par), _d(st), _d(d), int(frame), _d(rg), int(n),
                                      recs.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), live.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    assert rc == 0, rc
    return recs, live.astype(bool)


def numpy_w(W0, d, s_range, n):
    """NumPy statement of W (n, 2N): W0 + s d (rounded as NumPy rounds it)"""
    s = np.linspace(s_range[0], s_range[1], n)[:, None]
    return np.asarray(W0, np.float64) + s * np.asarray(d, np.float64)


def numpy_line(N, st, origin, d, s_range, n, frame=VIRTUAL):
    """NumPy statement of the line's v_ext (n, 2N)"""
    L = layout(N); G = N + 1
    W = numpy_w(AH.base_point(N, st), d, s_range, n)
    if frame == PHYSICAL:
        return W
    vgm = st[L.s_vgm:L.s_vgm + G * G].reshape(G, G)
    out = W.copy()
    out[:, :G] = W[:, :G] @ vgm.T + origin
    return out
