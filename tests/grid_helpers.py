"""Shared by the grid tests (test_grid_cpu.py, test_gpu_scan_grid.py): the CPU build of the grid front end (tests/hosttest_grid:
qd_grid_voltages, qd_grid_record and the row walk of the latching stage, csrc/qd_grid.h) and a NumPy statement of the points
an nx x ny grid visits."""
import ctypes
import os
import subprocess

import numpy as np

import affine_helpers as AH
import helpers as H
import line_helpers as LH
from qadapt_hip.layout import layout

VIRTUAL, PHYSICAL = 0, 1
_LIB = None


def grid_lib():
    global _LIB
    if _LIB is None:
        hdir = os.path.join(H.ROOT, "tests", "hosttest_grid")
        subprocess.check_call(["make", "-s", "-C", hdir, "libqdsim_hosttest_grid.so"])
        _LIB = ctypes.CDLL(os.path.join(hdir, "libqdsim_hosttest_grid.so"))
    return _LIB


def _d(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def _dirs(N, dx, dy):
    dirs = np.ascontiguousarray(np.stack([np.asarray(dx, np.float64), np.asarray(dy, np.float64)]))
    assert dirs.shape == (2, 2 * N)
    return dirs


def grid_voltages(N, par, st, dx, dy, ranges, nx, ny, frame=VIRTUAL):
    """qd_grid_voltages of every point (row-major, p = y nx + x): v_ext (ny*nx, 2N), vpp (ny*nx, N+1), tc (ny*nx, N-1)"""
    par = np.ascontiguousarray(par, np.float64); st = np.ascontiguousarray(st, np.float64)
    rg = np.ascontiguousarray(ranges, np.float64).reshape(4)
    dirs = _dirs(N, dx, dy)
    n = nx * ny
    v_ext = np.zeros((n, 2 * N)); vpp = np.zeros((n, N + 1)); tc = np.zeros((n, N - 1))
    rc = grid_lib().qdhg_grid_voltages(N, _d(par), _d(st), _d(dirs), int(frame), _d(rg), int(nx), int(ny), _d(v_ext), _d(vpp), _d(tc))
    assert rc == 0, rc
    return v_ext, vpp, tc


def grid_records(N, par, st, dx, dy, ranges, nx, ny, frame=VIRTUAL, fill=0xA5):
    """The side*side records of the grid's slot as qd_grid_record leaves them, over a buffer pre-filled with `fill`:
    (bytes (SP, record size) uint8, live (SP,) bool)"""
    par = np.ascontiguousarray(par, np.float64); st = np.ascontiguousarray(st, np.float64)
    rg = np.ascontiguousarray(ranges, np.float64).reshape(4)
    dirs = _dirs(N, dx, dy)
    side = LH.slot(nx * ny)[0]
    SP, size = side * side, int(grid_lib().qdhg_record_bytes())
    recs = np.full((SP, size), fill, np.uint8)
    live = np.zeros(SP, np.int32)
    rc = grid_lib().qdhg_grid_records(N, _d(par), _d(st), _d(dirs), int(frame), _d(rg), int(nx), int(ny),
                                      recs.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), live.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
    assert rc == 0, rc
    return recs, live.astype(bool)


def latch_grid(N, par, occ, z, nx, ny, stream):
    """The latching walk of one slot as the grid's kernel runs it (one row of nx points after the other, in place on copies):
    occ (SP, N) and z (SP,) with SP >= nx*ny; `stream` a qd_noise_oracle.Stream.  Returns (occ, z)."""
    par = np.ascontiguousarray(par, np.float64)
    occ = np.array(occ, np.float64, order="C"); z = np.array(z, np.float64, order="C")
    assert occ.shape == (z.shape[0], N) and z.shape[0] >= nx * ny
    u32 = ctypes.c_uint32
    rc = grid_lib().qdhg_latch_grid(N, _d(par), _d(occ), _d(z), int(nx), int(ny), u32(stream.k0), u32(stream.ser_lo), u32(stream.ser_hi),
                                    u32(stream.k1))
    assert rc == 0, rc
    return occ, z


def numpy_w(W0, dx, dy, ranges, nx, ny):
    """NumPy statement of W (ny, nx, 2N), rows y, columns x: W0 + sx dx + sy dy (rounded as NumPy rounds it)"""
    sx = np.linspace(ranges[0], ranges[1], nx)[None, :, None]
    sy = np.linspace(ranges[2], ranges[3], ny)[:, None, None]
    return np.asarray(W0, np.float64) + sx * np.asarray(dx, np.float64) + sy * np.asarray(dy, np.float64)


def numpy_grid(N, st, origin, dx, dy, ranges, nx, ny, frame=VIRTUAL):
    """NumPy statement of the grid's v_ext (ny, nx, 2N)"""
    L = layout(N); G = N + 1
    W = numpy_w(AH.base_point(N, st), dx, dy, ranges, nx, ny)
    if frame == PHYSICAL:
        return W
    vgm = st[L.s_vgm:L.s_vgm + G * G].reshape(G, G)
    out = W.copy()
    out[:, :, :G] = np.einsum("ij,...j->...i", vgm, W[:, :, :G]) + origin
    return out
