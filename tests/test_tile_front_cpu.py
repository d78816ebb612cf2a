"""The reworked pieces of the tile search, compiled for the CPU (tests/hosttest_tile), each against the form it replaced.
No GPU needed.

  * projected gradient (csrc/qd_pixel.h, qd_pixel_continuous<N, INTERLEAVED>): the row-major and the interleaved form of the
    same source, -ffp-contract=off, give bit-equal ncont, vd and isa for N = 2..8;
  * packed minimum / maximum of the floors (qd_fl_pack, qd_fl_pkmin): plain min / max over the admissible range;
  * selection (qd_tile_select): the uniform fill against the general loop: slots, ids, maxE / maxS / maxG, eout, count, redo.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers as H
from qadapt_hip.layout import layout

_LIB = None
D = ctypes.c_double
I = ctypes.c_int


def tile_lib():
    global _LIB
    if _LIB is None:
        hdir = os.path.join(H.ROOT, "tests", "hosttest_tile")
        subprocess.check_call(["make", "-s", "-C", hdir, "libqdsim_hosttest_tile.so"])
        _LIB = ctypes.CDLL(os.path.join(hdir, "libqdsim_hosttest_tile.so"))
        _LIB.qdht_fl_minmax.restype = None
    return _LIB


# ---------------------------------------------------------------------------------------------------------------------
# projected gradient
# ---------------------------------------------------------------------------------------------------------------------
NBLK = 2000
_BLOCKS = {}


def blocks(N):
    """NBLK parameter blocks of the product's device sampler (one per seed), shared by the cases and left unchanged"""
    if N not in _BLOCKS:
        _BLOCKS[N] = np.ascontiguousarray(H.sample_blocks(N, 9000 + np.arange(NBLK)).params)
        _BLOCKS[N].setflags(write=False)
    return _BLOCKS[N]


def run_pg(N, par, v_ext, vd):
    L = layout(N); n = par.shape[0]
    assert par.shape[1] == L.size
    out = []
    for il in (0, 1):
        vo = np.empty((n, N)); nc = np.empty((n, N)); isa = np.empty(n)
        rc = tile_lib().qdht_pg(N, il, ctypes.c_long(n), H._p(par, D), ctypes.c_long(L.size), H._p(v_ext, D), H._p(vd, D),
                                H._p(vo, D), H._p(nc, D), H._p(isa, D))
        assert rc == 0
        out.append((vo, nc, isa))
    return out


PG_CASES = ["random", "all_positive", "one_depleted", "all_depleted", "zero_vdash", "nan_row", "vc_model"]


@pytest.mark.parametrize("N", range(2, 9))
@pytest.mark.parametrize("case", PG_CASES)
def test_projected_gradient_forms_bit_equal(N, case):
    L = layout(N)
    rng = np.random.default_rng(100 * N + PG_CASES.index(case))
    par = blocks(N).copy()
    v_ext = rng.uniform(-3.0, 3.0, (NBLK, 2 * N))
    vd = rng.uniform(-2.0, 6.0, (NBLK, N))
    if case == "all_positive":
        vd = rng.uniform(0.05, 6.0, (NBLK, N))
    elif case == "one_depleted":
        vd = rng.uniform(0.05, 6.0, (NBLK, N))
        vd[np.arange(NBLK), rng.integers(0, N, NBLK)] = -rng.uniform(0.01, 3.0, NBLK)
    elif case == "all_depleted":
        vd = -rng.uniform(0.01, 3.0, (NBLK, N))
    elif case == "zero_vdash":
        vd[: NBLK // 2] = 0.0                                             # v' = 0 in every dot (no step runs)
        vd[NBLK // 2:, 0] = 0.0                                           # one zero among depleted and filled dots
        vd[NBLK // 2:, 1] = -rng.uniform(0.01, 3.0, NBLK - NBLK // 2)
    elif case == "nan_row":
        G = N + 1
        rows = rng.integers(0, N, NBLK)
        for b in range(NBLK):
            par[b, L.cdd_inv + rows[b] * G: L.cdd_inv + rows[b] * G + N] = np.nan
        vd[np.arange(NBLK), rng.integers(0, N, NBLK)] = -1.0             # the steps run
    elif case == "vc_model":
        par[:, L.scal + 4] = 1.0
        par[:, L.scal + 5] = rng.uniform(0.0, 0.05, NBLK)
        par[:, L.scal + 6] = rng.uniform(0.0, 0.05, NBLK)
    par = np.ascontiguousarray(par); v_ext = np.ascontiguousarray(v_ext); vd = np.ascontiguousarray(vd)
    (vo0, nc0, isa0), (vo1, nc1, isa1) = run_pg(N, par, v_ext, vd)
    for a, b in ((vo0, vo1), (nc0, nc1), (isa0, isa1)):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    if case in ("random", "one_depleted", "vc_model"):                    # (all dots depleted: n stays at 0)
        assert (nc0 != np.maximum(vo0, 0)).any()                          # the 50 steps ran: not the clipped v'


# ---------------------------------------------------------------------------------------------------------------------
# packed min / max
# ---------------------------------------------------------------------------------------------------------------------
BIAS = 0x7FFF


def fl_minmax(fl):
    fl = np.ascontiguousarray(fl, np.int32); mn = I(0); mx = I(0)
    tile_lib().qdht_fl_minmax(H._p(fl, I), ctypes.byref(mn), ctypes.byref(mx))
    return mn.value, mx.value


def test_packed_floor_min_max():
    rng = np.random.default_rng(3)
    lib = tile_lib()
    for v, ok in ((0, 1), (1, 1), (BIAS - 1, 1), (BIAS, 1), (BIAS + 1, 0), (-1, 0), (2 ** 31 - 1, 0), (-2 ** 31, 0), (0x10000, 0)):
        assert lib.qdht_fl_packable(I(v)) == ok, v
    for rep in range(600):
        kind = rep % 4
        if kind == 0:
            fl = rng.integers(0, BIAS + 1, 64)
        elif kind == 1:
            fl = rng.integers(0, 6, 64) + rng.integers(0, BIAS - 5)         # a tile's spread
        elif kind == 2:
            fl = np.full(64, rng.integers(0, BIAS + 1)); fl[rng.integers(0, 64)] = rng.choice([0, BIAS])
        else:
            fl = rng.choice([0, BIAS], 64)
        assert fl_minmax(fl) == (int(fl.min()), int(fl.max())), fl
    for lane in range(64):                                                  # both ends, in every lane
        fl = np.full(64, 100); fl[lane] = 0; fl[(lane + 17) % 64] = BIAS
        assert fl_minmax(fl) == (0, BIAS)
    assert fl_minmax(np.zeros(64)) == (0, 0) and fl_minmax(np.full(64, BIAS)) == (BIAS, BIAS)


# ---------------------------------------------------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------------------------------------------------
SCAP = 383


def run_select(KC, fill, nS, nSfront, scode, sD, sa, sb, xs, ys, blo, bhi, amb):
    e = np.zeros(32); ids = np.zeros(32, np.uint16); maxE = D(0); eout = D(0); ms = np.zeros(3, np.int32); redo = I(0)
    U32 = ctypes.c_uint32
    rc = tile_lib().qdht_select(KC, fill, nS, nSfront, SCAP, H._p(scode, U32), H._p(sD, D), H._p(sa, D), H._p(sb, D), D(xs), D(ys),
                                U32(blo), U32(bhi), D(amb), H._p(e, D), H._p(ids, ctypes.c_uint16), ctypes.byref(maxE), H._p(ms, I),
                                ctypes.byref(eout), ctypes.byref(redo))
    assert rc == 0
    return e[:KC].tobytes(), ids[:KC].tobytes(), maxE.value, tuple(ms), eout.value, redo.value


@pytest.mark.parametrize("KC", [8, 16, 32])
@pytest.mark.parametrize("energies", ["random", "ties"])
def test_uniform_fill_equals_general_loop(KC, energies):
    rng = np.random.default_rng(KC + (0 if energies == "random" else 1))
    blo, bhi = 0x00000000, 0x33333333                                      # the lane's box: digits 0..3 of 8 dots
    redone = 0
    for rep in range(500):
        nSfront = KC + int(rng.integers(0, 3 * KC)) if rep % 5 else KC
        nback = int(rng.integers(0, SCAP - nSfront)) if rep % 3 else 0
        nS = nSfront + nback
        digits = rng.integers(0, 4, (SCAP, 8))
        back = np.ones(SCAP, bool); back[:nSfront] = False                 # states of the front are valid in every lane
        spoil = back & (rng.random(SCAP) < 0.4)
        digits[spoil, rng.integers(0, 8, spoil.sum())] = rng.integers(4, 8, spoil.sum())
        scode = np.ascontiguousarray((digits << (4 * np.arange(7, -1, -1))).sum(axis=1).astype(np.uint32))
        if energies == "random":
            sD, sa, sb = rng.normal(0, 1, SCAP), rng.normal(0, 0.1, SCAP), rng.normal(0, 0.1, SCAP); amb = 1e-3
        else:
            sD, sa, sb = (rng.integers(0, 5, SCAP).astype(float), rng.integers(-1, 2, SCAP).astype(float),
                          rng.integers(-1, 2, SCAP).astype(float)); amb = 0.5
        xs, ys = float(rng.integers(-3, 5)), float(rng.integers(-3, 5))
        a = run_select(KC, 0, nS, nSfront, scode, sD, sa, sb, xs, ys, blo, bhi, amb)
        b = run_select(KC, 1, nS, nSfront, scode, sD, sa, sb, xs, ys, blo, bhi, amb)
        assert a == b, (rep, a[2:], b[2:])
        assert a[3][2] == KC
        redone += a[5]
    assert 0 < redone < 500                                                 # both outcomes of the redo decision were met
    # fewer than KC states in the front: the general path of both
    for nSfront in (0, KC - 1):
        scode = np.zeros(SCAP, np.uint32); sD = rng.normal(0, 1, SCAP); z = np.zeros(SCAP)
        a = run_select(KC, 0, nSfront + 5, nSfront, scode, sD, z, z, 0.0, 0.0, blo, bhi, 1e-3)
        b = run_select(KC, 1, nSfront + 5, nSfront, scode, sD, z, z, 0.0, 0.0, blo, bhi, 1e-3)
        assert a == b
