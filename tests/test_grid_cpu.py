"""Grids of nx x ny points (qd_scan_grid), CPU tier: the grid front end (csrc/qd_grid.h: qd_grid_voltages, compiled for the host
in tests/hosttest_grid) against the affine front end bit for bit at nx = ny and against the line front end at ny = 1, against
NumPy at rectangular shapes and against the reference composer's do2d with nx != ny (tests/golden/grid_grids.npz); the slot
arithmetic and the inert tail records; the row starts of the latching walk; a stand-alone sanitizer run of the host harness;
the argument checks, prototype and export of qd_scan_grid; the axis resolver; the `env.array.scan_grid` mirror and the
`env.array.model.do2d_open` facade on a stub backend.  No GPU needed."""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest
import yaml

import affine_helpers as AH
import grid_helpers as GH
import helpers as H
import line_helpers as LH
import points_helpers as PH
import qd_noise_oracle as NO
import scan_helpers as SH
from qadapt_hip import device_model as DM
from qadapt_hip.env import QuantumDeviceEnv
from qadapt_hip.layout import layout

ROOT = H.ROOT
EPS = np.finfo(np.float64).eps


def _scene(N, seed, mode="mid"):
    eb = H.sample_blocks(N, [seed])
    rng = np.random.default_rng(seed)
    par, st = eb.params[0], H.place(N, eb.state[0], mode, rng)
    st[layout(N).s_sensor_gt] = rng.uniform(-1, 1)
    return par, st, rng


def _directions(N, rng):
    """a plunger, the sensor, a barrier, an e axis and a dense direction"""
    from qadapt_hip.vec_env import scan_axis_vector as vec
    return [("plunger", vec(N - 1, N)), ("sensor", vec("S", N)), ("barrier", vec("B1", N)), ("e", vec(f"e1_{N}", N)),
            ("dense", rng.normal(0, 1, 2 * N))]


# ------------------------------------------------------------------ the affine front end at nx = ny
@pytest.mark.parametrize("N", [2, 4, 8])
def test_grid_voltages_equal_the_affine_front_end_at_square_shapes(N):
    """qd_grid_voltages(dx, dy, nx = ny = R) has the bits of qd_affine_voltages(dx, dy, R) at every pixel, in v_ext, vpp and tc:
    both frames, every ordered pair of a plunger, the sensor, a barrier, an e axis and a dense direction that has two
    different members, a forward and a reversed range, R in {1, 5, 8}."""
    par, st, rng = _scene(N, 1900 + N)
    for frame in (GH.VIRTUAL, GH.PHYSICAL):
        for R in (1, 5, 8):
            dirs = _directions(N, rng)
            for xn, dx in dirs:
                for yn, dy in dirs:
                    if xn == yn:
                        continue
                    rg = np.array([-3.25, 7.5, 6.5, -2.75]) + rng.uniform(-1, 1, 4)
                    got = GH.grid_voltages(N, par, st, dx, dy, rg, R, R, frame)
                    ref = AH.affine_voltages(N, par, st, dx, dy, rg, R, frame)
                    for what, a, b in zip(("v_ext", "vpp", "tc"), got, ref):
                        assert np.isfinite(a).all()
                        assert PH.same(a, b), (what, frame, R, xn, yn)
                    if R > 1 and "sensor" not in (xn, yn):
                        vpp = got[1].reshape(R, R, N + 1)
                        assert np.ptp(vpp, axis=0).max() > 0 and np.ptp(vpp, axis=1).max() > 0       # both axes move


# ------------------------------------------------------------------ the line front end at ny = 1
@pytest.mark.parametrize("N", [2, 4, 8])
def test_grid_voltages_equal_the_line_front_end_on_one_row(N):
    """qd_grid_voltages(dx = d, dy = 0, nx = n, ny = 1) has the bits of qd_line_voltages(d, [x_lo, x_hi], n): both frames, the
    five directions, a forward and a reversed range, n in {1, 5, 8, 37}.  (The y range is finite and arbitrary: with ny = 1,
    sy = y_lo and fma(sy, 0, w) = w for every w but -0.)"""
    par, st, rng = _scene(N, 1920 + N)
    for frame in (GH.VIRTUAL, GH.PHYSICAL):
        for n in (1, 5, 8, 37):
            for name, d in _directions(N, rng):
                for rg in ((-3.25, 7.5), (6.5, -2.75)):
                    rg = np.array(rg) + rng.uniform(-1, 1, 2)
                    got = GH.grid_voltages(N, par, st, d, np.zeros(2 * N), [rg[0], rg[1], 11.0, -2.0], n, 1, frame)
                    ref = LH.line_voltages(N, par, st, d, rg, n, frame)
                    for what, a, b in zip(("v_ext", "vpp", "tc"), got, ref):
                        assert PH.same(a, b), (what, frame, n, name, tuple(rg))


# ------------------------------------------------------------------ rectangular shapes against NumPy
SHAPES = [(1, 1), (5, 3), (3, 5), (8, 1), (1, 8)]


@pytest.mark.parametrize("N", [2, 4, 8])
def test_rectangular_grids_match_numpy(N):
    """v_ext against NumPy at (nx, ny) in {(1, 1), (5, 3), (3, 5), (8, 1), (1, 8)}, a forward x range with a reversed y range
    and the other way round, dense directions.  Physical frame: W[i] = fma(sy, dy[i], fma(sx, dx[i], W0[i])) against NumPy's
    W0 + sx dx + sy dy.  The front end rounds twice, NumPy four times, each by at most eps / 2 of a partial sum bounded by
    M = |W0| + Sx |dx| + Sy |dy| with S = |lo| + |hi| >= |s|: 3 eps M; sx and sy are start + i * step on both sides with the
    same three roundings, at most 3 eps S apart (the bound of test_line_cpu): another 3 eps (Sx |dx| + Sy |dy|).  6 eps M
    per element bounds the sum.  Virtual frame: the same W through the matrix, (G + 1) eps (|VGM| |W| + |origin|) for the G
    products and sums of a row on either side, on top of 6 eps |VGM| M.  vpp and tc have the bits of qd_point_front at that
    v_ext, and the grid is laid out row-major with x along columns: the NumPy grid with its axes swapped is NOT within the bound."""
    par, st, rng = _scene(N, 1940 + N)
    L, G = layout(N), N + 1
    W0 = AH.base_point(N, st)
    origin = par[L.origin:L.origin + G]
    vgm = st[L.s_vgm:L.s_vgm + G * G].reshape(G, G)
    for nx, ny in SHAPES:
        for rg in ([-3.25, 7.5, 6.5, -2.75], [4.5, -1.25, -0.75, 2.5]):
            rg = np.array(rg) + rng.uniform(-0.5, 0.5, 4)
            dx, dy = rng.normal(0, 1, 2 * N), rng.normal(0, 1, 2 * N)
            M = np.abs(W0) + (abs(rg[0]) + abs(rg[1])) * np.abs(dx) + (abs(rg[2]) + abs(rg[3])) * np.abs(dy)
            v_ext, vpp, tc = GH.grid_voltages(N, par, st, dx, dy, rg, nx, ny, GH.PHYSICAL)
            want = GH.numpy_grid(N, st, None, dx, dy, rg, nx, ny, GH.PHYSICAL)
            tol = 6 * EPS * M
            got = v_ext.reshape(ny, nx, 2 * N)
            assert np.all(np.abs(got - want) <= tol), (nx, ny, float((np.abs(got - want) / tol).max()))
            pv, pt = SH.point_front(N, par, v_ext)
            assert PH.same(vpp, pv) and PH.same(tc, pt), (nx, ny)
            if nx > 1 and ny > 1:
                t = GH.numpy_grid(N, st, None, dy, dx, [rg[2], rg[3], rg[0], rg[1]], ny, nx, GH.PHYSICAL).transpose(1, 0, 2)
                assert t.shape == want.shape and np.all(np.abs(t - want) <= tol)          # the same points, built transposed
                wrong = GH.numpy_grid(N, st, None, dy, dx, rg, nx, ny, GH.PHYSICAL)       # the axes swapped
                assert not np.all(np.abs(got - wrong) <= tol), (nx, ny)
            # corner points: the ends of both ranges, x along columns
            assert np.all(np.abs(got[0, 0] - (W0 + rg[0] * dx + rg[2] * dy)) <= tol)
            assert np.all(np.abs(got[-1, -1] - (W0 + (rg[1] if nx > 1 else rg[0]) * dx + (rg[3] if ny > 1 else rg[2]) * dy)) <= tol)
            v_ext, vpp, tc = GH.grid_voltages(N, par, st, dx, dy, rg, nx, ny, GH.VIRTUAL)
            want = GH.numpy_grid(N, st, origin, dx, dy, rg, nx, ny, GH.VIRTUAL)
            Wn = np.abs(GH.numpy_w(W0, dx, dy, rg, nx, ny)[:, :, :G])
            tol = np.empty((ny, nx, 2 * N))
            tol[:, :, :G] = (G + 1) * EPS * (Wn @ np.abs(vgm).T + np.abs(origin)) + 6 * EPS * (np.abs(vgm) @ M[:G])
            tol[:, :, G:] = 6 * EPS * M[G:]
            got = v_ext.reshape(ny, nx, 2 * N)
            assert np.all(np.abs(got - want) <= tol), (nx, ny, float((np.abs(got - want) / tol).max()))
            pv, pt = SH.point_front(N, par, v_ext)
            assert PH.same(vpp, pv) and PH.same(tc, pt), (nx, ny)


# ------------------------------------------------------------------ the reference composer's grids
def test_golden_grid_grids():
    """GateVoltageComposer.do2d(x, x_min, x_max, nx, y, y_min, y_max, ny) of the reference with nx != ny on P x P, vP x vP,
    e x U, e x vP and U x vP pairs (non-adjacent and reversed dot pairs, the sensor gate, asymmetric and reversed ranges, N in
    {2, 4, 8}, one-row and one-column grids).  The composer holds the other gates at 0, renders "P" without matrix or origin
    and adds its origin once per vP axis, sqrt(2) times per U axis and never per e axis; the front end adds it once in the
    virtual frame, so the surplus (multiplicity - 1) origin is taken off the reference.  Gate part of v_ext within
    (G+1) eps (|VGM| |W| + |origin|) per element (the bound of test_golden_affine_grids; in the physical frame the matrix is
    the identity and the origin 0), same orientation (x along columns)."""
    from qadapt_hip.vec_env import scan_axis_vector
    z = np.load(os.path.join(ROOT, "tests", "golden", "grid_grids.npz"))
    n = int(z["n_cases"])
    assert n >= 12
    seen_N, shapes, kinds = set(), set(), set()
    for c in range(n):
        g = lambda k: z[f"c{c}_{k}"]     # noqa: E731
        N, nx, ny, xa, ya = int(g("n_dot")), int(g("nx")), int(g("ny")), str(g("x_axis")), str(g("y_axis"))
        assert nx != ny
        L = layout(N); G = N + 1
        seen_N.add(N); shapes.add((nx, ny))
        rg = g("ranges")
        pair = tuple(sorted((xa[0], ya[0])))
        kinds.add({("P", "P"): "P_x_P", ("v", "v"): "vP_x_vP", ("U", "e"): "e_x_U", ("e", "v"): "e_x_vP", ("U", "v"): "U_x_vP"}[pair])
        for a in (xa, ya):
            if a[0] in "eU":
                i, j = (int(t) for t in a[1:].split("_"))
                kinds |= {"nonadjacent"} if abs(i - j) > 1 else set()
                kinds |= {"reversed_pair"} if i > j else set()
            if a == f"P{N + 1}":
                kinds.add("sensor_gate")
        kinds |= {"reversed_range"} if rg[0] > rg[1] else set()
        kinds |= {"asymmetric"} if abs(rg[0] + rg[1]) > 1e-9 else set()
        mult = float(g("origin_multiplicity"))
        want_mult = sum({"P": 0.0, "e": 0.0, "U": np.sqrt(2.0), "v": 1.0}[a[0]] for a in (xa, ya))
        assert mult == want_mult
        physical = pair == ("P", "P")
        par = np.zeros(L.size); st = np.zeros(L.s_size)
        par[L.origin:L.origin + G] = g("origin")
        st = SH.query_state(N, st, np.zeros(N), np.zeros(N - 1), 0.0, g("vgm"))
        if physical:          # "P{g}" is the composer's physical gate g, 1-indexed, g = N+1 the sensor gate: control index g - 1
            dx, dy = (scan_axis_vector(int(a[1:]) - 1, N, "physical") for a in (xa, ya))
        else:
            dx, dy = scan_axis_vector(xa, N), scan_axis_vector(ya, N)
        v_ext, _, _ = GH.grid_voltages(N, par, st, dx, dy, rg, nx, ny, GH.PHYSICAL if physical else GH.VIRTUAL)
        got = v_ext[:, :G].reshape(ny, nx, G)
        W = GH.numpy_w(np.zeros(2 * N), dx, dy, rg, nx, ny)[:, :, :G]
        assert g("vg").shape == (ny, nx, G)
        if physical:
            ref = g("vg")
            bound = (G + 1) * EPS * np.abs(W)
        else:
            ref = g("vg") - (mult - 1.0) * g("origin")
            bound = (G + 1) * EPS * (np.abs(W) @ np.abs(g("vgm")).T + np.abs(g("origin")))
        worst = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
        print(f"[golden grids] case {c} N={N} {nx}x{ny} {xa} x {ya}: worst |diff| / bound {worst:.3f}")
        assert np.all(np.abs(got - ref) <= bound), (c, worst)
        # orientation: with the two axes swapped the grid is NOT within the bound
        if nx > 1 and ny > 1:
            wrong, _, _ = GH.grid_voltages(N, par, st, dy, dx, rg, nx, ny, GH.PHYSICAL if physical else GH.VIRTUAL)
            assert not np.all(np.abs(wrong[:, :G].reshape(ny, nx, G) - ref) <= bound), c
        assert PH.same(v_ext[:, G:], np.zeros((nx * ny, N - 1)))
    assert seen_N == {2, 4, 8}
    assert {(8, 1), (1, 8), (5, 3), (3, 5)} <= shapes
    assert kinds == {"P_x_P", "vP_x_vP", "e_x_U", "e_x_vP", "U_x_vP", "nonadjacent", "reversed_pair", "sensor_gate",
                     "reversed_range", "asymmetric"}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "grid_grids.npz")) < 64 * 1024


# ------------------------------------------------------------------ slot arithmetic and the inert tail
def test_grid_slot_arithmetic_and_inert_tail():
    """A grid of nx x ny points lives in the slot of a line of nx*ny points: Rl = ceil(sqrt(nx*ny)), record p = y*nx + x, the
    Rl^2 - nx*ny tail records the inert all-zero record, written over a 0xA5 fill; every point's record is not, and its vpp
    and tc are those of the front end.  (18, 5) and (10, 6) are the shapes of the GPU tier's latching test: Rl = 10 and 8, off
    nx, ny and the handles' R.  The descriptor is 4 + 4*8 doubles and four ints."""
    assert GH.grid_lib().qdhg_axes_bytes() == 8 * (4 + 4 * 8) + 16 == 304
    N = 4
    par, st, rng = _scene(N, 1960)
    dx, dy = rng.normal(0, 1, 2 * N), rng.normal(0, 1, 2 * N)
    rg = (-2.0, 3.0, 1.5, -0.5)
    off_vpp = 2 * 32 + 4 * 8 + 8                       # QdPixelRec: idx[32] uint16, fl[8] int32, nvalid, pad, then vpp[9], tc[7], E[32]
    want_side = {(1, 1): 1, (2, 1): 2, (5, 3): 4, (3, 5): 4, (8, 1): 3, (1, 8): 3, (18, 5): 10, (10, 6): 8, (16, 4): 8, (37, 3): 11,
                 (3, 21): 8, (1, 7): 3, (8, 8): 8}
    tails = 0
    for (nx, ny), side in want_side.items():
        n = nx * ny
        assert LH.slot(n)[0] == side and (side - 1) ** 2 < n <= side * side
        recs, live = GH.grid_records(N, par, st, dx, dy, rg, nx, ny)
        assert recs.shape == (side * side, off_vpp + 8 * (9 + 7 + 32))
        assert live[:n].all() and not live[n:].any() and int((~live).sum()) == side * side - n == LH.slot(n)[1]
        assert not recs[n:].any(), (nx, ny)                                    # the tail: all zero, written over the fill
        tails += side * side - n
        _, vpp, tc = GH.grid_voltages(N, par, st, dx, dy, rg, nx, ny)
        got = np.ascontiguousarray(recs[:n, off_vpp:off_vpp + 8 * 16]).view(np.float64).reshape(n, 16)
        assert PH.same(got[:, :N + 1], vpp) and PH.same(got[:, 9:9 + N - 1], tc)
        # record p = y*nx + x: the record of (row y, column x) is point x of the line through row y
        y = ny - 1
        sy = np.linspace(rg[2], rg[3], ny)[y]
        row = GH.grid_voltages(N, par, st, dx, dy, (rg[0], rg[1], sy, sy), nx, 1)
        assert PH.same(vpp[y * nx:(y + 1) * nx], row[1])
    assert tails > 0


# ------------------------------------------------------------------ the latching walk starts anew at every row
def _raster(N, n, rng):
    """(n, N) occupations along the raster in which ANY two points differ in one or two dots, by whole carriers (dot 0 counts
    the points, dot 1 flips at random): whatever state is held, a point differs from it in one or two dots, so with
    probability 0 of a transition every point but a row start is held"""
    occ = np.tile(rng.integers(0, 3, N).astype(float), (n, 1))
    occ[:, 0] += np.arange(n)
    occ[:, 1] += rng.integers(0, 2, n)
    return occ


@pytest.mark.parametrize("N", [2, 4])
def test_host_walk_resets_exactly_at_row_starts(N):
    """The walk of the grid's latching kernel (qd_grid_latch_row on rows of nx points, compiled for the host) on slots with a
    tail.  Probability 0: any two points differ in one or two dots, so every point is held EXCEPT those with
    p % nx == 0 -- the set of untouched points is exactly the row starts, and each row repeats its first point.  Probability
    0.5: the walk is oracle/qd_noise_oracle.py::latch_walk with R = nx bit for bit (the Philox counter of a point is
    y*nx + x); on the two larger shapes it holds at least 5 points and is none of the walks that reset every Rl, every 8 or
    12 (a handle's R) or never.  The tail of the slot is not touched.  nx = 1: no point is ever held."""
    L, G = layout(N), N + 1
    rng = np.random.default_rng(70 + N)
    for nx, ny in ((18, 5), (10, 6), (5, 3), (3, 5), (1, 8), (8, 1)):
        n, side = nx * ny, LH.slot(nx * ny)[0]
        SP = side * side
        occ = np.full((SP, N), 77.0); occ[:n] = _raster(N, n, rng)
        z = rng.normal(0, 1, SP)
        par = rng.normal(0, 0.3, L.size)
        s = NO.Stream(0x1234ABCD5678, 1000 + N, (1 << 63) | 5)
        par[L.pleads:L.pleads + N] = 0.0
        par[L.pinter:L.pinter + N * N] = 0.0
        got, zg = GH.latch_grid(N, par, occ, z, nx, ny, s)
        held = (got[:n] != occ[:n]).any(axis=1)
        assert np.array_equal(~held, np.arange(n) % nx == 0), (nx, ny)             # resets exactly at p % nx == 0
        assert PH.same(got[:n].reshape(ny, nx, N), np.repeat(occ[:n].reshape(ny, nx, N)[:, :1], nx, axis=1))
        assert PH.same(got[n:], occ[n:]) and PH.same(zg[n:], z[n:])                # the tail
        assert PH.same(zg[:n][~held], z[:n][~held]) and (nx == 1 or not np.array_equal(zg[:n][held], z[:n][held]))
        if nx == 1:
            assert not held.any()
        par[L.pleads:L.pleads + N] = 0.5
        par[L.pinter:L.pinter + N * N] = 0.5
        pl, pi = par[L.pleads:L.pleads + N], par[L.pinter:L.pinter + N * N].reshape(N, N)
        got, zg = GH.latch_grid(N, par, occ, z, nx, ny, s)
        ref = NO.latch_walk(s, 0, occ[:n], nx, pl, pi)
        assert PH.same(got[:n], ref), (nx, ny)
        assert PH.same(got[n:], occ[n:]) and PH.same(zg[n:], z[n:])
        if n >= 60:                                      # (the walks of a small grid may coincide by chance)
            assert int((ref != occ[:n]).any(axis=1).sum()) >= 5
            for other in (side, 12, 8, n):
                if other != nx:
                    assert not PH.same(NO.latch_walk(s, 0, occ[:n], other, pl, pi), ref), (nx, ny, other)
    assert GH.grid_lib().qdhg_latch_grid(N, None, None, None, 0, 1, 0, 0, 0, 0) == 1


# ------------------------------------------------------------------ the sanitizer run of the host harness
def test_grid_front_end_under_the_sanitizers():
    """tests/hosttest_grid/qd_grid_asan: a program of its own (nothing is loaded into Python), built with
    -fsanitize=address,undefined, that walks qd_grid_record over slots with a tail in heap buffers of exactly Rl*Rl records,
    with the descriptor on the heap, and the latching rows over buffers of exactly nx*ny points."""
    hdir = os.path.join(ROOT, "tests", "hosttest_grid")
    subprocess.check_call(["make", "-s", "-C", hdir, "qd_grid_asan"])
    r = subprocess.run([os.path.join(hdir, "qd_grid_asan")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "grid asan ok" in r.stdout


# ------------------------------------------------------------------ the axis resolver
def test_scan_grid_axis_resolver():
    """scan_grid resolves its two axes as scan_affine does: (nq, 2, 2N) of dx then dy"""
    from qadapt_hip.vec_env import scan_axis_vector as vec, scan_axis_vectors as vecs
    N = 4
    dirs = np.stack([vecs("e1_2", N, "virtual", 3), vecs(["vP2", {"vP1": 1.0, "B2": -0.5}, 4], N, "virtual", 3)], axis=1)
    assert dirs.shape == (3, 2, 8)
    assert dirs[0, 0].tolist() == [1, -1, 0, 0, 0, 0, 0, 0] and dirs[2, 0].tolist() == dirs[0, 0].tolist()
    assert dirs[0, 1].tolist() == vec("vP2", N).tolist() and dirs[1, 1].tolist() == [1, 0, 0, 0, 0, 0, -0.5, 0]
    assert dirs[2, 1].tolist() == vec("S", N).tolist()
    assert vecs("P3", N, "physical", 1).tolist() == [[0, 0, 1, 0, 0, 0, 0, 0]]
    with pytest.raises(ValueError, match="physical frame"):
        vecs("P3", N, "virtual", 1)
    with pytest.raises(ValueError):
        vecs(["vP1", "vP2"], N, "virtual", 3)
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    sig = inspect.signature(VecQuantumDeviceEnv.scan_grid).parameters
    assert list(sig)[:11] == ["self", "env_ids", "x", "y", "x_range", "y_range", "nx", "ny", "gate_voltages", "barrier_voltages",
                              "sensor_voltage"]
    kw = ["frame", "vgm", "gamma", "noise", "serial", "stream_base", "occupations"]
    assert list(sig)[11:] == kw and all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in kw)


# ------------------------------------------------------------------ C ABI without a GPU
def _built_lib():
    from qadapt_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is missing: run __graft_entry__.build() before the tests (no test compiles it)")
    return _lib, _lib.lib()


def test_scan_grid_symbol_and_prototype():
    _lib, L = _built_lib()
    assert "qd_scan_grid" in _lib.EXPORTS and hasattr(L, "qd_scan_grid")
    at = L.qd_scan_grid.argtypes
    assert len(at) == 15 and all(at[i] is ctypes.c_int for i in (2, 3, 4)) and L.qd_scan_grid.restype is ctypes.c_int
    assert at[13]._type_ is _lib.QdScanGridOpts and ctypes.sizeof(_lib.QdScanGridOpts) == 56
    assert [f[0] for f in _lib.QdScanGridOpts._fields_] == [f[0] for f in _lib.QdScanAffineOpts._fields_]
    hdr = open(os.path.join(ROOT, "include", "qdsim.h")).read()
    assert "int qd_scan_grid(qd_handle* h, const int32_t* env_of_query_dev, int nq, int nx, int ny, const double* dir_dev," in hdr
    assert "} qd_scan_grid_opts;" in hdr and f"#define QD_GRID_SLOTS {_lib.QD_GRID_SLOTS}" in hdr and _lib.QD_GRID_SLOTS == 4096
    # the contracts and the stream rule are stated, and what is still not built is named
    doc = hdr[hdr.index("Stateless 2-D scans on any nx x ny GRID"):hdr.index("#define QD_GRID_SLOTS")]
    for phrase in ("qd_scan_affine with the same arguments", "equals qd_scan1d", "equals qd_eval_points", "belong on the stream",
                   "Grids of more than P points", "different shapes within one call", "tile search on a rectangular slot",
                   "radial noise"):
        assert phrase in doc, phrase
    assert "Rx != Ry are" not in hdr.replace("\n *", "")
    # the siblings and their options are untouched
    assert ctypes.sizeof(_lib.QdScanOpts) == 56 and ctypes.sizeof(_lib.QdScanAffineOpts) == 56 and ctypes.sizeof(_lib.QdScan1dOpts) == 56
    assert L.qd_scan_grid(None, None, 1, 1, 1, None, None, None, None, None, None, None, None, None, None) == _lib.QD_ERR_ARG   # no crash


def _handle(L, N, R, B, flags=0, qconfig=None):
    from qadapt_hip.vec_env import make_qd_config
    cfg = make_qd_config(DM.load_yaml(None, "env_config.yaml"), qconfig or DM.load_yaml(None, "qarray_config.yaml"), N, R, B,
                         flags=flags)
    h = ctypes.c_void_p()
    L.qd_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    if not h:
        pytest.fail("qd_create handed out no handle")
    return h


def test_scan_grid_argument_checks_need_no_device():
    """Without a GPU qd_create fails with QD_ERR_HIP and still hands out the partial handle (qdsim.h), which is all these
    checks need: each returns before anything touches the device."""
    _lib, L = _built_lib()
    B, R = 3, 8
    h = _handle(L, 4, R, B)
    one = ctypes.c_void_p(64)                      # a device pointer that is never dereferenced

    def opts(**kw):
        o = _lib.QdScanGridOpts(struct_size=ctypes.sizeof(_lib.QdScanGridOpts))
        for k, v in kw.items():
            setattr(o, k, v)
        return ctypes.byref(o)

    def call(hh=h, env=one, nq=1, nx=5, ny=3, dirs=one, rng=one, gv=one, bv=one, o=None):
        return L.qd_scan_grid(hh, env, nq, nx, ny, dirs, rng, gv, bv, None, one, None, None, o, None)

    try:
        assert call(env=None) == _lib.QD_ERR_ARG and b"env_of_query_dev" in L.qd_last_error(h)
        assert call(dirs=None) == _lib.QD_ERR_ARG and b"dir_dev" in L.qd_last_error(h)
        assert call(rng=None) == _lib.QD_ERR_ARG and b"range_dev" in L.qd_last_error(h)
        assert call(gv=None) == _lib.QD_ERR_ARG and b"gate_v_dev" in L.qd_last_error(h)
        assert call(bv=None) == _lib.QD_ERR_ARG and b"barrier_v_dev" in L.qd_last_error(h)
        assert call(nq=-1) == _lib.QD_ERR_ARG and b"nq < 0" in L.qd_last_error(h)
        for nx, ny in ((0, 3), (3, 0), (-1, 4), (4, -1), (-4, -4), (R * R + 1, 1), (1, R * R + 1), (R + 1, R), (R, R + 1),
                       (65536, 65536), (2 ** 30, 4)):
            assert call(nx=nx, ny=ny) == _lib.QD_ERR_ARG and b"nx*ny <= P" in L.qd_last_error(h), (nx, ny)
            assert call(nx=nx, ny=ny, nq=0) == _lib.QD_ERR_ARG                  # the argument checks come before "nothing to do"
        assert call(o=opts(struct_size=8)) == _lib.QD_ERR_ARG and b"struct_size" in L.qd_last_error(h)
        assert call(o=opts(frame=2)) == _lib.QD_ERR_ARG and b"frame" in L.qd_last_error(h)
        assert call(o=opts(frame=-1)) == _lib.QD_ERR_ARG
        assert call(o=opts(frame=_lib.QD_SCAN_PHYSICAL, vgm_dev=64)) == _lib.QD_ERR_ARG and b"vgm_dev" in L.qd_last_error(h)
        assert call(o=opts(noise_flags=_lib.QD_NOISE_RADIAL)) == _lib.QD_ERR_ARG and b"radial" in L.qd_last_error(h)
        assert call(o=opts(noise_flags=_lib.QD_NOISE_SENSOR | _lib.QD_NOISE_RADIAL)) == _lib.QD_ERR_ARG
        assert call(o=opts(noise_flags=8)) == _lib.QD_ERR_ARG
        assert b"qd_scan_grid" in L.qd_last_error(h)
        for nx, ny in ((1, 1), (R, R), (R * R, 1), (1, R * R), (2 * R, R // 2)):
            assert call(nq=0, nx=nx, ny=ny) == 0
        assert call(nq=0, o=opts(noise_flags=_lib.QD_NOISE_SENSOR | _lib.QD_NOISE_LATCH)) == 0
    finally:
        L.qd_destroy(h)
    hv = _handle(L, 4, R, B, flags=_lib.QD_FLAG_VALIDATE)
    try:
        assert call(hh=hv) == _lib.QD_ERR_STATE and b"QD_FLAG_VALIDATE" in L.qd_last_error(hv)
        assert call(hh=hv, nq=0) == _lib.QD_ERR_STATE
        assert call(hh=hv, dirs=None) == _lib.QD_ERR_ARG                 # the argument checks come first
        assert call(hh=hv, nx=0) == _lib.QD_ERR_ARG and call(hh=hv, ny=R * R + 1) == _lib.QD_ERR_ARG
        assert call(hh=hv, o=opts(noise_flags=_lib.QD_NOISE_RADIAL)) == _lib.QD_ERR_ARG
    finally:
        L.qd_destroy(hv)
    from qadapt_hip.vec_env import override_charge_states
    q = override_charge_states(DM.load_yaml(None, "qarray_config.yaml"), "all")
    q["simulator"]["model"]["max_charge_carriers"] = 2
    hf = _handle(L, 3, R, B, qconfig=q)
    try:
        assert call(hh=hf) == _lib.QD_ERR_STATE and b"full charge-state space" in L.qd_last_error(hf)
        assert call(hh=hf, nx=0) == _lib.QD_ERR_ARG
    finally:
        L.qd_destroy(hf)


# ------------------------------------------------------------------ the facades on a stub backend
class StubBackend:
    """Shape-faithful stand-in for VecQuantumDeviceEnv with B = 1 that records its scan_grid calls."""

    def __init__(self, N, R):
        self.N, self.R = N, R
        self.calls = []

    def _obs(self):
        N, R = self.N, self.R
        return {"image": np.zeros((1, R, R, N - 1), np.float32), "obs_gate_voltages": np.zeros((1, N), np.float32),
                "obs_barrier_voltages": np.zeros((1, N - 1), np.float32)}

    def reset(self, seed=None, **kw):
        return self._obs()

    def device_state(self):
        N = self.N
        return {"gate_ground_truth": np.ones((1, N), np.float32), "barrier_ground_truth": np.zeros((1, N - 1), np.float32),
                "sensor_ground_truth": np.array([0.5]), "current_gate_voltages": np.full((1, N), 2.0),
                "current_barrier_voltages": np.full((1, N - 1), 3.0),
                "virtual_gate_matrix": -np.eye(N + 1)[None], "virtual_gate_origin": np.zeros((1, N + 1))}

    def scan_grid(self, env_ids, x, y, x_range, y_range, nx, ny, gate_voltages, barrier_voltages, sensor_voltage=None, **kw):
        self.calls.append(dict(env_ids=list(env_ids), x=x, y=y, x_range=tuple(x_range), y_range=tuple(y_range), nx=nx, ny=ny,
                               gv=np.array(gate_voltages), bv=np.array(barrier_voltages), sv=sensor_voltage, kw=kw))
        nx, ny = int(nx), int(ny)
        out = {"raw": np.arange(nx * ny, dtype=np.float64).reshape(1, ny, nx), "image": np.zeros((1, ny, nx), np.float32),
               "plohi": np.array([[0.0, 1.0]])}
        if kw.get("occupations"):
            out["occupations"] = np.arange(nx * ny * self.N, dtype=np.float64).reshape(1, ny, nx, self.N)
        return out


def _stub_env(tmp_path, N, R):
    cfg = DM.load_yaml(None, "env_config.yaml")
    cfg["capacitance_model"]["update_method"] = None
    cfg["simulator"].update(num_dots=N, resolution=R)
    p = tmp_path / "env.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return QuantumDeviceEnv(config_path=str(p), backend=StubBackend(N, R))


def test_array_scan_grid_mirror(tmp_path):
    N, R = 4, 6
    env = _stub_env(tmp_path, N, R)
    gv, bv = np.array([1.0, -2.0, 3.0, 4.5]), np.array([0.1, 0.2, 0.3])
    out = env.array.scan_grid("e1_2", "B1", (-1, 1), (0, 2), 9, 4, gv, bv, occupations=True, frame="virtual")
    assert out["raw"].shape == (4, 9) and out["raw"].dtype == np.float64 and out["occupations"].shape == (4, 9, N)
    assert out["image"].shape == (4, 9) and out["image"].dtype == np.float32 and out["plohi"].shape == (2,)
    c = env._b.calls[-1]
    assert (c["x"], c["y"], c["env_ids"], c["sv"], c["nx"], c["ny"]) == ("e1_2", "B1", [0], None, 9, 4)
    assert c["x_range"] == (-1, 1) and c["y_range"] == (0, 2) and c["kw"] == {"occupations": True, "frame": "virtual"}
    assert c["gv"].shape == (1, N) and c["bv"].shape == (1, N - 1) and np.array_equal(c["gv"][0], gv) and np.array_equal(c["bv"][0], bv)
    d = {"vP1": 1.0, "B1": -0.3}
    out = env.array.scan_grid(d, 2, (2, 0), (1, 1), 1, 7, gv, bv, 0.25, noise=("sensor", "latch"))
    c = env._b.calls[-1]
    assert c["x"] is d and c["y"] == 2 and c["sv"] == 0.25 and c["x_range"] == (2, 0) and c["kw"] == {"noise": ("sensor", "latch")}
    assert set(out) == {"raw", "image", "plohi"} and out["raw"].shape == (7, 1)
    assert env.current_step == 0


def test_model_do2d_open_facade(tmp_path):
    """The reference's gate grammar on both axes: an int and "P{g}" sweep physical gate g (control g - 1, g = N + 1 the sensor
    gate), "vP", "e" and "U" go through as names; two physical gates render in the physical frame, two virtual axes in the
    virtual frame, a mixed pair is refused: one call has one frame.  The base point is zero, the grid noise-free, the peak
    width the model's, and the result (signal (y_points, x_points, 1), n_open (y_points, x_points, N))."""
    N, R = 4, 8
    env = _stub_env(tmp_path, N, R)
    m = env.array.model
    m.coulomb_peak_width = 0.125
    for xg, yg, xa, ya, frame in ((2, "P3", 1, 2, "physical"), ("P1", N + 1, 0, N, "physical"), (np.int64(1), f"P{N + 1}", 0, N, "physical"),
                                  ("vP2", "vP3", "vP2", "vP3", "virtual"), ("e1_3", "U1_3", "e1_3", "U1_3", "virtual"),
                                  ("U4_2", "vP1", "U4_2", "vP1", "virtual"), ("vP4", "e2_1", "vP4", "e2_1", "virtual")):
        sig, occ = m.do2d_open(xg, -1.5, 2.5, 9, yg, 0.5, -0.25, 4)
        c = env._b.calls[-1]
        assert c["x"] == xa and c["y"] == ya and c["kw"] == {"frame": frame, "gamma": 0.125, "occupations": True}, (xg, yg)
        assert c["x_range"] == (-1.5, 2.5) and c["y_range"] == (0.5, -0.25) and (c["nx"], c["ny"]) == (9, 4)
        assert c["env_ids"] == [0] and c["sv"] == 0.0
        assert c["gv"].shape == (1, N) and not c["gv"].any() and c["bv"].shape == (1, N - 1) and not c["bv"].any()
        assert sig.shape == (4, 9, 1) and sig.dtype == np.float64 and np.array_equal(sig[:, :, 0], np.arange(36.0).reshape(4, 9))
        assert occ.shape == (4, 9, N) and occ.dtype == np.float64 and np.array_equal(occ, np.arange(36.0 * N).reshape(4, 9, N))
    m.coulomb_peak_width = None
    m.do2d_open("vP1", 0, 1, 3, "vP2", 0, 1, 2)
    assert env._b.calls[-1]["kw"]["gamma"] is None
    ncalls = len(env._b.calls)
    for xg, yg in (("P1", "vP2"), ("vP1", "P2"), (1, "e1_2"), ("U1_2", N + 1), ("P1", "U2_3")):
        with pytest.raises(NotImplementedError, match="one call has one frame"):
            m.do2d_open(xg, 0, 1, 3, yg, 0, 1, 3)
    for bad in (0, N + 2, "P0", f"P{N + 2}", "B1", "S", "x", "", 1.5, None, True):
        with pytest.raises(ValueError):
            m.do2d_open(bad, 0, 1, 3, "vP1", 0, 1, 3)
        with pytest.raises(ValueError):
            m.do2d_open("vP1", 0, 1, 3, bad, 0, 1, 3)
    assert len(env._b.calls) == ncalls                   # a refused pair reaches no backend
    doc = type(m).do2d_open.__doc__
    assert "sqrt(2)" in doc and "origin" in doc and "ONCE" in doc and "one call has one frame" in " ".join(doc.split()).lower()
    # do1d_open keeps its grammar and its words
    assert "ONCE" in type(m).do1d_open.__doc__
    assert env.current_step == 0


def test_scan_grid_checks_its_counts_before_the_library(monkeypatch):
    """nx, ny outside 1.. or nx*ny > R*R and radial noise are ValueErrors raised before anything reaches the library: the
    method runs on an object that has no handle and no library at all."""
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    env = object.__new__(VecQuantumDeviceEnv)
    env.N, env.C, env.R = 4, 3, 8
    gv, bv = np.zeros((1, 4)), np.zeros((1, 3))
    for nx, ny in ((0, 3), (3, 0), (-2, 2), (65, 1), (1, 65), (9, 8), (8, 9)):
        with pytest.raises(ValueError, match="nx"):
            env.scan_grid([0], "vP1", "vP2", (0, 1), (0, 1), nx, ny, gv, bv)
    with pytest.raises(ValueError, match="frame"):
        env.scan_grid([0], "vP1", "vP2", (0, 1), (0, 1), 4, 4, gv, bv, frame="other")
    with pytest.raises(ValueError, match="vgm"):
        env.scan_grid([0], "P1", "P2", (0, 1), (0, 1), 4, 4, gv, bv, frame="physical", vgm=np.eye(5)[None])
