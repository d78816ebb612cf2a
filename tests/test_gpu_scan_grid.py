"""Grids of nx x ny points on the MI355X (run with -m gpu): qd_scan_grid against qd_scan_affine at nx = ny = R, against qd_scan1d at
ny = 1 and against qd_eval_points at rectangular shapes, the latching walk that starts anew at every row against the noise
oracle, NumPy-built grids against the oracle, percentiles and image, the launch chunking with guard rows and inert queries, the
absent footprint on a noisy auto-resetting run and beside qd_scan1d on the shared buffers, and the refusals."""
import ctypes

import numpy as np
import pytest
import yaml

import affine_helpers as AH
import grid_helpers as GH
import helpers as H
import line_helpers as LH
import points_helpers as PH
import qd_noise_oracle as NO
import qd_oracle as O
import scan_helpers as SH
from qadapt_hip import device_model as DM
from qadapt_hip.layout import layout

pytestmark = pytest.mark.gpu


def _cfg(tmp_path, **sim):
    cfg = DM.load_yaml(None, "env_config.yaml")
    cfg["capacitance_model"]["update_method"] = None          # deterministic physics, no CNN in the loop
    cfg["simulator"].update(sim)
    p = tmp_path / "env.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def _vec(tmp_path, B, N, R, seed, **kw):
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    if "config_path" not in kw:
        kw["config_path"] = _cfg(tmp_path)
    return VecQuantumDeviceEnv(B, num_dots=N, resolution=R, seed=seed, **kw)


def _load(env, params, state):
    """these parameter and state blocks as the handle's devices"""
    from qadapt_hip import _lib
    ids = np.arange(env.B, dtype=np.int32)
    rc = env._lib.qd_load_episodes(env._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), env.B,
                                   np.ascontiguousarray(params).ctypes.data, np.ascontiguousarray(state).ctypes.data, 0,
                                   env._stream())
    _lib.check(env._h, rc, "qd_load_episodes")
    env._params_host[:] = params
    env._needs_reset = False


def _placed(env, N, seed, modes):
    env.load_new_devices(seed=seed)
    st, steps = env.get_state()
    rng = np.random.default_rng(seed)
    for e, mode in enumerate(modes):
        st[e] = H.place(N, st[e], mode, rng)
        st[e, layout(N).s_sensor_gt] += rng.uniform(-0.3, 0.3)
    env.set_state(st, steps)
    return st


def _volts(N, st):
    L = layout(N)
    return st[:, L.s_gate_v:L.s_gate_v + N], st[:, L.s_barrier_v:L.s_barrier_v + N - 1], st[:, L.s_sensor_gt]


def _physical_point(N, st, par):
    """the env's physical working point VGM [gate_v, sensor] + origin"""
    L = layout(N); G = N + 1
    vgm = st[L.s_vgm:L.s_vgm + G * G].reshape(G, G)
    return vgm @ np.concatenate([st[L.s_gate_v:L.s_gate_v + N], [st[L.s_sensor_gt]]]) + par[L.origin:L.origin + G]


def _dense(N, rng):
    """a dense direction: normal coefficients, the sensor component x0.1 and the barrier components x0.5"""
    d = rng.normal(size=2 * N)
    d[N] *= 0.1
    d[N + 1:] *= 0.5
    return d


def _np(t):
    return t.cpu().numpy()


def _fr(frame):
    return GH.PHYSICAL if frame == "physical" else GH.VIRTUAL


# ------------------------------------------------------------------ scenes with latching, fixed on the CPU
LATCH_SEED, LATCH_SERIAL, LATCH_BASE = 9200, (1 << 63) | 91, 4321


def _latch_scene(N, nx, ny, seed, x, y, rgx, rgy, p_lead=0.15, p_inter=0.15, st=None, par=None):
    """One device of `seed` "near" its ground truth (vgm_noise 0) whose parameter block latches often (every p_leads and p_inter
    entry set to the given probabilities); a virtual-frame grid of nx x ny points along (x, y) from the env's own voltages; the
    oracle's clean occupations there, (ny*nx, N).  CPU only."""
    from qadapt_hip.vec_env import scan_axis_vector
    L, G = layout(N), N + 1
    if par is None:
        eb = H.sample_blocks(N, [seed])
        rng = np.random.default_rng(seed)
        par, st = eb.params[0].copy(), H.place(N, eb.state[0], "near", rng, vgm_noise=0.0)
        par[L.pleads:L.pleads + N] = p_lead
        par[L.pinter:L.pinter + N * N] = p_inter
    dx, dy = scan_axis_vector(x, N), scan_axis_vector(y, N)
    grid = GH.numpy_grid(N, st, par[L.origin:L.origin + G], dx, dy, [*rgx, *rgy], nx, ny).reshape(nx * ny, 2 * N)
    occ = O.ground_state_open(H.dev_view(N, par), grid[:, :G], grid[:, G:])
    return par, st, dx, dy, occ


def _walk(par, N, occ, R, q, seed):
    """the oracle's latching walk of query q on occupations occ (n, N) with rows of R"""
    L = layout(N)
    s = NO.Stream(seed, LATCH_BASE + q, LATCH_SERIAL)
    return NO.latch_walk(s, 0, occ, R, par[L.pleads:L.pleads + N], par[L.pinter:L.pinter + N * N].reshape(N, N))


# ------------------------------------------------------------------ 1. a grid of R x R = an affine scan
@pytest.mark.parametrize("N,K", [(2, 8), (2, 32), (4, 8), (4, 32)])
def test_square_grid_equals_the_affine_scan(tmp_path, N, K):
    """pixel_search handle, nx = ny = R = 8: raw, occupations, percentiles and image of the grid have the bits of scan_affine with
    the same arguments, deterministically and with sensor noise and latching under the same serial and stream base -- Rl = R, so
    point indices, telegraph chain and row walks coincide.  Two queries on one env: e1_2 against vP_N, and a dense direction
    against a barrier downwards.  Fixed on the CPU beforehand with the oracle: at least one point of each noisy grid is held."""
    from qadapt_hip.vec_env import scan_axis_vector as vec
    R = 8
    seed = LATCH_SEED + 10 * N
    rng = np.random.default_rng(seed)
    xs, ys = ["e1_2", _dense(N, rng)], [f"vP{N}", "B1"]
    rgx, rgy = [(-6.0, 6.0), (7.0, -6.0)], [(-1.0, 1.5), (2.0, -2.0)]
    par, st, _, _, _ = _latch_scene(N, R, R, seed, xs[0], ys[0], rgx[0], rgy[0])
    for q in range(2):
        _, _, _, _, occ = _latch_scene(N, R, R, seed, xs[q], ys[q], rgx[q], rgy[q], st=st, par=par)
        held = int((_walk(par, N, occ, R, q, seed) != occ).any(axis=1).sum())
        assert held > 0, f"the oracle holds no point of grid {q}"
    env = _vec(tmp_path, 1, N, R, seed, pixel_search=True, num_charge_states=K)
    _load(env, par[None], st[None])
    gv, bv, sv = _volts(N, st[None])
    ids = [0, 0]
    dxs, dys = np.stack([vec(a, N) for a in xs]), np.stack([vec(a, N) for a in ys])
    for kw in (dict(), dict(noise=("sensor", "latch"), serial=LATCH_SERIAL, stream_base=LATCH_BASE)):
        grid = env.scan_grid(ids, dxs, dys, rgx, rgy, R, R, gv[ids], bv[ids], sv[ids], occupations=True, **kw)
        img = env.scan_affine(ids, dxs, dys, rgx, rgy, gv[ids], bv[ids], sensor_voltage=sv[ids], occupations=True, normalised=True, **kw)
        assert grid["raw"].shape == (2, R, R) and grid["occupations"].shape == (2, R, R, N)
        for key in ("raw", "occupations", "plohi", "image"):
            a, b = _np(grid[key]), _np(img[key])
            assert a.shape == b.shape and a.dtype == b.dtype and np.isfinite(a).all()
            assert PH.same(a, b), ("noise" in kw, key, int((a != b).sum()))
        if kw:
            clean = env.scan_grid(ids, dxs, dys, rgx, rgy, R, R, gv[ids], bv[ids], sv[ids], occupations=True)
            assert not PH.same(clean["raw"], grid["raw"])                          # the noise really ran
            held = (_np(clean["occupations"]) != _np(grid["occupations"])).any(axis=3).reshape(2, -1)
            print(f"[grid vs affine] N={N} K={K}: held points per grid {held.sum(axis=1).tolist()}")
            assert held.any(axis=1).all()
    env.close()


# ------------------------------------------------------------------ 2. a grid of one row = a line
@pytest.mark.parametrize("nx", [1, 37, 64])
def test_one_row_grid_equals_the_line(tmp_path, nx):
    """ny = 1, dy = 0 on a 4-dot 8 x 8 handle: raw, image, percentiles and occupations have the bits of scan1d(n_points = nx, d = dx,
    [lo, hi] = x_range), deterministically and with sensor noise and latching under the same serial and stream base.  The y range
    is finite and arbitrary.  Three queries: e1_2 on a device that latches often, a dense direction downwards, a plunger."""
    from qadapt_hip.vec_env import scan_axis_vector as vec
    N, R = 4, 8
    seed = LATCH_SEED + 100
    par, st, _, _, _ = _latch_scene(N, nx, 1, seed, "e1_2", "vP1", (-6.0, 6.0), (0.0, 0.0))
    env = _vec(tmp_path, 1, N, R, seed)
    _load(env, par[None], st[None])
    gv, bv, sv = _volts(N, st[None])
    ids = [0, 0, 0]
    dxs = np.stack([vec("e1_2", N), _dense(N, np.random.default_rng(seed)), vec(f"vP{N}", N)])
    rgx = [(-6.0, 6.0), (3.0, -2.5), (-4.0, 4.0)]
    for kw in (dict(), dict(noise=("sensor", "latch"), serial=LATCH_SERIAL, stream_base=LATCH_BASE)):
        grid = env.scan_grid(ids, dxs, np.zeros_like(dxs), rgx, (11.0, -2.0), nx, 1, gv[ids], bv[ids], sv[ids], occupations=True, **kw)
        line = env.scan1d(ids, dxs, rgx, nx, gv[ids], bv[ids], sv[ids], occupations=True, **kw)
        assert grid["raw"].shape == (3, 1, nx) and grid["image"].shape == (3, 1, nx) and grid["occupations"].shape == (3, 1, nx, N)
        for key in ("raw", "image", "occupations"):
            a, b = _np(grid[key])[:, 0], _np(line[key])
            assert np.isfinite(a).all() and PH.same(a, b), ("noise" in kw, key, int((a != b).sum()))
        assert PH.same(grid["plohi"], line["plohi"])
        if kw and nx > 1:
            clean = env.scan_grid(ids, dxs, np.zeros_like(dxs), rgx, (11.0, -2.0), nx, 1, gv[ids], bv[ids], sv[ids], occupations=True)
            assert not PH.same(clean["raw"], grid["raw"])
            assert (_np(clean["occupations"])[0] != _np(grid["occupations"])[0]).any()       # the e1_2 line holds a point
    env.close()


# ------------------------------------------------------------------ 3. grids = points
def _grid_queries(N, st, par, seed):
    """(x, y, x_range, y_range, frame, base W0, vgm or None, gamma or None, numpy) per query; `numpy` marks the queries whose
    voltages NumPy builds with the bits of the front end: two physical unit axes with 0 at the swept controls of the base point
    (fma(sx, 1, 0) = sx and fma(sy, 0, w) = w are exact, and np.linspace rounds as qd_linspace does).  The others take the
    voltages of the host front end (tests/hosttest_grid)."""
    L, G = layout(N), N + 1
    gv = st[L.s_gate_v:L.s_gate_v + N]; bvv = st[L.s_barrier_v:L.s_barrier_v + N - 1]; sv = st[L.s_sensor_gt]
    virt = np.concatenate([gv, [sv], bvv])
    phys = np.concatenate([_physical_point(N, st, par), bvv])
    swept = phys.copy(); swept[0] = 0.0; swept[G] = 0.0
    rng = np.random.default_rng(seed)
    vgm = -np.eye(G) + rng.normal(0, 0.05, (G, G))
    return [("P1", "B1", (phys[0] - 2.0, phys[0] + 2.5), (phys[G] + 1.0, phys[G] - 1.0), "physical", swept, None, None, True),
            ("e1_2", f"vP{N}", (-1.5, 1.5), (-2.0, 2.5), "virtual", virt, vgm, None, False),
            (_dense(N, rng), {"P1": 0.5, "B1": -1.0}, (1.6, -0.8), (-1.0, 2.0), "physical", phys, None, None, False),
            ("U1_2", _dense(N, rng), (-1.2, 1.2), (0.4, -0.9), "virtual", virt, None, 0.7 * par[L.scal + 1], False)]


@pytest.mark.parametrize("N,K,nx,ny", [(4, 32, 5, 3), (2, 20, 16, 4), (4, 20, 3, 21), (2, 32, 1, 7)])
def test_grids_equal_points(tmp_path, N, K, nx, ny):
    """A default and a pixel_search handle of 8 x 8, envs "near" and "mid": the raw signal of a grid over two physical unit axes has
    the bits of eval_points(signal) at voltages built in NumPy (np.linspace and nothing else); over e1_2 x vP_N under a matrix
    override, a dense direction against a dict axis in the physical frame and U1_2 against a dense direction downwards with
    an explicit gamma, at the v_ext of the host front end.  The occupations have the bits of eval_points(occupations) for
    K = 20; for K = 32 the points solve the occupations from the reference order and the grid from the search order: rtol 1e-9,
    atol 1e-12, the rule of test_lines_equal_points.  (5, 3) and (1, 7) leave a tail of 1 and 2 inert records, (16, 4) fills the
    slot of the handle, (3, 21) is one point short of it."""
    from qadapt_hip.vec_env import scan_axis_vector as vec
    B, G, R = 2, N + 1, 8
    seed = 9100 + 10 * N + K
    n = nx * ny
    for pixel_search in (False, True):
        env = _vec(tmp_path, B, N, R, seed, num_charge_states=K, pixel_search=pixel_search)
        st = _placed(env, N, seed, ("near", "mid"))
        frames = set()
        for e in range(B):
            par = env._params_host[e]
            for x, y, rgx, rgy, frame, W0, vgm, gamma, numpy_built in _grid_queries(N, st[e], par, seed + 1 + e):
                out = env.scan_grid([e], x, y, rgx, rgy, nx, ny, W0[None, :N], W0[None, G:], W0[N], frame=frame, occupations=True,
                                    vgm=None if vgm is None else vgm[None], gamma=gamma)
                if numpy_built:
                    v_ext = np.tile(W0, (ny, nx, 1))
                    v_ext[:, :, 0] = np.linspace(rgx[0], rgx[1], nx)[None, :]
                    v_ext[:, :, G] = np.linspace(rgy[0], rgy[1], ny)[:, None]
                    v_ext = v_ext.reshape(n, 2 * N)
                else:
                    qst = SH.query_state(N, st[e], W0[:N], W0[G:], float(W0[N]), vgm)
                    v_ext, _, _ = GH.grid_voltages(N, par, qst, vec(x, N, frame), vec(y, N, frame), [*rgx, *rgy], nx, ny, _fr(frame))
                pts = env.eval_points([e], v_ext[None, :, :G], v_ext[None, :, G:], gamma=gamma)
                raw, occ = _np(out["raw"])[0], _np(out["occupations"])[0]
                sig, occ_pts = _np(pts["signal"])[0].reshape(ny, nx), _np(pts["occupations"])[0].reshape(ny, nx, N)
                tag = (pixel_search, e, x if isinstance(x, str) else "dense", frame, vgm is not None, gamma is not None)
                frames.add(frame)
                assert raw.shape == (ny, nx) and occ.shape == (ny, nx, N) and np.isfinite(raw).all() and np.ptp(raw) > 0, tag
                d = float(np.abs(raw - sig).max()); do = float(np.abs(occ - occ_pts).max())
                print(f"[grid vs points] N={N} K={K} {nx}x{ny} {tag}: raw diff {d:.3e}, occupation diff {do:.3e}")
                assert PH.same(raw, sig), (tag, d)
                if K in (8, 16, 32):
                    assert np.allclose(occ, occ_pts, rtol=1e-9, atol=1e-12), (tag, do)
                else:
                    assert PH.same(occ, occ_pts), (tag, do)
        assert frames == {"virtual", "physical"}
        env.close()


# ------------------------------------------------------------------ 4. the walk starts anew at every row
# (nx, ny): (N, R of the handle, device seed, x range); chosen on the CPU so that the oracle tells the four walks apart (on most
# 4-dot scenes the points on either side of a row start differ in three or more dots, where every walk accepts)
LATCH_ROWS = {(18, 5): (2, 12, LATCH_SEED + 52, (-20.0, 20.0)), (10, 6): (4, 8, LATCH_SEED + 55, (-6.0, 6.0))}


def _latch_rows_scene(nx, ny):
    N, R, seed, rgx = LATCH_ROWS[(nx, ny)]
    x, y, rgy = "e1_2", "U1_2", (-1.5, 1.5)
    par, st, dx, dy, occ = _latch_scene(N, nx, ny, seed, x, y, rgx, rgy, p_lead=0.08, p_inter=0.08)
    return N, R, seed, x, y, rgx, rgy, par, st, dx, dy, occ


@pytest.mark.parametrize("nx,ny", [(18, 5), (10, 6)])
def test_latching_resets_at_every_row_start(tmp_path, nx, ny):
    """(18, 5) on a 2-dot 12 x 12 handle: the slot side Rl = 10 differs from nx, ny and R; (10, 6) on a 4-dot 8 x 8 handle: Rl = 8 =
    R.  With LATCH alone the occupations are, bit for bit, qd_noise_oracle.latch_walk(stream, 0, occ_clean, nx, ...) on the clean
    occupations of a deterministic run of the same query -- rows of nx points, the Philox counter of a point y*nx + x -- and
    differ from the walks that reset every Rl, every R, and never.  Asserted on the CPU first, on the oracle's own occupations:
    the walk holds at least 5 points and the four walks differ.
    The corrected signal follows the rule of test_latching_walks_the_line_as_one_row, for the reason given there: the kernel
    adds 2 sum_i A[N][i] (held_i - n_i) to the sensor constant of a held point and forms the Lorentzians from it, the oracle's
    sensor_signal forms the free energies from the held occupations and differences them; two float64 evaluations of one
    expression that differ by the rounding of the free energies, ~1e-13 in a signal of O(0.1): rtol 1e-9, atol 1e-12."""
    N, R, seed, x, y, rgx, rgy, par, st, dx, dy, occ_oracle = _latch_rows_scene(nx, ny)
    L, n = layout(N), nx * ny
    side = LH.slot(n)[0]
    assert side == {(18, 5): 10, (10, 6): 8}[(nx, ny)] and side not in (nx, ny)
    others = sorted({side, R, n} - {nx})
    rows = _walk(par, N, occ_oracle, nx, 0, seed)
    assert int((rows != occ_oracle).any(axis=1).sum()) >= 5, "the oracle holds too few points of the grid"
    assert not (rows != occ_oracle).any(axis=1)[::nx].any()
    for o in others:
        assert not np.array_equal(rows, _walk(par, N, occ_oracle, o, 0, seed)), f"a walk that resets every {o} points gives the same grid"
    env = _vec(tmp_path, 1, N, R, seed)
    _load(env, par[None], st[None])
    gv, bv, sv = _volts(N, st[None])
    clean = env.scan_grid([0], x, y, rgx, rgy, nx, ny, gv, bv, sv, occupations=True)
    got = env.scan_grid([0], x, y, rgx, rgy, nx, ny, gv, bv, sv, occupations=True, noise=("latch",), serial=LATCH_SERIAL,
                        stream_base=LATCH_BASE)
    occ0, occ1 = _np(clean["occupations"])[0].reshape(n, N), _np(got["occupations"])[0].reshape(n, N)
    want = _walk(par, N, occ0, nx, 0, seed)
    held = (want != occ0).any(axis=1)
    print(f"[latching rows] N={N} R={R} {nx}x{ny} side={side}: held points {int(held.sum())}, per row "
          f"{held.reshape(ny, nx).sum(axis=1).tolist()}")
    assert held.sum() >= 5 and not held[::nx].any()
    assert PH.same(occ1, want)
    for o in others:
        assert not np.array_equal(occ1, _walk(par, N, occ0, o, 0, seed)), o
    v_ext, _, _ = GH.grid_voltages(N, par, st, dx, dy, [*rgx, *rgy], nx, ny)
    sig = NO.sensor_signal(H.dev_view(N, par), v_ext, want, float(par[L.scal + 1]), np.zeros(n))
    raw0, raw1 = _np(clean["raw"])[0].reshape(n), _np(got["raw"])[0].reshape(n)
    print(f"[latching rows] worst corrected signal difference {np.abs(raw1 - sig).max():.3e}")
    assert np.allclose(raw1, sig, rtol=1e-9, atol=1e-12)
    assert PH.same(raw1[~held], raw0[~held]) and not np.any(raw1[held] == raw0[held])
    # nx = 1: every point starts a row, no point is ever held
    col = env.scan_grid([0], x, y, rgx, (-20.0, 20.0), 1, 30, gv, bv, sv, occupations=True, noise=("latch",), serial=LATCH_SERIAL,
                        stream_base=LATCH_BASE)
    col0 = env.scan_grid([0], x, y, rgx, (-20.0, 20.0), 1, 30, gv, bv, sv, occupations=True)
    assert PH.same(col["occupations"], col0["occupations"]) and PH.same(col["raw"], col0["raw"])
    assert np.ptp(_np(col0["occupations"]).reshape(30, N), axis=0).max() >= 1.0                  # and the column does cross transitions
    env.close()


# ------------------------------------------------------------------ 5. the oracle on NumPy-built grids
ORACLE_SEEDS = {2: 50, 4: 50, 6: 51}                       # the devices of test_gpu_scan1d._oracle_case
ORACLE_NX, ORACLE_NY = 16, 4


def _oracle_grids(N):
    """(dx, dy, x_range, y_range, frame): e1_2 over the line case's range against vP_N, and the line cases' dense physical
    direction against a barrier"""
    from qadapt_hip.vec_env import scan_axis_vector as vec
    return [(vec("e1_2", N), vec(f"vP{N}", N), (-2.0, 2.0), (-0.6, 0.9), "virtual"),
            (_dense(N, np.random.default_rng(2000 + N)), vec("B1", N, "physical"), (-1.2, 1.2), (-0.5, 0.75), "physical")]


_ORACLE = {}


def _oracle_case(N):
    """The devices of seed ORACLE_SEEDS[N] "near" and "far" from the ground truth (rng of that seed, vgm_noise = 0), as
    test_gpu_scan1d._oracle_case places them; per env and grid 16 x 4 points built in NumPy (grid_helpers.numpy_grid) from the
    env's own voltages (its physical working point in the physical frame) and the oracle's occupations, signal and relative gap
    there.  CPU only, computed once."""
    if N not in _ORACLE:
        nx, ny, L, G = ORACLE_NX, ORACLE_NY, layout(N), N + 1
        seed = ORACLE_SEEDS[N]
        eb = H.sample_blocks(N, [seed, seed])
        rng = np.random.default_rng(seed)
        states, cases = [], []
        for e, mode in enumerate(("near", "far")):
            par, st = eb.params[e], H.place(N, eb.state[e], mode, rng, vgm_noise=0.0)
            states.append(st)
            dev = H.dev_view(N, par)
            bv = st[L.s_barrier_v:L.s_barrier_v + N - 1]
            virt = AH.base_point(N, st)
            phys = np.concatenate([_physical_point(N, st, par), bv])
            for dx, dy, rgx, rgy, frame in _oracle_grids(N):
                base = phys if frame == "physical" else virt
                qst = SH.query_state(N, st, base[:N], bv, base[N])
                pts = GH.numpy_grid(N, qst, par[L.origin:L.origin + G], dx, dy, [*rgx, *rgy], nx, ny, _fr(frame)).reshape(nx * ny, 2 * N)
                vg, vb = pts[:, :G], pts[:, G:]
                occ, sts, F, tc = O.ground_state_open(dev, vg, vb, return_states=True)
                sig, _ = O.charge_sensor_open(dev, vg, vb, n_open=occ)
                Hm = F[:, :, None] * np.eye(sts.shape[1]) + O.tunnel_hamiltonian(tc, sts)
                w = np.linalg.eigvalsh(Hm)
                hn = np.abs(Hm).sum(axis=2).max(axis=1)
                cases.append(dict(e=e, mode=mode, dx=dx, dy=dy, rgx=rgx, rgy=rgy, frame=frame, gv=base[:N], sv=base[N], bv=bv, occ=occ,
                                  sig=sig[:, 0], rel_gap=(w[:, 1] - w[:, 0]) / hn))
        _ORACLE[N] = (eb.params[:2], np.stack(states), cases)
    return _ORACLE[N]


@pytest.mark.parametrize("N", [2, 4, 6])
def test_grids_against_the_oracle(tmp_path, N):
    """O.ground_state_open / O.charge_sensor_open at NumPy-built grids of 16 x 4 points, on a device near and one far from its
    ground truth, in both frames.  The per-point rule of helpers: where the oracle's relative gap is above GAP_MIN, occupations
    and signal agree within 1e-6; 0 of 64 points may be excused.  Asserted before the GPU is touched: the oracle alone leaves 0
    of 64 points unresolved in each of the 4 grids."""
    params, state, cases = _oracle_case(N)
    nx, ny = ORACLE_NX, ORACLE_NY
    assert len(cases) == 4 and {c["mode"] for c in cases} == {"near", "far"} and {c["frame"] for c in cases} == {"virtual", "physical"}
    for c in cases:
        unres = int((c["rel_gap"] <= H.GAP_MIN).sum())
        assert unres == 0, f"the oracle alone leaves {unres} of 64 points unresolved"
    env = _vec(tmp_path, 2, N, 8, ORACLE_SEEDS[N])
    _load(env, params, state)
    for k, c in enumerate(cases):
        out = env.scan_grid([c["e"]], c["dx"], c["dy"], c["rgx"], c["rgy"], nx, ny, c["gv"][None], c["bv"][None], c["sv"],
                            frame=c["frame"], occupations=True)
        occ, sig = _np(out["occupations"])[0].reshape(nx * ny, N), _np(out["raw"])[0].reshape(nx * ny)
        ok = c["rel_gap"] > H.GAP_MIN
        d_occ = np.abs(occ - c["occ"]).max(axis=1)
        d_sig = np.abs(sig - c["sig"]) / np.maximum(np.abs(c["sig"]), 1e-3)
        print(f"[grid vs oracle] N={N} grid {k} {c['mode']} {c['frame']}: worst occupation {d_occ[ok].max():.3e}, worst signal "
              f"{d_sig[ok].max():.3e}, unresolved {int((~ok).sum())}, smallest gap {c['rel_gap'].min():.2e}, total charge "
              f"{c['occ'].sum(axis=1).min():.2f}..{c['occ'].sum(axis=1).max():.2f}")
        assert np.all(c["rel_gap"][d_occ > 1e-6] <= H.GAP_MIN), d_occ[ok].max()
        assert np.all(c["rel_gap"][d_sig > 1e-6] <= H.GAP_MIN), d_sig[ok].max()
        assert int((~ok).sum()) == 0
    env.close()


# ------------------------------------------------------------------ 6. percentiles and image
def test_percentiles_and_image(tmp_path):
    """plohi has the bits of np.percentile(raw, [0.5, 99.5]) and image those of O.normalise_image(raw), ONE pair per grid: grids of
    1 x 1, 2 x 1, 37 x 3 and 16 x 16 points with and without sensor noise, a constant grid (lo == hi on both axes: all zeros) and
    the two zero directions."""
    N, R = 4, 16
    env = _vec(tmp_path, 2, N, R, 9500)
    st = _placed(env, N, 9500, ("near", "mid"))
    gv, bv, sv = _volts(N, st)
    ids = [0, 1, 1]
    zero = np.zeros(2 * N)
    for nx, ny in ((1, 1), (2, 1), (37, 3), (16, 16)):
        for kw in (dict(), dict(noise=("sensor",), serial=(1 << 63) | 3)):
            out = env.scan_grid(ids, ["e1_2", "vP1", zero], ["U1_2", "vP2", zero], [(-2.0, 2.0), (1.25, 1.25), (-1.0, 1.0)],
                                [(-1.0, 1.5), (-0.5, -0.5), (2.0, -2.0)], nx, ny, gv[ids], bv[ids], sv[ids], **kw)
            raw, img, plohi = _np(out["raw"]), _np(out["image"]), _np(out["plohi"])
            assert raw.shape == (3, ny, nx) and img.shape == (3, ny, nx) and img.dtype == np.float32 and plohi.shape == (3, 2)
            for q in range(3):
                assert PH.same(plohi[q], np.percentile(raw[q], [0.5, 99.5])), (nx, ny, q, bool(kw))
                assert PH.same(img[q], O.normalise_image(raw[q])), (nx, ny, q, bool(kw))
            if not kw:
                # the constant grid and the zero directions repeat one point: equal signals, equal percentiles, an all-zero image
                for q in (1, 2):
                    assert PH.same(raw[q], np.full((ny, nx), raw[q, 0, 0])) and plohi[q, 0] == plohi[q, 1] and not img[q].any(), (nx, ny, q)
            if nx * ny > 2:
                assert np.ptp(raw[0]) > 0 and img[0].max() == 1.0 and img[0].min() == 0.0
                assert np.ptp(raw[0], axis=0).max() > 0 and np.ptp(raw[0], axis=1).max() > 0          # both axes move
            if nx * ny == 1:
                assert not img.any()
    env.close()


# ------------------------------------------------------------------ 7. chunking, guards, inert queries
def _raw_call(env, ids, dirs, rg, gv, bv, nq, nx, ny, raw, image=None, plohi=None, occ=None, flags=0):
    import torch
    from qadapt_hip import _lib
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dt)).cuda()      # noqa: E731
    keep = [t(ids, np.int32), t(dirs, np.float64), t(rg, np.float64), t(gv, np.float64), t(bv, np.float64)]
    o = _lib.QdScanGridOpts(struct_size=ctypes.sizeof(_lib.QdScanGridOpts), noise_flags=flags, serial=(1 << 63) | 5,
                            occ_dst=None if occ is None else occ.data_ptr())
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())          # noqa: E731
    rc = env._lib.qd_scan_grid(env._h, p(keep[0]), nq, nx, ny, p(keep[1]), p(keep[2]), p(keep[3]), p(keep[4]), None, p(raw), p(image),
                               p(plohi), ctypes.byref(o), env._stream())
    torch.cuda.synchronize()
    return rc


def _slots(chunk, N, R, n):
    """qd_line_slots of a handle without the full charge-state space: what lane 0's chunk * C * P records and its
    chunk * C * ceil(P / 256) slabs hold in slots of Rl^2 records, ceil(Rl^2 / 256) slabs each, at most QD_GRID_SLOTS"""
    from qadapt_hip import _lib
    C, P, sp = N - 1, R * R, LH.slot(n)[0] ** 2
    return min(chunk * C * P // sp, chunk * C * -(-P // 256) // -(-sp // 256), _lib.QD_GRID_SLOTS)


@pytest.mark.parametrize("R,nx,ny,chunks", [(8, 16, 4, (2, 3)), (8, 9, 4, (2, 3)), (12, 18, 5, (1, 3))])
def test_guards_inert_queries_and_chunks(tmp_path, R, nx, ny, chunks):
    """7 queries on 3 envs through the C entry point with sensor noise and latching, guard rows on both sides of every
    destination: the same bits with two values of env_chunk that cut the call into launches differently, as qd_line_slots
    says (restated in _slots): a 4-dot 8 x 8 handle with env_chunk 2 and 3 holds 6 and 9 slots of 64 or 36 records (its slabs set
    the count): launches of 6 + 1, then one.  A 12 x 12 handle with env_chunk 1 and 3 holds 3 and 9 slots of 100 records: 3 + 3 +
    1, then one.  Then env ids outside [0, B) leave their pre-filled slots untouched while the live queries beside them keep their bits,
    and a call whose queries are all inert writes nothing."""
    import torch
    from qadapt_hip.vec_env import scan_axis_vector as vec
    N, B, seed = 4, 3, 9600
    ids = np.array([0, 1, 2, 1, 0, 2, 2], np.int32)
    nq, g0, g1, guard = 7, 2, 3, -12345.678
    n = nx * ny
    slots = [_slots(c, N, R, n) for c in chunks]
    assert 1 <= slots[0] < nq <= slots[1], slots                       # several launches, then one
    full = lambda *s: torch.full(s, guard, dtype=torch.float64, device="cuda")     # noqa: E731
    rng = np.random.default_rng(seed)
    dxs = np.stack([vec("e1_2", N), vec("U1_4", N), _dense(N, rng), vec("B2", N), vec("vP1", N), _dense(N, rng),
                    vec({"vP2": 1.0, "B2": -0.5}, N)])
    dys = np.stack([vec("U1_2", N), vec("vP3", N), vec("B1", N), _dense(N, rng), np.zeros(2 * N), vec("e3_4", N), vec("S", N)])
    dirs = np.stack([dxs, dys], axis=1)
    rg = np.tile([-2.5, 2.5, -1.0, 1.5], (nq, 1)) + rng.uniform(-0.3, 0.3, (nq, 4))
    rg[3] = rg[3, [1, 0, 3, 2]]
    flags = 1 | 4
    results = {}
    for chunk in chunks:
        env = _vec(tmp_path, B, N, R, seed, env_chunk=chunk)
        assert env.chunk_envs() == chunk
        st = _placed(env, N, seed, ("near", "mid", "near"))
        gv, bv, _ = _volts(N, st)
        raw, plohi, occ = full(g0 + nq + g1, ny, nx), full(g0 + nq + g1, 2), full(g0 + nq + g1, ny, nx, N)
        img = torch.full((g0 + nq + g1, ny, nx), -7.0, dtype=torch.float32, device="cuda")
        assert _raw_call(env, ids, dirs, rg, gv[ids], bv[ids], nq, nx, ny, raw[g0:], img[g0:], plohi[g0:], occ[g0:], flags) == 0
        out = [a.cpu().numpy() for a in (raw, plohi, occ, img)]
        for a, gval in zip(out, (guard, guard, guard, -7.0)):
            assert np.all(a[:g0] == gval) and np.all(a[g0 + nq:] == gval)
            assert np.isfinite(a[g0:g0 + nq]).all() and not np.any(a[g0:g0 + nq] == gval)
        results[chunk] = out
        if chunk == chunks[0]:
            # inert queries: their slots keep the pre-fill, the live ones keep their bits (same query index = same streams)
            bad_ids = np.array([0, B, -1, 1, B + 5, 2, -7], np.int32)
            live = (bad_ids >= 0) & (bad_ids < B)
            r2, p2, o2 = full(nq, ny, nx), full(nq, 2), full(nq, ny, nx, N)
            i2 = torch.full((nq, ny, nx), -7.0, dtype=torch.float32, device="cuda")
            assert _raw_call(env, bad_ids, dirs, rg, gv[ids], bv[ids], nq, nx, ny, r2, i2, p2, o2, flags) == 0
            for a, b, gval in zip((r2, p2, o2, i2), out, (guard, guard, guard, -7.0)):
                a = a.cpu().numpy()
                assert np.all(a[~live] == gval)
                assert PH.same(a[live], b[g0:g0 + nq][live])
            # an all-inert call writes nothing at all
            r3 = full(nq, ny, nx)
            assert _raw_call(env, np.full(nq, B, np.int32), dirs, rg, gv[ids], bv[ids], nq, nx, ny, r3, flags=flags) == 0
            assert np.all(r3.cpu().numpy() == guard)
        env.close()
    for a, b in zip(results[chunks[0]], results[chunks[1]]):
        assert PH.same(a, b)


# ------------------------------------------------------------------ 8. nothing else moves
def test_grids_leave_no_footprint_on_a_noisy_run(tmp_path):
    """Two handles with all stochastic stages on, env_chunk = 2, a rollout of 3 steps through a truncation with automatic
    reloads; one of them calls scan_grid between all calls: observations, rewards, state blocks, raw signal, percentiles, parameter
    blocks and the observation serial stay byte-identical.  A probe, a scan2d, a scan_affine, a scan1d and an eval_points call
    before and after are byte-equal.  Then grids and lines of different sizes in turn on one handle, whose buffers they share (each
    call may grow them): every repetition of a call keeps its bits."""
    import torch
    N, R, B, seed, max_steps = 4, 16, 3, 2719, 2
    L, C, G = layout(N), N - 1, N + 1
    path = _cfg(tmp_path, max_steps=max_steps)
    plain, poked = [_vec(tmp_path, B, N, R, seed, config_path=path, noise=("sensor", "radial", "latch"), env_chunk=2)
                    for _ in range(2)]
    prng = np.random.default_rng(9)
    calls = [0]

    def poke():
        k = calls[0] % 3
        calls[0] += 1
        nq = (5, 1, 3)[k]
        ids = prng.integers(0, B, nq)
        par = poked._params_host[ids]
        st, _ = poked.get_state()
        gv = st[ids, L.s_gate_gt:L.s_gate_gt + N] + prng.uniform(-2, 2, (nq, N))
        bv = par[:, L.vbopt:L.vbopt + C] + prng.uniform(-2, 2, (nq, C))
        x = ("e1_2", _dense(N, prng), {"vP3": 1.0, "B2": -0.4})[k]
        y = ("U1_2", "B1", _dense(N, prng))[k]
        nx, ny = ((25, 4), (16, 16), (1, 7))[k]
        out = poked.scan_grid(ids, x, y, (-1.5, 1.5), (1.0, -0.5), nx, ny, gv, bv, noise=("sensor", "latch") if k != 1 else None,
                              occupations=k == 2, vgm=None if k else np.broadcast_to(-np.eye(G), (nq, G, G)), gamma=None if k != 2 else 0.2)
        assert np.isfinite(_np(out["raw"])).all() and np.isfinite(_np(out["image"])).all()

    def snapshot(env, obs, rew=None, trunc=None):
        st, steps = env.get_state()
        raw, plohi = env.raw()
        ser = ctypes.c_uint64(0)
        assert env._lib.qd_get_rng_state(env._h, ctypes.byref(ser)) == 0
        d = {k: obs[k].cpu().numpy().copy() for k in ("image", "obs_gate_voltages", "obs_barrier_voltages",
                                                      "plunger_images", "barrier_images")}
        d.update(state=st, steps=steps, raw=raw, plohi=plohi, serial=np.array([ser.value], np.uint64),
                 params=env._params_host.copy())
        if rew is not None:
            d.update(rew=rew.cpu().numpy().copy(), trunc=trunc.cpu().numpy().astype(np.uint8))
        return d

    def side_questions(env):
        par = env._params_host
        st, _ = env.get_state()
        gt = st[:, L.s_gate_gt:L.s_gate_gt + N]
        vb = par[:, L.vbopt:L.vbopt + C]
        out = dict(env.probe(np.arange(B), gt + 1.5, vb, normalised=True))
        out["scan2d"] = env.scan2d(np.arange(B), 0, N + 1, (-1, 2), (1, -1), gt, vb)["raw"]
        out["affine"] = env.scan_affine(np.arange(B), "e1_2", "U1_2", (-1, 2), (1, -1), gt, vb, noise=("sensor", "latch"),
                                        serial=(1 << 63) | 11)["raw"]
        line = env.scan1d(np.arange(B), "e1_2", (-1, 2), 100, gt, vb, noise=("sensor", "latch"), serial=(1 << 63) | 12, occupations=True)
        out.update(line=line["raw"], line_image=line["image"], line_occ=line["occupations"])
        pts = env.eval_points(np.arange(B), par[:, None, L.vopt:L.vopt + G] + np.linspace(-1, 1, 5)[None, :, None],
                              np.repeat(par[:, None, L.vbopt:L.vbopt + C], 5, axis=1))
        out.update(signal=pts["signal"], occupations=pts["occupations"])
        return out

    trace = [[], []]
    for k, env in enumerate((plain, poked)):
        trace[k].append(snapshot(env, env.reset(seed=seed)))
    before = side_questions(poked)
    poke(); poke(); poke()
    after = side_questions(poked)
    for key in before:
        assert PH.same(before[key], after[key]), key
    acts = np.random.default_rng(12).uniform(-1, 1, (3, B, 2 * N - 1)).astype(np.float32)
    truncations = 0
    for t in range(3):
        for k, env in enumerate((plain, poked)):
            obs, rew, term, trunc = env.step(torch.as_tensor(acts[t]).cuda(), auto_reset=True)
            trace[k].append(snapshot(env, obs, rew, trunc))
        truncations += int(trace[0][-1]["trunc"].sum())
        poke(); poke()
    assert truncations >= B, "no truncation and reload fell inside the run"
    for a, b in zip(*trace):
        assert a.keys() == b.keys()
        for key in a:
            assert PH.same(a[key], b[key]), key
    # grids and lines in turn on the shared buffers
    st, _ = poked.get_state()
    gt = st[:, L.s_gate_gt:L.s_gate_gt + N]
    vb = poked._params_host[:, L.vbopt:L.vbopt + C]
    ids = np.arange(B)
    noisy = dict(noise=("sensor", "latch"), serial=(1 << 63) | 21, occupations=True)
    turns = [lambda: poked.scan1d(ids, "e1_2", (-1, 2), 7, gt, vb, **noisy),
             lambda: poked.scan_grid(ids, "e1_2", "U1_2", (-1, 2), (1, -1), 5, 3, gt, vb, **noisy),
             lambda: poked.scan1d(ids, "vP2", (2, -1), 200, gt, vb, **noisy),
             lambda: poked.scan_grid(ids, "vP1", "B2", (-1, 2), (1, -1), 40, 6, gt, vb, **noisy),
             lambda: poked.scan_grid(ids, "e1_2", "U1_2", (-1, 2), (1, -1), 5, 3, gt, vb, occupations=True)]
    first = [{k: _np(v).copy() for k, v in f().items()} for f in turns]
    for i in (3, 0, 4, 2, 1, 0, 3):
        again = turns[i]()
        for key, v in first[i].items():
            assert PH.same(_np(again[key]), v), (i, key)
    assert not PH.same(first[1]["raw"], first[4]["raw"])
    plain.close(); poked.close()


# ------------------------------------------------------------------ 9. refusals
def test_refusals(tmp_path):
    import torch
    from qadapt_hip import _lib
    N, R = 3, 8
    q = DM.load_yaml(None, "qarray_config.yaml")
    q["simulator"]["model"]["max_charge_carriers"] = 2
    qp = tmp_path / "qarray_m2.yaml"
    qp.write_text(yaml.safe_dump(q))
    gv, bv = np.zeros((1, N)), np.zeros((1, N - 1))
    d = np.stack([AH.unit(N, 0), AH.unit(N, 1)])[None]
    rg = [[-1, 1, -1, 1]]
    for kw, word in ((dict(validate=True), "QD_FLAG_VALIDATE"),
                     (dict(num_charge_states="all", qarray_config_path=str(qp)), "full charge-state space")):
        env = _vec(tmp_path, 1, N, R, 77, **kw)
        env.reset(seed=77)
        raw0 = env.raw()[0].copy()
        with pytest.raises(_lib.QdError, match=word) as ei:
            env.scan_grid([0], "e1_2", "vP3", (-1, 1), (-1, 1), 8, 2, gv, bv)
        assert f"code {_lib.QD_ERR_STATE}" in str(ei.value)
        dst = torch.full((1, 2, 8), -5.0, dtype=torch.float64, device="cuda")
        assert _raw_call(env, [0], d, rg, gv, bv, 1, 8, 2, dst) == _lib.QD_ERR_STATE
        assert np.all(dst.cpu().numpy() == -5.0)
        assert PH.same(env.raw()[0], raw0)
        env.close()
    env = _vec(tmp_path, 1, N, R, 78)
    env.reset(seed=78)
    with pytest.raises(ValueError, match="radial"):
        env.scan_grid([0], "e1_2", "vP3", (-1, 1), (-1, 1), 8, 2, gv, bv, noise=("sensor", "radial"))
    for nx, ny in ((0, 4), (4, 0), (R * R + 1, 1), (R + 1, R), (13, 5)):
        with pytest.raises(ValueError, match="nx"):
            env.scan_grid([0], "e1_2", "vP3", (-1, 1), (-1, 1), nx, ny, gv, bv)
    raw = torch.full((1, R * R + 1), -5.0, dtype=torch.float64, device="cuda")
    rc = _raw_call(env, [0], d, rg, gv, bv, 1, 8, 2, raw, flags=_lib.QD_NOISE_RADIAL)
    assert rc == _lib.QD_ERR_ARG and b"radial" in env._lib.qd_last_error(env._h)
    for nx, ny in ((R * R + 1, 1), (13, 5), (1, R * R + 1)):                       # P + 1 points
        rc = _raw_call(env, [0], d, rg, gv, bv, 1, nx, ny, raw)
        assert rc == _lib.QD_ERR_ARG and b"nx*ny <= P" in env._lib.qd_last_error(env._h)
    assert np.all(raw.cpu().numpy() == -5.0)
    for nx, ny in ((R * R, 1), (16, 4), (1, R * R)):                               # P points are the largest grid
        out = env.scan_grid([0], "e1_2", "vP3", (-1, 1), (-1, 1), nx, ny, gv, bv)
        assert np.isfinite(_np(out["raw"])).all() and out["raw"].shape == (1, ny, nx)
    with pytest.raises(ValueError):
        env.scan_grid([0], "e1_1", "vP3", (-1, 1), (-1, 1), 8, 2, gv, bv)
    env.close()
