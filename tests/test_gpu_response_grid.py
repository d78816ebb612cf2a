"""Charge-response grids on the MI355X (run with -m gpu): qd_scan_grid_response / scan_grid_response against the reference of
tests/response_helpers.py (compare_points, as it is) at EVERY point of every grid, at the voltages of the host build of the grid
front end (tests/grid_helpers.py); the two axis outputs against tests/response_grid_helpers.py (the chain is pinned against a
central difference in tests/test_response_blocks_cpu.py); the bits of scan_grid_thermal; the closed regime bit for bit against
eval_points(n_charge=, kT=, response=True); the open grid against the points; every coupling zero; designed scenes; destinations,
chunks and guard rows; the absent footprint; the refusals; the facade.

Small envs (resolution 9: slots of 64 or 81 records) and the shapes (12, 5), (7, 9), (8, 8), (13, 5): 60, 63, 64 live records in
a slot of 64 and 65 in one of 81.  The grids of the parity tests are drawn ACROSS transition lines: a window around a point where
the two lowest charge states of the kept list cross, a few kT wide in energy, so that -- by the reference alone, checked on the
CPU before the device is asked -- at least a quarter of the points of each query have |chi| kT > 1e-3.

Bounds: response_helpers (chi, jac, dsignal, as they are); docc_axes within tol_jac . |u| + 64 eps sum |jac u|, dsignal_axes
likewise from tol_dsignal.  Worst err / tol measured on an MI355X (also in DESIGN 7, "Charge-response grids"): open grids chi
4.2e-5, jac 1.9e-5, dsignal 4.0e-6, docc_axes 3.8e-5, dsignal_axes 1.2e-5; closed grids chi 5.2e-4; against eval_points 9.9e-5 of
the sum of both tolerances; every tc zero 3.0e-6, tc[1] underflowed 3.0e-4; all_sizes 3.8e-4, one_sector 2.8e-4."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import closed_helpers as CH
import gs_cases as GC
import helpers as H
import points_helpers as PH
import qd_oracle as O
import response_grid_helpers as RG
import response_helpers as RH
import thermal_helpers as TH
import test_gpu_thermal_grid as TG
from qadapt_hip.layout import layout
from test_gpu_levels import _cfg, _load, _np, _vec

pytestmark = pytest.mark.gpu

SHAPES = [(12, 5), (7, 9), (8, 8), (13, 5)]
KT_100K, KT_1K = TH.KB_REF * 100, TH.KB_REF * 1
ALL = ("chi", "jacobian", "dsignal", "docc_axes", "dsignal_axes")


# ------------------------------------------------------------------ grids across transition lines, from the reference alone
def _gaps(dev, N, K, v):
    """energy difference of the two lowest valid charge states of the oracle's kept list at every point (inf with one state)"""
    states, nv = RG.open_lists(dev, v, K)
    F = O.free_energy_states(v, dev.cdd_inv_full, dev.cgd_full, states.astype(np.int64), N)
    F = np.where(np.arange(F.shape[1])[None, :] < nv[:, None], F, np.inf)
    F = np.sort(F, axis=1)
    return F[:, 1] - F[:, 0] if F.shape[1] > 1 else np.full(len(v), np.inf)


def _window(N, K, par, st, frame, rng, kT, vgm=None, barrier=None):
    """a query (dx, dy, x_range, y_range, W0) whose window sits on a crossing of the two lowest charge states along dx: the base
    point is moved to the crossing (three nested scans of the gap along the line), and the ranges are +-4 kT / (d gap / d s) along
    x and half of that figure along y.  None where the line meets no crossing.  barrier = (b, volts): the grid holds barrier b at
    that voltage, compensated on the gates, and moves no barrier"""
    dev = H.dev_view(N, par)
    dx, dy, _, _, W0 = TG._query(N, par, st, frame, rng)
    if barrier is not None:
        dx[N + 1:] = 0.0; dy[N + 1:] = 0.0
        assert frame == "physical"
        W0 = W0.copy()
        b = N + 1 + barrier[0]
        # (the gates take back what the barrier's cross-talk does to the dots' potentials, so the window stays near a transition)
        W0[:N + 1] += np.linalg.solve(dev.cgd_full[:, :N + 1], -dev.cgd_full[:, b] * (barrier[1] - W0[b]))
        W0[b] = barrier[1]
    line = lambda s: _gaps(dev, N, K, RG.physical(N, par, st, frame, W0[None, :] + s[:, None] * dx[None, :], vgm))     # noqa: E731
    lo, hi = -3.0, 3.0
    for level in range(4 if N > 4 else 3):
        s = np.linspace(lo, hi, 61 if N > 4 else 121)
        g = line(s)
        inner = np.flatnonzero((g[1:-1] <= g[:-2]) & (g[1:-1] <= g[2:]) & np.isfinite(g[1:-1])) + 1
        if not inner.size:
            return None
        i = inner[np.argmin(g[inner])]
        lo, hi = s[i - 1], s[i + 1]
    s0 = s[i]
    g3 = line(np.array([s0 - 20 * (hi - lo), s0, s0 + 20 * (hi - lo)]))
    slope = max(abs(g3[0] - g3[1]), abs(g3[2] - g3[1])) / (20 * (hi - lo))
    if not (np.isfinite(slope) and slope > 0):
        return None
    r = 4.0 * kT / slope
    return dx, dy, (-r, r), (0.5 * r, -0.5 * r), W0 + s0 * dx


def _window_on_a_line(N, K, par, st, frame, rng, kT, nx, ny, gamma, vgm=None, barrier=None):
    """(query, reference, share) of the first of at most 40 draws in which, by the reference alone, at least a quarter of the
    points have |chi| kT > 1e-3"""
    for draw in range(40):
        q = _window(N, K, par, st, frame, rng, kT, vgm, barrier)
        if q is None:
            continue
        ref = _reference(N, K, par, st, q, nx, ny, frame, kT, gamma, vgm)
        share = _crossing_share(ref[5], kT)
        if share >= 0.25:
            return q, ref, share
    raise AssertionError("no grid in 40 draws with a quarter of its points on a transition line")


def _reference(N, K, par, st, q, nx, ny, frame, kT, gamma, vgm=None):
    """(v_ext, Hs, states, nv, tcs, refs) of a query, refs[p] the point_reference dict or None without a valid state"""
    dev = H.dev_view(N, par)
    G = N + 1
    if vgm is None:
        v = TG._voltages(N, par, st, q, nx, ny, frame)
    else:
        import grid_helpers as GH
        import scan_helpers as SH
        dx, dy, rgx, rgy, W0 = q
        qst = SH.query_state(N, st, W0[:N], W0[G:], float(W0[N]), vgm=vgm)
        v = GH.grid_voltages(N, par, qst, dx, dy, [*rgx, *rgy], nx, ny, GH.VIRTUAL)[0]
    states, nv = RG.open_lists(dev, v, K)
    Hs, tcs = TH.hamiltonians(dev, v[:, :G], v[:, G:], states, nv)
    refs = [None if Hm is None else RH.point_reference(dev, Hm, states[p, :nv[p]], tcs[p], kT, v[p], gamma)
            for p, Hm in enumerate(Hs)]
    return v, Hs, states, nv, tcs, refs


def _crossing_share(refs, kT):
    return float(np.mean([r is not None and np.abs(r["chi"]).max() * kT > 1e-3 for r in refs]))


def _scan(env, ids, qs, nx, ny, frame, kT, response=ALL, closed=None, **kw):
    N, G = env.N, env.N + 1
    args = ([list(ids), np.stack([q[0] for q in qs]), np.stack([q[1] for q in qs]), [q[2] for q in qs], [q[3] for q in qs], nx, ny,
             np.stack([q[4][:N] for q in qs]), np.stack([q[4][G:] for q in qs])])
    sv = np.array([q[4][N] for q in qs])
    if response is None:
        return env.scan_grid_thermal(*args, kT, sv, n_charge=closed, frame=frame, occupations=True, variance=True, ztail=True, **kw)
    return env.scan_grid_response(*args, kT, sv, n_charge=closed, frame=frame, occupations=True, variance=True, ztail=True,
                                  response=response, **kw)


def _flat(out, key, q, n):
    a = _np(out[key][q])
    return a.reshape((n,) + a.shape[2:])


def _check_query(tag, N, par, st, v, Hs, states, nv, tcs, refs, kT, gamma, out, q, frame, dx, dy, vgm=None, closed=False):
    n = v.shape[0]
    G = N + 1
    dev = H.dev_view(N, par)
    worst = RH.compare_points(tag, dev, Hs, states, nv, tcs, kT, v[:, :G], v[:, G:], gamma, _flat(out, "chi", q, n),
                              _flat(out, "jacobian", q, n), _flat(out, "dsignal", q, n), closed=closed)
    u = RG.axis_directions(N, st, frame, dx, dy, vgm)
    return max(worst, RG.compare_axes(tag, refs, u, _flat(out, "docc_axes", q, n), _flat(out, "dsignal_axes", q, n)))


# ------------------------------------------------------------------ 1. open parity
# (every shape in both frames at 2 and 4 dots; at 8 dots, where the reference of a grid takes seconds on the CPU, one shape per
# frame: 63 live records in a slot of 64 and 65 in one of 81)
_PARITY = [(N, 8, f, s) for N in (2, 4) for f in ("virtual", "physical") for s in range(len(SHAPES))] \
    + [(8, 32, "virtual", 1), (8, 32, "physical", 3)]


@pytest.mark.parametrize("N,K,frame,shape", _PARITY)
def test_open_parity(tmp_path, N, K, frame, shape):
    """R = 9, two envs near their working points (at 1 K a transition shows in chi kT only where tc is within a few hundred kT); one of the four shapes in one of the frames; two queries per call, the kT of 100 K on one
    env and of 1 K on the other (swapped from shape to shape), each across a transition line; in the virtual frame the second
    query brings a matrix of its own.  Every point of every query against the reference"""
    nx, ny = SHAPES[shape]
    rng = np.random.default_rng(9500 + 100 * N + 10 * shape + (frame == "physical"))
    params, state = TG._placed_blocks(N, [51, 52], ("near", "near"), rng)
    kTs = [KT_100K, KT_1K] if shape % 2 == 0 else [KT_1K, KT_100K]
    G = N + 1
    own = np.eye(G) + rng.normal(0, 0.1, (G, G)) if frame == "virtual" else None
    cases = []
    for e in range(2):
        vgm = own if e == 1 else None
        gamma = float(params[e][layout(N).scal + 1])
        q, ref, share = _window_on_a_line(N, K, params[e], state[e], frame, rng, kTs[e], nx, ny, gamma, vgm)
        cases.append((q, ref, share, vgm, gamma))
    env = _vec(tmp_path, 2, N, 9, 51, num_charge_states=K)
    _load(env, params, state)
    kw = {}
    if frame == "virtual":
        kw["vgm"] = np.stack([RG.slot_vgm(N, state[0]), own])
    out = _scan(env, [0, 1], [c[0] for c in cases], nx, ny, frame, np.array(kTs), **kw)
    assert out["chi"].shape == (2, ny, nx, N, 2 * N - 1) and out["jacobian"].shape == (2, ny, nx, N, 2 * N)
    assert out["dsignal"].shape == (2, ny, nx, 2 * N) and out["docc_axes"].shape == (2, ny, nx, N, 2)
    assert out["dsignal_axes"].shape == (2, ny, nx, 2)
    worst = 0.0
    for e, (q, ref, share, vgm, gamma) in enumerate(cases):
        v, Hs, states, nv, tcs, refs = ref
        worst = max(worst, _check_query(f"open N={N} K={K} {frame} {nx}x{ny} env {e} kT={kTs[e]:.2e} ({share:.0%} of the points on a "
                                        f"transition)", N, params[e], state[e], v, Hs, states, nv, tcs, refs, kTs[e], gamma, out, e,
                                        frame, q[0], q[1], vgm))
    print(f"[response grid] open N={N} K={K} {frame} {nx}x{ny}: worst err / tol {worst:.2e}")
    env.close()


# ------------------------------------------------------------------ 2. the thermal bits, with and without sensor noise
@pytest.mark.parametrize("N,K", [(4, 8), (8, 32)])
def test_thermal_outputs_keep_their_bits(tmp_path, N, K):
    """raw, image, plohi, occupations, variance and ztail equal scan_grid_thermal under the same arguments, open (with and without
    noise=("sensor",)) and closed; the response does not depend on the noise"""
    rng = np.random.default_rng(9600 + N)
    params, state = TG._placed_blocks(N, [53, 54], ("near", "mid"), rng)
    env = _vec(tmp_path, 2, N, 9, 53, num_charge_states=K)
    _load(env, params, state)
    nx, ny = 13, 5
    kT = np.array([KT_100K, 3 * KT_1K])
    qs = [_window_on_a_line(N, K, params[e], state[e], "virtual", rng, kT[e], nx, ny, float(params[e][layout(N).scal + 1]))[0]
          for e in range(2)]
    keys = ("raw", "image", "plohi", "occupations", "variance", "ztail")
    noise = dict(noise=("sensor",), serial=(1 << 63) | 9, stream_base=77)
    plain = _scan(env, [0, 1], qs, nx, ny, "virtual", kT)
    noisy = _scan(env, [0, 1], qs, nx, ny, "virtual", kT, **noise)
    for got, kw in ((plain, {}), (noisy, noise)):
        want = _scan(env, [0, 1], qs, nx, ny, "virtual", kT, response=None, **kw)
        for k in keys:
            assert PH.same(got[k], want[k]), (k, kw)
    assert not PH.same(plain["raw"], noisy["raw"])
    for k in ALL:
        assert PH.same(plain[k], noisy[k]), k
        assert np.isfinite(_np(plain[k])).all() and _np(plain[k]).any(), k
    Q = [N, N + 1]
    got = _scan(env, [0, 1], qs, nx, ny, "virtual", kT, closed=Q)
    want = _scan(env, [0, 1], qs, nx, ny, "virtual", kT, response=None, closed=Q)
    for k in keys:
        assert PH.same(got[k], want[k]), ("closed", k)
    env.close()


# ------------------------------------------------------------------ 3. closed parity
def _fma_dot(a, b):
    """sum_j a[j] b[j] in index order with fused multiply-adds from 0.0, exactly rounded"""
    acc = 0.0
    for x, y in zip(a, b):
        acc = float(Fraction(float(x)) * Fraction(float(y)) + Fraction(acc))
    return acc


@pytest.mark.parametrize("N", [2, 4, 8])
def test_closed_parity(tmp_path, N):
    """a closed list is one component: the whole-block solver and epilogue of eval_points.  In the physical frame all five outputs
    are bit for bit those of eval_points(n_charge=, kT=, response=True) at the grid's voltages, the axis outputs contracted on
    the host in index order with fma; every point against the reference on the lists of the host build of the sector search, and
    every column of chi sums to zero"""
    seed = 9700 + N
    rng = np.random.default_rng(seed)
    params, state = TG._placed_blocks(N, [seed, seed + 1], ("near", "mid"), rng)
    env = _vec(tmp_path, 2, N, 9, seed)
    _load(env, params, state)
    nx, ny = 7, 9
    n, G = nx * ny, N + 1
    Qv = [N, N + 1]
    kT = np.array([KT_100K, 10 * KT_1K])
    qs = [TG._query(N, params[e], state[e], "physical", rng) for e in range(2)]
    out = _scan(env, [0, 1], qs, nx, ny, "physical", kT, closed=Qv)
    worst = 0.0
    for e, Q in enumerate(Qv):
        v = TG._voltages(N, params[e], state[e], qs[e], nx, ny, "physical")
        pts = env.eval_points([e], v[None, :, :G], v[None, :, G:], n_charge=Q, kT=kT[e], response=True,
                              outputs=("signal", "occupations", "variance", "ztail"))
        for a, b in (("raw", "signal"), ("occupations", "occupations"), ("variance", "variance"), ("ztail", "ztail"),
                     ("chi", "chi"), ("jacobian", "jacobian"), ("dsignal", "dsignal")):
            assert PH.same(_flat(out, a, e, n), _np(pts[b][0])), (Q, a)
        jac, ds = _np(pts["jacobian"][0]), _np(pts["dsignal"][0])
        u = np.stack([qs[e][0], qs[e][1]])
        docc, dsa = _flat(out, "docc_axes", e, n), _flat(out, "dsignal_axes", e, n)
        for p in range(n):
            for a in range(2):
                assert dsa[p, a] == _fma_dot(ds[p], u[a]), (Q, p, a)
                for i in range(N):
                    assert docc[p, i, a] == _fma_dot(jac[p, i], u[a]), (Q, p, i, a)
        host = CH.host_closed(N, params[e], v, Q, 32)
        nv = np.minimum(host["nvalid"], 32)
        dev = H.dev_view(N, params[e])
        Hs, tcs = TH.hamiltonians(dev, v[:, :G], v[:, G:], host["states"], nv)
        gamma = float(params[e][layout(N).scal + 1])
        worst = max(worst, RH.compare_points(f"closed N={N} Q={Q} kT={kT[e]:.2e}", dev, Hs, host["states"], nv, tcs, kT[e], v[:, :G],
                                             v[:, G:], gamma, _flat(out, "chi", e, n), _flat(out, "jacobian", e, n),
                                             _flat(out, "dsignal", e, n), closed=True))
    print(f"[response grid] closed N={N}: worst err / tol {worst:.2e}")
    env.close()


# ------------------------------------------------------------------ 4. the open grid against the points
@pytest.mark.parametrize("N,K", [(4, 8), (8, 32)])
def test_open_grid_against_eval_points(tmp_path, N, K):
    """the per-component epilogue of the grid and the whole-block one of eval_points(kT=, response=True) at the same voltages:
    within the sum of both tolerances"""
    rng = np.random.default_rng(9800 + N)
    params, state = TG._placed_blocks(N, [55], ("near",), rng)
    env = _vec(tmp_path, 1, N, 9, 55, num_charge_states=K)
    _load(env, params, state)
    nx, ny = 8, 8
    n, G = nx * ny, N + 1
    gamma = float(params[0][layout(N).scal + 1])
    for kT in (KT_100K, KT_1K):
        q, (v, Hs, states, nv, tcs, refs), _ = _window_on_a_line(N, K, params[0], state[0], "physical", rng, kT, nx, ny, gamma)
        out = _scan(env, [0], [q], nx, ny, "physical", kT)
        pts = env.eval_points([0], v[None, :, :G], v[None, :, G:], kT=kT, response=True)
        worst = 0.0
        for p, ref in enumerate(refs):
            if ref is None:
                continue
            for a, b, t in (("chi", "chi", ref["tol_chi"][None, :]), ("jacobian", "jacobian", ref["tol_jac"][None, :]),
                            ("dsignal", "dsignal", ref["tol_dsignal"])):
                d = np.abs(_flat(out, a, 0, n)[p] - _np(pts[b][0])[p]) / (2.0 * np.maximum(t, 5e-324))
                worst = max(worst, float(d.max()))
        print(f"[response grid] against eval_points N={N} K={K} kT={kT:.2e}: worst difference / (tol + tol) {worst:.2e}")
        assert worst <= 1.0
    env.close()


# ------------------------------------------------------------------ 5. every coupling zero, one coupling zero, no valid state
def test_zero_couplings(tmp_path):
    """tc_base = 0: every tc is exactly zero, the hop columns are exactly 0.0 and chi_n = -cov / kT with the diagonal -var / kT of
    the device's own variance.  A barrier raised until exp underflows: that pair's column is exactly 0.0 among coupled pairs.
    (A point without a valid state cannot be asked for through the grid: the searches never produce such a record.  Its zeros and
    the slope at <n> = 0 are checked on the same source in tests/test_response_blocks_cpu.py and by the sanitizer program, and
    response_helpers.compare_points would compare one here if a grid held it.)"""
    N, K = 4, 8
    rng = np.random.default_rng(9900)
    params, state = TG._placed_blocks(N, [56, 56], ("near", "near"), rng)
    L, G = layout(N), N + 1
    params[0][L.scal + 0] = 0.0                                            # tc_base: env 0 has no coupling at all
    env = _vec(tmp_path, 2, N, 9, 56, num_charge_states=K)
    _load(env, params, state)
    nx, ny = 8, 8
    n = nx * ny
    kT = KT_100K
    gamma = float(params[0][L.scal + 1])
    q, (v, Hs, states, nv, tcs, refs), _ = _window_on_a_line(N, K, params[0], state[0], "physical", rng, kT, nx, ny, gamma)
    assert not tcs.any()
    out = _scan(env, [0], [q], nx, ny, "physical", kT)
    chi, var = _flat(out, "chi", 0, n), _flat(out, "variance", 0, n)
    assert not chi[:, :, N:].any()
    _check_query("every tc zero", N, params[0], state[0], v, Hs, states, nv, tcs, refs, kT, gamma, out, 0, "physical", q[0], q[1])
    for p, ref in enumerate(refs):
        st = states[p, :nv[p]].astype(np.float64)
        P, _, _ = TH.reference(Hs[p], kT)
        mean = P @ st
        cov = (st - mean).T @ ((st - mean) * P[:, None])
        t = ref["tol_chi"][:N].max()
        assert np.all(np.abs(chi[p][:, :N] + cov / kT) <= t), p
        assert np.all(np.abs(np.diag(chi[p][:, :N]) + var[p] / kT) <= t + TH.tol_occ(Hs[p], kT, st.max()) * st.max() / kT), p
    # env 1: barrier 1 raised until tc[1] underflows to exactly zero
    q1, (v, Hs, states, nv, tcs, refs), _ = _window_on_a_line(N, K, params[1], state[1], "physical", rng, kT, nx, ny, gamma,
                                                              barrier=(1, 800.0))
    assert not tcs[:, 1].any() and np.all(tcs[:, 0] > 0) and np.all(tcs[:, 2] > 0)
    want = np.array([r["chi"] for r in refs])
    coupled = [d for d in (0, 2) if np.abs(want[:, :, N + d]).max() * kT > 1e-6]
    assert coupled, "the reference has no response to a coupled pair in this window"
    out = _scan(env, [1], [q1], nx, ny, "physical", kT)
    chi = _flat(out, "chi", 0, n)
    assert not chi[:, :, N + 1].any() and all(chi[:, :, N + d].any() for d in coupled)
    _check_query("tc[1] underflows", N, params[1], state[1], v, Hs, states, nv, tcs, refs, kT, gamma, out, 0, "physical", q1[0], q1[1])
    env.close()


# ------------------------------------------------------------------ 6. designed scenes
@pytest.mark.parametrize("name", ["all_sizes", "one_sector"])
def test_designed_scenes(tmp_path, name):
    """the 5-dot scenes of gs_cases.py at R = 16: all_sizes holds many small components (every size 1..32), one_sector a single
    component of 32 states per pixel, the case in which the per-component schedule is the whole-block one"""
    N, R = 5, 16
    c = GC.census(name, N, R, 0)
    sizes = np.concatenate(c["sizes"])
    if name == "all_sizes":
        assert set(sizes.tolist()) == set(range(1, 33))
    else:
        assert set(sizes.tolist()) == {32}
    par, st = GC.make(name, N, R)
    L = layout(N)
    env = _vec(tmp_path, 1, N, R, 9200)
    _load(env, par[None], st[None])
    w = float(par[L.scal + 2])
    W0 = np.concatenate([st[L.s_gate_v:L.s_gate_v + N], [st[L.s_sensor_gt]], st[L.s_barrier_v:L.s_barrier_v + N - 1]])
    q = (np.eye(2 * N)[0], np.eye(2 * N)[1], (-w, w), (-w, w), W0)
    v = TG._voltages(N, par, st, q, R, R, "virtual")
    states = np.asarray(c["states"])
    nv = np.full(R * R, 32)
    dev = H.dev_view(N, par)
    Hs, tcs = TH.hamiltonians(dev, v[:, :N + 1], v[:, N + 1:], states, nv)
    gamma = float(par[L.scal + 1])
    kT = 0.05
    refs = [RH.point_reference(dev, Hm, states[p], tcs[p], kT, v[p], gamma) for p, Hm in enumerate(Hs)]
    out = _scan(env, [0], [q], R, R, "virtual", kT)
    _check_query(f"{name} kT={kT}", N, par, st, v, Hs, states, nv, tcs, refs, kT, gamma, out, 0, "virtual", q[0], q[1])
    env.close()


# ------------------------------------------------------------------ 7. destinations, chunks, guard rows
def _raw_call(env, ids, dirs, rg, gv, bv, kT, nq, nx, ny, dst, n_charge=None, flags=0, ropts_size=None, null_ropts=False):
    import torch
    from qadapt_hip import _lib
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dt)).cuda()      # noqa: E731
    keep = [t(ids, np.int32), t(dirs, np.float64), t(rg, np.float64), t(gv, np.float64), t(bv, np.float64),
            None if kT is None else t(kT, np.float64), None if n_charge is None else t(n_charge, np.int32)]
    addr = lambda x: None if x is None else x.data_ptr()                        # noqa: E731
    o = _lib.QdScanGridOpts(struct_size=ctypes.sizeof(_lib.QdScanGridOpts), frame=_lib.QD_SCAN_PHYSICAL, noise_flags=flags,
                            serial=(1 << 63) | 5, occ_dst=addr(dst.get("occupations")))
    ro = _lib.QdGridResponseOpts(struct_size=ctypes.sizeof(_lib.QdGridResponseOpts) if ropts_size is None else ropts_size,
                                 n_charge_dev=addr(keep[6]), var_dst=addr(dst.get("variance")), ztail_dst=addr(dst.get("ztail")),
                                 chi_dst=addr(dst.get("chi")), jac_dst=addr(dst.get("jacobian")), dsignal_dst=addr(dst.get("dsignal")),
                                 docc_axes_dst=addr(dst.get("docc_axes")), dsignal_axes_dst=addr(dst.get("dsignal_axes")))
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())          # noqa: E731
    rc = env._lib.qd_scan_grid_response(env._h, p(keep[0]), nq, nx, ny, p(keep[1]), p(keep[2]), p(keep[3]), p(keep[4]), None, p(keep[5]),
                                        p(dst.get("raw")), p(dst.get("image")), p(dst.get("plohi")), ctypes.byref(o),
                                        None if null_ropts else ctypes.byref(ro), env._stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("nq", [1, 5])
def test_destinations_chunks_inert_queries_and_guard_rows(tmp_path, nq):
    """a 4-dot 8 x 8 handle with env_chunk = 2 holds 6 slots of 36 records: nq + 2 queries, two of them with env ids outside
    [0, B), through the C entry point with guard rows on both sides of every destination.  Every live query has the bits of the
    same query alone, the inert ones leave their rows untouched, the guards stay; each response destination alone gives the
    bits it has among all five; with all five null the call is scan_grid_thermal"""
    import torch
    N, R, B, seed = 4, 8, 3, 9600
    nx, ny = 9, 4
    G = N + 1
    env = _vec(tmp_path, B, N, R, seed, env_chunk=2)
    assert env.chunk_envs() == 2
    rng = np.random.default_rng(seed + nq)
    params, state = TG._placed_blocks(N, [seed, seed + 1, seed + 2], ("near", "mid", "near"), rng)
    _load(env, params, state)
    tot = nq + 2
    ids = np.array({1: [B, 1, -3], 5: [0, B, 2, 1, -1, 2, 0]}[nq], np.int32)
    live = (ids >= 0) & (ids < B)
    envs = np.clip(ids, 0, B - 1)
    qs = [TG._query(N, params[e], state[e], "physical", rng) for e in envs]
    dirs = np.stack([np.stack([q[0], q[1]]) for q in qs])
    rg = np.array([[*q[2], *q[3]] for q in qs])
    gv, bv = np.stack([q[4][:N] for q in qs]), np.stack([q[4][G:] for q in qs])
    kT = KT_100K * (1.0 + 0.37 * np.arange(tot))
    g0, g1, guard = 2, 3, -12345.678
    full = lambda *s: torch.full(s, guard, dtype=torch.float64, device="cuda")     # noqa: E731
    shapes = {"chi": (N, 2 * N - 1), "jacobian": (N, 2 * N), "dsignal": (2 * N,), "docc_axes": (N, 2), "dsignal_axes": (2,)}

    def buffers(rows, which=ALL):
        d = dict(raw=full(rows, ny, nx), plohi=full(rows, 2), occupations=full(rows, ny, nx, N), variance=full(rows, ny, nx, N),
                 ztail=full(rows, ny, nx))
        d["image"] = torch.full((rows, ny, nx), -7.0, dtype=torch.float32, device="cuda")
        for k in which:
            d[k] = full(rows, ny, nx, *shapes[k])
        return d

    big = buffers(g0 + tot + g1)
    view = {k: v[g0:] for k, v in big.items()}
    assert _raw_call(env, ids, dirs, rg, gv, bv, kT, tot, nx, ny, view) == 0
    got = {k: v.cpu().numpy() for k, v in big.items()}
    for k, a in got.items():
        gval = -7.0 if k == "image" else guard
        assert np.all(a[:g0] == gval) and np.all(a[g0 + tot:] == gval), k
        assert np.all(a[g0:g0 + tot][~live] == gval), k
        assert np.isfinite(a[g0:g0 + tot][live]).all() and not np.any(a[g0:g0 + tot][live] == gval), k
    for q in np.flatnonzero(live):
        alone = buffers(1)
        assert _raw_call(env, ids[q:q + 1], dirs[q:q + 1], rg[q:q + 1], gv[q:q + 1], bv[q:q + 1], kT[q:q + 1], 1, nx, ny, alone) == 0
        for k in alone:
            assert PH.same(alone[k].cpu().numpy()[0], got[k][g0 + q]), (k, q)
    # each destination alone, and none at all
    for which in [(k,) for k in ALL] + [()]:
        one = buffers(tot, which)
        assert _raw_call(env, ids, dirs, rg, gv, bv, kT, tot, nx, ny, one) == 0
        for k in one:
            assert PH.same(one[k].cpu().numpy(), got[k][g0:g0 + tot]), (which, k)
    none = buffers(tot, ())
    assert _raw_call(env, ids, dirs, rg, gv, bv, kT, tot, nx, ny, none, null_ropts=True) == 0
    for k in ("raw", "image", "plohi", "occupations"):
        assert PH.same(none[k].cpu().numpy(), got[k][g0:g0 + tot]), k
    env.close()


# ------------------------------------------------------------------ 8. nothing else moves
def test_response_grids_leave_no_footprint(tmp_path):
    """scan_grid at T = 0, scan_grid_thermal and eval_points(kT=, response=True) give the same bits before and after response
    grids on the same handle, two identical response grids give the same bits, and one step() of a handle that rendered response
    grids equals that of its twin that did not"""
    import torch
    N, R, B, seed = 4, 8, 2, 9700
    plain, poked = [_vec(tmp_path, B, N, R, seed) for _ in range(2)]
    for env in (plain, poked):
        env.reset(seed=seed)
    L = layout(N)
    st, _ = poked.get_state()
    gv, bv = st[:, L.s_gate_gt:L.s_gate_gt + N], st[:, L.s_barrier_gt:L.s_barrier_gt + N - 1]
    vg, vb = CH.points(N, np.random.default_rng(seed), 40)
    cold = lambda: poked.scan_grid([0, 1], "e1_2", "U1_2", (-2, 2), (1, -1), 9, 5, gv, bv, occupations=True)      # noqa: E731
    warm = lambda: poked.scan_grid_thermal([0, 1], "e1_2", "U1_2", (-2, 2), (1, -1), 9, 5, gv, bv, [0.01, 0.3], variance=True)   # noqa: E731
    pts = lambda: poked.eval_points([0, 1], np.stack([vg, vg]), np.stack([vb, vb]), kT=[0.01, 0.3], response=True)   # noqa: E731
    hot = lambda **kw: poked.scan_grid_response([1, 0], "e1_2", "U1_2", (-2, 2), (1, -1), 9, 5, gv[::-1], bv[::-1], [0.01, 0.3],   # noqa: E731
                                                occupations=True, response=ALL, **kw)
    before = [cold(), warm(), pts()]
    t1, t2 = hot(), hot()
    t3 = poked.scan_grid_response([1, 0], "vP1", "vP2", (-2, 2), (1, -1), 7, 3, gv, bv, 0.05, n_charge=3, response=ALL)
    t4 = hot(noise=("sensor",), serial=(1 << 63) | 3)
    for key in t1:
        assert PH.same(t1[key], t2[key]), key
        assert np.isfinite(_np(t1[key])).all(), key
    assert np.isfinite(_np(t3["chi"])).all() and np.all(np.abs(_np(t3["chi"]).sum(axis=-2)) <= 1e-6)
    assert all(PH.same(t4[k], t1[k]) for k in ALL) and not PH.same(t4["raw"], t1["raw"])
    after = [cold(), warm(), pts()]
    for a, b in zip(before, after):
        assert a.keys() == b.keys()
        for key in a:
            assert PH.same(a[key], b[key]), key
    act = torch.as_tensor(np.random.default_rng(13).uniform(-1, 1, (B, 2 * N - 1)).astype(np.float32)).cuda()
    res = []
    for env in (plain, poked):
        obs, rew, term, trunc = env.step(act)
        stt, steps = env.get_state()
        res.append(dict(image=_np(obs["image"]).copy(), rew=_np(rew).copy(), raw=env.raw()[0].copy(), state=stt, steps=steps))
    for key in res[0]:
        assert PH.same(res[0][key], res[1][key]), key
    plain.close(); poked.close()


# ------------------------------------------------------------------ 9. refusals and the facade
def test_refusals(tmp_path):
    import torch
    from qadapt_hip import _lib
    N, R = 3, 8
    rng = np.random.default_rng(31)
    params, state = TG._placed_blocks(N, [31, 32], ("near", "near"), rng)
    L = layout(N)
    params[1][L.scal + 4] = 1.0; params[1][L.scal + 5] = 1e-3; params[1][L.scal + 6] = 1e-3      # env 1: voltage-dependent capacitances
    env = _vec(tmp_path, 2, N, R, 78)
    _load(env, params, state)
    gv, bv = np.zeros((1, N)), np.zeros((1, N - 1))
    grid = lambda e, kT, **kw: env.scan_grid_response([e], "e1_2", "vP3", (-1, 1), (-1, 1), 8, 2, gv, bv, kT, **kw)      # noqa: E731
    with pytest.raises(ValueError, match="kT"):
        grid(0, None)
    with pytest.raises(ValueError, match="latch"):
        grid(0, 0.01, noise=("latch",))
    for bad in ((), ("chi", "nope"), "dsdv"):
        with pytest.raises(ValueError, match="response must name"):
            grid(0, 0.01, response=bad)
    before = grid(0, 0.02, response=ALL)
    with pytest.raises(_lib.QdError, match="voltage-dependent capacitance") as ei:
        grid(1, 0.02)
    assert f"code {_lib.QD_ERR_STATE}" in str(ei.value) and "qd_scan_grid_response" in str(ei.value)
    # ... and accepted with no response destination: the call is scan_grid_thermal, which takes such envs
    d = np.stack([np.eye(2 * N)[0], np.eye(2 * N)[1]])[None]
    rg = [[-1, 1, -1, 1]]
    dst = dict(raw=torch.full((1, 2, 8), -5.0, dtype=torch.float64, device="cuda"))
    assert _raw_call(env, [1], d, rg, gv, bv, [0.02], 1, 8, 2, dst) == 0
    want = env.scan_grid_thermal([1], 0, 1, (-1, 1), (-1, 1), 8, 2, gv, bv, 0.02, frame="physical")
    assert PH.same(dst["raw"].cpu().numpy(), want["raw"])
    # a query that is not live does not count: its env id names no env
    dst5 = dict(dsignal_axes=torch.full((2, 2, 8, 2), -5.0, dtype=torch.float64, device="cuda"))
    assert _raw_call(env, [0, 7], np.tile(d, (2, 1, 1)), rg * 2, np.tile(gv, (2, 1)), np.tile(bv, (2, 1)), [0.02, 0.02], 2, 8, 2, dst5) == 0
    assert np.all(dst5["dsignal_axes"].cpu().numpy()[1] == -5.0) and not np.any(dst5["dsignal_axes"].cpu().numpy()[0] == -5.0)
    dstr = dict(chi=torch.full((1, 2, 8, N, 2 * N - 1), -5.0, dtype=torch.float64, device="cuda"))
    size_r = ctypes.sizeof(_lib.QdGridResponseOpts)
    cases = [(dict(kT=[0.0]), "kT", _lib.QD_ERR_ARG), (dict(kT=None), "kT_dev", _lib.QD_ERR_ARG),
             (dict(kT=[0.02], ropts_size=size_r - 8), "struct_size", _lib.QD_ERR_ARG),
             (dict(kT=[0.02], flags=_lib.QD_NOISE_LATCH), "QD_NOISE_LATCH", _lib.QD_ERR_ARG),
             (dict(kT=[0.02], flags=_lib.QD_NOISE_SENSOR, n_charge=[2]), "closed regime", _lib.QD_ERR_ARG)]
    for kw, word, code in cases:
        rc = _raw_call(env, [0], d, rg, gv, bv, kw.pop("kT"), 1, 8, 2, dstr, **kw)
        msg = env._lib.qd_last_error(env._h).decode()
        assert rc == code and msg.startswith("qd_scan_grid_response") and word in msg, (kw, rc, msg)
        assert np.all(dstr["chi"].cpu().numpy() == -5.0)
    rc = _raw_call(env, [1], d, rg, gv, bv, [0.02], 1, 8, 2, dstr)
    assert rc == _lib.QD_ERR_STATE and np.all(dstr["chi"].cpu().numpy() == -5.0)
    after = grid(0, 0.02, response=ALL)                                   # the handle is usable
    for key in before:
        assert PH.same(before[key], after[key]), key
    env.close()


def test_facade_response_grids(tmp_path):
    """do2d_response and do1d_response equal the vectorised call bit for bit"""
    from qadapt_hip.env import QuantumDeviceEnv
    N, R = 3, 8
    path = _cfg(tmp_path, num_dots=N, resolution=R)
    backend = _vec(tmp_path, 1, N, R, 9900, config_path=path)
    env = QuantumDeviceEnv(config_path=path, num_dots=N, backend=backend)
    model = env.array.model
    T = float(backend.last_episode.extras["T"][0])
    par = backend._params_host[0]
    L, G = layout(N), N + 1
    p0 = par[L.vopt:L.vopt + G]
    nx, ny = 7, 5
    xs, ys = (p0[0] - 3, p0[0] + 3), (p0[1] + 2, p0[1] - 2)
    sig, dsx, dsy, dnx, dny = model.do2d_response("P1", xs[0], xs[1], nx, "P2", ys[0], ys[1], ny)
    assert sig.shape == (ny, nx, 1) and dsx.shape == dsy.shape == (ny, nx) and dnx.shape == dny.shape == (ny, nx, N)
    want = backend.scan_grid_response([0], 0, 1, xs, ys, nx, ny, np.zeros((1, N)), np.zeros((1, N - 1)), TH.KB_REF * T, 0.0,
                                      frame="physical", gamma=float(model.coulomb_peak_width), response=ALL)
    assert PH.same(sig[:, :, 0], want["raw"][0])
    assert PH.same(dsx, _np(want["dsignal_axes"])[0, ..., 0]) and PH.same(dsy, _np(want["dsignal_axes"])[0, ..., 1])
    assert PH.same(dnx, _np(want["docc_axes"])[0, ..., 0]) and PH.same(dny, _np(want["docc_axes"])[0, ..., 1])
    # physical axes P1, P2: the axis derivatives are columns 0 and 1 of the jacobian and of dsignal
    assert PH.same(dnx, _np(want["jacobian"])[0, ..., 0]) and PH.same(dsy, _np(want["dsignal"])[0, ..., 1])
    s1, d1x, d1y, n1x, n1y = model.do1d_response("P1", xs[0], xs[1], nx, T=T)
    row = backend.scan_grid_response([0], 0, np.zeros(2 * N), xs, (0.0, 0.0), nx, 1, np.zeros((1, N)), np.zeros((1, N - 1)),
                                     TH.KB_REF * T, 0.0, frame="physical", gamma=float(model.coulomb_peak_width))
    assert s1.shape == (nx, 1) and PH.same(d1x, _np(row["dsignal_axes"])[0, 0, :, 0]) and PH.same(n1x, _np(row["docc_axes"])[0, 0, ..., 0])
    assert not d1y.any() and not n1y.any()
    sv, *_ = model.do2d_response("vP1", -1, 1, 4, "e1_2", -1, 1, 3, T=T, n_charge=2)
    assert sv.shape == (3, 4, 1)
    with pytest.raises(NotImplementedError):
        model.do2d_response("P1", 0, 1, 3, "vP2", 0, 1, 3)
    backend.close()
