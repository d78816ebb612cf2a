"""Finite-temperature grids on the MI355X (run with -m gpu): qd_scan_grid_thermal / scan_grid_thermal(..., kT, n_charge=...)
against the reference of tests/thermal_helpers.py at EVERY point of every grid -- eigh of the oracle's Hamiltonian on its kept list
cut to the nv valid states, P = V^2 softmax(-w / kT) -- at the voltages of the host build of the grid front end
(tests/grid_helpers.py); the designed scenes of gs_cases.py and search_cases.py, the per-point route, sensor noise, slots and
launch chunks with guard rows, more than one point per block, the absent footprint, the refusals and the facade.

Bound everywhere (thermal_helpers, as it is): occupations within tol_occ = n_max 4 (1e-12 hs + 1e-13 hn) min(1 / kT, 1 / g) + 1e-12,
variances within n_max tol_occ, ztail within the same expression without n_max; the signal within 1e-12 relative of the sensor
expression at the device's own occupations; plohi and image bit for bit those of numpy.percentile and the oracle's normalisation
of the raw signal.  In the open regime the kernel (csrc/qd_thermal_blocks.h) solves each hop component by itself and is NOT
bitwise equal to eval_points(kT=), which solves the whole block (csrc/qd_thermal.h): the two are compared within the sum of both
tolerances.  A closed list is one component and runs the whole-block core: bit for bit the points, in the physical frame."""
import ctypes

import numpy as np
import pytest
import yaml

import closed_helpers as CH
import grid_helpers as GH
import gs_cases as GC
import helpers as H
import points_helpers as PH
import probe_noise_helpers as PN
import qd_noise_oracle as NO
import qd_oracle as O
import scan_helpers as SH
import search_cases as SC
import thermal_helpers as TH
from qadapt_hip import device_model as DM
from qadapt_hip.layout import layout
from test_gpu_levels import _cfg, _load, _np, _open_lists, _vec
from test_gpu_thermal import KT_100K, _gaps, _signal_from

pytestmark = pytest.mark.gpu

SHAPES = [(12, 5), (7, 9), (8, 8), (13, 5)]           # 60, 63, 64 live records in a slot of 64, 65 in one of 81


def _dense(N, rng):
    """a dense direction: normal coefficients, the sensor component x0.1 and the barrier components x0.02.
    The barriers move little WITHIN a grid on purpose.  The bound of thermal_helpers on ztail, 4 (1e-12 hs + 1e-13 hn) / kT, has
    no floor, and a float64 quotient of order 1 / K carries half an ulp of its own (7e-18 at 1/8) whatever computes it, the
    reference included: the bound means something only where kT is below about 1e4 (hs + hn / 10).  The temperatures here are
    tied to the MEDIAN gap of a grid's points, and the gap follows the tunnel couplings, which change by a decade per 0.1 V of a
    barrier on these devices: a grid that swept its barriers by volts would hold points whose whole Hamiltonian lies six decades
    below kT.  The decades of tc are covered from env to env and call to call instead (helpers.place moves the barriers of the
    three envs by up to 3, 6 and 12 V)."""
    d = rng.normal(size=2 * N)
    d[N] *= 0.1
    d[N + 1:] *= 0.02
    return d


def _physical_point(N, st, par):
    L = layout(N); G = N + 1
    vgm = st[L.s_vgm:L.s_vgm + G * G].reshape(G, G)
    return vgm @ np.concatenate([st[L.s_gate_v:L.s_gate_v + N], [st[L.s_sensor_gt]]]) + par[L.origin:L.origin + G]


def _query(N, par, st, frame, rng):
    """one grid on a placed env: (dx, dy, x_range, y_range, base point W0 (2N,)) -- two dense directions through the env's own
    working point, the second range downwards"""
    L, G = layout(N), N + 1
    bv = st[L.s_barrier_v:L.s_barrier_v + N - 1]
    if frame == "physical":
        W0 = np.concatenate([_physical_point(N, st, par), bv])
    else:
        W0 = np.concatenate([st[L.s_gate_v:L.s_gate_v + N], [st[L.s_sensor_gt]], bv])
    return _dense(N, rng), _dense(N, rng), (-1.5, 1.5), (1.0, -2.0), W0


def _voltages(N, par, st, q, nx, ny, frame):
    """v_ext (ny*nx, 2N) of the grid, with the bits of the device's front end (tests/hosttest_grid)"""
    dx, dy, rgx, rgy, W0 = q
    G = N + 1
    qst = SH.query_state(N, st, W0[:N], W0[G:], float(W0[N]))
    return GH.grid_voltages(N, par, qst, dx, dy, [*rgx, *rgy], nx, ny, GH.PHYSICAL if frame == "physical" else GH.VIRTUAL)[0]


def _scan(env, ids, qs, nx, ny, frame, kT, closed=None, **kw):
    N, G = env.N, env.N + 1
    args = ([list(ids), np.stack([q[0] for q in qs]), np.stack([q[1] for q in qs]), [q[2] for q in qs], [q[3] for q in qs], nx, ny,
             np.stack([q[4][:N] for q in qs]), np.stack([q[4][G:] for q in qs])])
    sv = np.array([q[4][N] for q in qs])
    return env.scan_grid_thermal(*args, kT, sv, n_charge=closed, frame=frame, occupations=True, variance=True, ztail=True, **kw)


def _check(tag, N, par, v_ext, Hs, states, nv, kT, out, q, gamma=None, signal=True):
    """query q of a grid call against the reference at every point; the signal against the sensor expression at the device's own
    occupations to 1e-12 relative; plohi and image against numpy; returns the worst err / tol"""
    n = v_ext.shape[0]
    occ, var, zt, raw = (_np(out[k][q]).reshape((n, -1)) for k in ("occupations", "variance", "ztail", "raw"))
    worst = TH.compare_points(tag, Hs, states, nv, kT, occ, var, zt[:, 0])
    if signal:
        L = layout(N)
        want = _signal_from(N, par, v_ext, occ, par[L.scal + 1] if gamma is None else gamma)
        rel = np.abs(raw[:, 0] - want) / np.abs(want)
        print(f"[thermal grid] {tag}: worst signal difference from the sensor expression at the device's occupations {rel.max():.2e}")
        assert np.all(rel <= 1e-12), (tag, float(rel.max()))
    r2 = _np(out["raw"][q])
    assert PH.same(_np(out["plohi"][q]), np.percentile(r2, [0.5, 99.5])), tag
    assert PH.same(_np(out["image"][q]), O.normalise_image(r2)), tag
    return worst


def _placed_blocks(N, seeds, modes, rng):
    eb = H.sample_blocks(N, seeds)
    st = np.stack([H.place(N, eb.state[e], mode, rng) for e, mode in enumerate(modes)])
    return eb.params.copy(), st


def _draw(N, par, st, frame, nx, ny, rng, lists, kind):
    """A grid on a placed env, its reference and its temperature of `kind` (0: 1e-2 times the median gap of its points, 1: that
    gap, 2: the kT of 100 K): (query, v_ext, Hs, states, nv, kT, largest tc).  `lists(v_ext)` gives the kept states and their
    number.  The directions are drawn again, at most 40 times, until the bound on ztail is at least half an ulp of 1 / nv at
    every point -- decided from the reference alone, before the device is asked: thermal_helpers' bound has no floor, and below
    that figure it is under the rounding of any float64 quotient of that size (see _dense).  It happens where the median gap of
    a grid is set by strongly coupled lists (1e6 and more on the far env) and single points hold a list without one coupled pair,
    whose whole Hamiltonian is of order 0.1."""
    for draws in range(1, 41):
        q = _query(N, par, st, frame, rng)
        v = _voltages(N, par, st, q, nx, ny, frame)
        states, nv = lists(v)
        assert nv.max() >= 2
        Hs, tc = TH.hamiltonians(H.dev_view(N, par), v[:, :N + 1], v[:, N + 1:], states, nv)
        gap = float(np.nanmedian(_gaps(Hs)))
        assert gap > 0
        kT = (1e-2 * gap, gap, KT_100K)[kind]
        if all(TH.tol_ztail(Hm, kT) >= 2.0 ** -53 / Hm.shape[0] for Hm in Hs if Hm is not None):
            return q, v, Hs, states, nv, kT, float(tc.max())
    raise AssertionError("no grid in 40 draws whose ztail bound is above the rounding of a quotient")


# ------------------------------------------------------------------ 1. oracle parity, open
@pytest.mark.parametrize("shape", range(len(SHAPES)))
@pytest.mark.parametrize("frame", ["virtual", "physical"])
@pytest.mark.parametrize("N,K", [(2, 32), (3, 32), (4, 32), (8, 32), (8, 8), (8, 16)])
def test_open_parity(tmp_path, N, K, frame, shape):
    """R = 16, one env near, one mid, one far (helpers.place, the spans of test_gpu_thermal.py); one of the four grid shapes in one
    of the frames, one query per env in one call, each query with a kT of its own: 1e-2 and 1 times the env's median gap and
    the kT of 100 K, rotated over the envs from case to case so that every env meets every temperature.  (One case per shape
    and frame: the oracle's kept lists of an 8-dot grid take a second or two.)"""
    nx, ny = SHAPES[shape]
    call = shape + len(SHAPES) * (frame == "physical")
    rng = np.random.default_rng(9000 + 10 * N + K)
    params, state = _placed_blocks(N, [41, 42, 43], ("near", "mid", "far"), rng)
    # (two cases whose first seed needs 4 and 9 redraws on the far env, seconds of oracle each: fixed on the CPU, from the reference
    # alone, at the first seed that needs none)
    shift = {(8, 8, "virtual", 1): 8, (8, 8, "physical", 0): 8}.get((N, K, frame, shape), 0)
    rng = np.random.default_rng(9000 + 10 * N + K + 1000 * (call + 1) + 100000 * shift)
    env = _vec(tmp_path, 3, N, 16, 41, num_charge_states=K)
    _load(env, params, state)
    cases = []
    for e in range(3):
        dev = H.dev_view(N, params[e])
        cases.append(_draw(N, params[e], state[e], frame, nx, ny, rng, lambda v: _open_lists(dev, v[:, :N + 1], v[:, N + 1:], K),
                           (e + call) % 3))
    kT = np.array([c[5] for c in cases])
    out = _scan(env, [0, 1, 2], [c[0] for c in cases], nx, ny, frame, kT)
    assert out["raw"].shape == (3, ny, nx) and out["variance"].shape == (3, ny, nx, N) and out["ztail"].shape == (3, ny, nx)
    assert len(set(kT.tolist())) == 3
    worst = 0.0
    for e, mode in enumerate(("near", "mid", "far")):
        _, v, Hs, states, nv, _, tcmax = cases[e]
        worst = max(worst, _check(f"open N={N} K={K} {frame} {nx}x{ny} {mode} kT={kT[e]:.2e} (tc up to {tcmax:.1e})", N, params[e], v,
                                  Hs, states, nv, kT[e], out, e))
    print(f"[thermal grid] open N={N} K={K} {frame} {nx}x{ny}: worst err / tol {worst:.2e}")
    env.close()


# ------------------------------------------------------------------ 2. oracle parity, closed
@pytest.mark.parametrize("N", [4, 8])
def test_closed_parity(tmp_path, N):
    """three envs, a total charge per query, the kept lists of the host build of the sector search (closed_helpers): the bound at
    every point, and occupations that sum to Q within 1e-9"""
    seed = 9100 + N
    rng = np.random.default_rng(seed)
    params, state = _placed_blocks(N, [seed, seed + 1, seed + 2], ("near", "mid", "near"), rng)
    env = _vec(tmp_path, 3, N, 16, seed)
    _load(env, params, state)
    Qv = [1, N, N + 2]
    worst = 0.0

    def closed_lists(e, Q):
        def lists(v):
            host = CH.host_closed(N, params[e], v, Q, 32)
            return host["states"], np.minimum(host["nvalid"], 32)
        return lists

    for frame, (nx, ny) in (("physical", (12, 5)), ("virtual", (13, 5))):
        cases = [_draw(N, params[e], state[e], frame, nx, ny, rng, closed_lists(e, Q), e) for e, Q in enumerate(Qv)]
        kT = np.array([c[5] for c in cases])
        out = _scan(env, [0, 1, 2], [c[0] for c in cases], nx, ny, frame, kT, closed=Qv)
        for e, Q in enumerate(Qv):
            _, v, Hs, states, nv, _, _ = cases[e]
            worst = max(worst, _check(f"closed N={N} Q={Q} {frame} {nx}x{ny} kT={kT[e]:.2e}", N, params[e], v, Hs, states, nv, kT[e], out, e))
            tot = _np(out["occupations"][e]).reshape(nx * ny, N).sum(axis=1)
            assert np.all(np.abs(tot[nv > 0] - Q) <= 1e-9), (Q, float(np.abs(tot[nv > 0] - Q).max()))
        if frame == "physical":
            # a closed list is one hop component, so the closed grid runs the whole-block core of eval_points(kT=): in the physical
            # frame it has the bits of the points at the grid's voltages, as the closed grid at T = 0 has
            for e, Q in enumerate(Qv):
                v = cases[e][1]
                pts = env.eval_points([e], v[None, :, :N + 1], v[None, :, N + 1:], n_charge=Q, kT=kT[e],
                                      outputs=("signal", "occupations", "variance", "ztail"))
                for a, b in (("raw", "signal"), ("occupations", "occupations"), ("variance", "variance"), ("ztail", "ztail")):
                    assert PH.same(_np(out[a][e]).reshape(_np(pts[b][0]).shape), pts[b][0]), (Q, a)
    print(f"[thermal grid] closed N={N}: worst err / tol {worst:.2e}")
    env.close()


# ------------------------------------------------------------------ 3. the designed scenes
def _designed(tmp_path, name, N, R, par, st, kTs, seed):
    """channel 0's window of a designed scene as a grid with nx = ny = R: (env, out per kT, v_ext, states of the C oracle)"""
    L = layout(N)
    env = _vec(tmp_path, 1, N, R, seed)
    _load(env, par[None], st[None])
    w = float(par[L.scal + 2])
    gv, bv, sv = st[L.s_gate_v:L.s_gate_v + N], st[L.s_barrier_v:L.s_barrier_v + N - 1], st[L.s_sensor_gt]
    W0 = np.concatenate([gv, [sv], bv])
    ux, uy = np.eye(2 * N)[0], np.eye(2 * N)[1]
    q = (ux, uy, (-w, w), (-w, w), W0)
    v = _voltages(N, par, st, q, R, R, "virtual")
    assert np.allclose(v, PH.scan_voltages(N, par, st, 0, R)[0], rtol=0, atol=1e-12)     # channel 0's pixels, in its order
    outs = [_scan(env, [0], [q], R, R, "virtual", kT) for kT in kTs]
    return env, outs, v


@pytest.mark.parametrize("name", ["all_sizes", "one_sector", "cut_pair", "denormal_pair", "cut_two"])
def test_designed_scenes(tmp_path, name):
    """the 5-dot scenes of gs_cases.py at R = 16, 256 pixels each.  all_sizes holds components of every size 1..32 (asserted
    from the census first); one_sector is one 32-state component per pixel, the case of the whole-block solver; cut_pair and
    cut_two fall apart along pairs whose coupling is exactly zero; in denormal_pair that coupling is a denormal, which links"""
    N, R = 5, 16
    c = GC.census(name, N, R, 0)
    sizes = np.concatenate(c["sizes"])
    if name == "all_sizes":
        assert set(sizes.tolist()) == set(range(1, 33)), "a component size is missing from the scene"
    if name in ("one_sector", "denormal_pair"):
        assert set(sizes.tolist()) == {32}
    if name in ("cut_pair", "cut_two"):
        assert sizes.max() < 32 and all(len(s) > 1 for s in c["sizes"])
    par, st = GC.make(name, N, R)
    kTs = (0.004, 0.05)
    env, outs, v = _designed(tmp_path, name, N, R, par, st, kTs, 9200)
    states = np.asarray(c["states"])
    nv = np.full(R * R, 32)
    Hs, tc = TH.hamiltonians(H.dev_view(N, par), v[:, :N + 1], v[:, N + 1:], states, nv)
    if name == "denormal_pair":
        assert np.all((tc[:, 1] > 0) & (tc[:, 1] < 2.3e-308))
    for kT, out in zip(kTs, outs):
        _check(f"{name} kT={kT}", N, par, v, Hs, states, nv, kT, out, 0)
    if name in ("cut_pair", "denormal_pair"):
        # the same physics with and without the link: a denormal coupling changes no occupation beyond the tolerance
        other = "denormal_pair" if name == "cut_pair" else "cut_pair"
        par2, st2 = GC.make(other, N, R)
        env2, outs2, _ = _designed(tmp_path, other, N, R, par2, st2, kTs[:1], 9201)
        d = np.abs(_np(outs[0]["occupations"]) - _np(outs2[0]["occupations"])).max()
        tol = 2 * max(TH.tol_occ(Hm, kTs[0], float(states[p].max())) for p, Hm in enumerate(Hs))
        print(f"[thermal grid] {name} against {other}: largest occupation difference {d:.2e} (tol {tol:.2e})")
        assert d <= tol
        env2.close()
    env.close()


def test_zero_couplings_give_the_boltzmann_distribution_over_the_oracles_energies(tmp_path):
    """all_sizes with tc_base = 0: every coupling exactly zero, every state a component of its own, no sweep; the occupations are
    the softmax over the oracle's free energies of the kept states"""
    N, R, name = 5, 16, "all_sizes"
    L = layout(N)
    par, st = GC.make(name, N, R)
    par[L.scal] = 0.0
    kTs = (0.004, 0.05)
    env, outs, v = _designed(tmp_path, name, N, R, par, st, kTs, 9210)
    states = np.asarray(GC.census(name, N, R, 0)["states"])
    nv = np.full(R * R, 32)
    Hs, tc = TH.hamiltonians(H.dev_view(N, par), v[:, :N + 1], v[:, N + 1:], states, nv)
    assert not tc.any()
    for kT, out in zip(kTs, outs):
        occ = _np(out["occupations"][0]).reshape(R * R, N)
        worst = 0.0
        for p, Hm in enumerate(Hs):
            F = np.diag(Hm)
            with np.errstate(under="ignore"):
                want = TH.softmax(-(F - F.min()) / kT) @ states[p].astype(np.float64)
            worst = max(worst, float(np.abs(occ[p] - want).max() / TH.tol_occ(Hm, kT, float(states[p].max()))))
        print(f"[thermal grid] zero couplings kT={kT}: worst |occ - softmax(-F / kT) . states| / tol_occ {worst:.2e}")
        assert worst <= 1.0
        _check(f"zero couplings kT={kT}", N, par, v, Hs, states, nv, kT, out, 0)
    env.close()


def test_dyadic_ties_have_exact_weights(tmp_path):
    """the dyadic scene of search_cases.py (cdd_inv = I / 4, exact energies) with tc_base = 0, as a grid of 2 x 1 points: dot 0 at
    1.5 with the others at integers, a two-fold tie with weights 1/2; every dot at 1.5, a 16-fold tie with weights 1/16"""
    N, R, kT = 4, 8, 0.005
    par, st = SC.make("dyadic", N, R, tc_base=0.0)
    env = _vec(tmp_path, 1, N, R, 9500)
    _load(env, par[None], st[None])
    dev = H.dev_view(N, par)
    a, b = np.array([1.5, 2.0, 1.0, 1.0, 0.25]), np.array([1.5, 1.5, 1.5, 1.5, 0.25])
    vb = np.zeros(N - 1)
    W0 = np.concatenate([a, vb])
    dx = np.concatenate([b - a, vb])
    out = env.scan_grid_thermal([0], dx, np.zeros(2 * N), (0.0, 1.0), (0.0, 0.0), 2, 1, a[None, :N], vb[None], kT, a[N],
                                frame="physical", occupations=True, variance=True, ztail=True)
    v = np.stack([W0, W0 + dx])
    states, nv = _open_lists(dev, v[:, :N + 1], v[:, N + 1:], 32)
    Hs, tc = TH.hamiltonians(dev, v[:, :N + 1], v[:, N + 1:], states, nv)
    assert not tc.any()
    E = [np.sort(np.diag(Hm)) for Hm in Hs]
    assert E[0][0] == E[0][1] < E[0][2] and E[1][0] == E[1][15] < E[1][16]
    _check("dyadic", N, par, v, Hs, states, nv, kT, out, 0)
    occ, var = _np(out["occupations"][0, 0]), _np(out["variance"][0, 0])
    # the tied weights are 1/2 and 1/16 exactly, and so are the sums over them
    # (the next levels lie 50 kT up: their weights of 2e-22 are lost in Z and in every sum over the tied states)
    assert np.array_equal(occ[0], [1.5, 2.0, 1.0, 1.0]) and var[0, 0] == 0.25 and np.all(var[0, 1:] <= 1e-18)
    assert np.array_equal(occ[1], [1.5] * 4) and np.array_equal(var[1], [0.25] * 4)
    env.close()


# ------------------------------------------------------------------ 4. the per-point route
@pytest.mark.parametrize("N,K", [(4, 32), (8, 16)])
def test_grid_against_eval_points(tmp_path, N, K):
    """scan_grid_thermal in the physical frame against eval_points(kT=) at the grid's voltages: occupations, variance and ztail
    within the sum of both tolerances at every point.  The routes solve the same block by different iterations and are not
    bitwise equal; where they are (a point of one component of one or two states can be), nothing is claimed."""
    rng = np.random.default_rng(9300 + N)
    params, state = _placed_blocks(N, [42], ("mid",), rng)
    env = _vec(tmp_path, 1, N, 16, 42, num_charge_states=K)
    _load(env, params, state)
    nx, ny = 13, 5
    q = _query(N, params[0], state[0], "physical", rng)
    v = _voltages(N, params[0], state[0], q, nx, ny, "physical")
    dev = H.dev_view(N, params[0])
    states, nv = _open_lists(dev, v[:, :N + 1], v[:, N + 1:], K)
    Hs, _ = TH.hamiltonians(dev, v[:, :N + 1], v[:, N + 1:], states, nv)
    for kT in (float(np.nanmedian(_gaps(Hs))), KT_100K):
        out = _scan(env, [0], [q], nx, ny, "physical", kT)
        pts = env.eval_points([0], v[None, :, :N + 1], v[None, :, N + 1:], kT=kT, outputs=("signal", "occupations", "variance", "ztail"))
        worst, same = 0.0, 0
        for p, Hm in enumerate(Hs):
            n_max = max(float(states[p, :nv[p]].max()), 1.0)
            to = 2 * TH.tol_occ(Hm, kT, n_max)
            o = np.abs(_np(out["occupations"][0]).reshape(-1, N)[p] - _np(pts["occupations"][0])[p]).max() / to
            va = np.abs(_np(out["variance"][0]).reshape(-1, N)[p] - _np(pts["variance"][0])[p]).max() / (n_max * to)
            z = abs(_np(out["ztail"][0]).reshape(-1)[p] - _np(pts["ztail"][0])[p]) / (2 * TH.tol_ztail(Hm, kT))
            worst = max(worst, o, va, z)
            same += PH.same(_np(out["occupations"][0]).reshape(-1, N)[p], _np(pts["occupations"][0])[p])
        print(f"[thermal grid] against eval_points N={N} K={K} kT={kT:.2e}: worst difference / (tol + tol) {worst:.2e}; "
              f"{same} of {nx * ny} points bitwise equal")
        assert worst <= 1.0
    env.close()


# ------------------------------------------------------------------ 5. sensor noise
def test_sensor_noise_on_the_thermal_constant(tmp_path):
    """noise=("sensor",): the occupations are those of the noise-free thermal grid bit for bit (the sensor stage reads c0 alone),
    and the signal is the oracle's sensor expression at those occupations with the oracle's white and telegraph noise on the
    sensor charge -- white noise keyed by the point index, the telegraph chain over the slot's Rl*Rl states from point 0, channel
    word 0 -- within rtol 1e-9, atol 1e-12, the rule of the latching tests of test_gpu_scan_grid.py for two float64 evaluations of
    one expression"""
    import line_helpers as LH
    N, R, seed, serial, base = 4, 16, 9400, (1 << 63) | 17, 321
    rng = np.random.default_rng(seed)
    params, state = _placed_blocks(N, [seed, seed + 1], ("near", "mid"), rng)
    L = layout(N)
    env = _vec(tmp_path, 2, N, R, seed)
    _load(env, params, state)
    nx, ny = 13, 5
    n, side = nx * ny, LH.slot(nx * ny)[0]
    qs = [_query(N, params[e], state[e], "virtual", rng) for e in range(2)]
    kT = np.array([KT_100K, 0.5 * KT_100K])
    clean = _scan(env, [0, 1], qs, nx, ny, "virtual", kT)
    noisy = _scan(env, [0, 1], qs, nx, ny, "virtual", kT, noise=("sensor",), serial=serial, stream_base=base)
    for key in ("occupations", "variance", "ztail"):
        assert PH.same(clean[key], noisy[key]), key
    assert not PH.same(clean["raw"], noisy["raw"])
    for e in range(2):
        par = params[e]
        v = _voltages(N, par, state[e], qs[e], nx, ny, "virtual")
        nz = PN.noise_params(par, L)
        s = NO.Stream(seed, base + e, serial)
        eta = nz["white_amp"] * NO.normal2(s.block(np.arange(n, dtype=np.uint32), 0, NO.RNG_WHITE))[0]
        eta = eta + nz["tel_amp"] * NO.telegraph_bits(s, 0, side * side, nz["tel_p01"], nz["tel_p10"])[:n]
        occ = _np(noisy["occupations"][e]).reshape(n, N)
        want = NO.sensor_signal(H.dev_view(N, par), v, occ, float(par[L.scal + 1]), eta)
        raw = _np(noisy["raw"][e]).reshape(n)
        print(f"[thermal grid] sensor noise env {e}: worst signal difference {np.abs(raw - want).max():.3e}, noise moves the signal by up "
              f"to {np.abs(raw - _np(clean['raw'][e]).reshape(n)).max():.3e}")
        assert np.allclose(raw, want, rtol=1e-9, atol=1e-12)
        assert PH.same(_np(noisy["plohi"][e]), np.percentile(_np(noisy["raw"][e]), [0.5, 99.5]))
    env.close()


# ------------------------------------------------------------------ 6. more than one point per block
def test_second_point_of_a_block_keeps_nothing_from_the_first(tmp_path):
    """3 dots on an R = 72 handle: one grid of 72 x 72 = 5184 points has more points than the 4096 blocks of its slot, so 1088
    blocks solve a second point on the workspace of the first; two grids of 72 x 36 over the same points have one point per
    block.  Occupations, variance, ztail and raw bit for bit, and 256 of the points against the reference"""
    N, R = 3, 72
    rng = np.random.default_rng(61)
    params, state = _placed_blocks(N, [61], ("mid",), rng)
    env = _vec(tmp_path, 1, N, R, 61)
    _load(env, params, state)
    par, st = params[0], state[0]
    L, G = layout(N), N + 1
    W0 = np.concatenate([_physical_point(N, st, par), st[L.s_barrier_v:L.s_barrier_v + N - 1]])
    ux, uy = np.eye(2 * N)[0], np.eye(2 * N)[1]
    ys = -8.875 + 0.25 * np.arange(R)                                     # a dyadic step: the rows of the halves are those of the whole
    one = _scan(env, [0], [(ux, uy, (-12.0, 12.0), (ys[0], ys[-1]), W0)], R, R, "physical", KT_100K)
    halves = [(ux, uy, (-12.0, 12.0), (ys[0], ys[R // 2 - 1]), W0), (ux, uy, (-12.0, 12.0), (ys[R // 2], ys[-1]), W0)]
    v1 = _voltages(N, par, st, (ux, uy, (-12.0, 12.0), (ys[0], ys[-1]), W0), R, R, "physical")
    v2 = np.concatenate([_voltages(N, par, st, h, R, R // 2, "physical") for h in halves])
    same_points = PH.same(v1, v2)
    two = _scan(env, [0, 0], halves, R, R // 2, "physical", KT_100K)
    if not same_points:
        # linspace over half the range need not round as linspace over the whole: then the points are compared where they agree
        keep = (v1.view(np.uint64) == v2.view(np.uint64)).all(axis=1)
        assert keep.sum() >= R * R // 2, "too few points of the two halves have the bits of the whole grid"
    else:
        keep = np.ones(R * R, bool)
    for key in ("occupations", "variance", "ztail", "raw"):
        a = np.ascontiguousarray(_np(one[key]).reshape(R * R, -1))[keep]
        b = np.ascontiguousarray(_np(two[key]).reshape(R * R, -1))[keep]
        diff = np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)).any(axis=1))
        assert diff.size == 0, (key, diff.size, diff[:8])
    second = np.arange(4096, R * R)                                         # the points a block solves after another
    pick = np.concatenate([second[:: max(1, second.size // 128)][:128], np.arange(0, 4096, 32)])
    assert pick.size == 256
    dev = H.dev_view(N, par)
    states, nv = _open_lists(dev, v1[pick, :G], v1[pick, G:], 32)
    Hs, _ = TH.hamiltonians(dev, v1[pick, :G], v1[pick, G:], states, nv)
    assert len(set(nv.tolist())) > 1, "every picked list has the same length"
    flat = {k: _np(one[k]).reshape((R * R,) + _np(one[k]).shape[3:])[pick] for k in ("occupations", "variance", "ztail")}
    TH.compare_points(f"second trip N={N} R={R}", Hs, states, nv, KT_100K, flat["occupations"], flat["variance"], flat["ztail"])
    env.close()


# ------------------------------------------------------------------ 7. slots, launch chunks, guard rows
def _raw_call(env, ids, dirs, rg, gv, bv, kT, nq, nx, ny, dst, n_charge=None, flags=0, topts_size=None, opts_size=None):
    import torch
    from qadapt_hip import _lib
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dt)).cuda()      # noqa: E731
    keep = [t(ids, np.int32), t(dirs, np.float64), t(rg, np.float64), t(gv, np.float64), t(bv, np.float64),
            None if kT is None else t(kT, np.float64), None if n_charge is None else t(n_charge, np.int32)]
    addr = lambda x: None if x is None else x.data_ptr()                        # noqa: E731
    o = _lib.QdScanGridOpts(struct_size=ctypes.sizeof(_lib.QdScanGridOpts) if opts_size is None else opts_size, frame=_lib.QD_SCAN_PHYSICAL,
                            noise_flags=flags, serial=(1 << 63) | 5, occ_dst=addr(dst.get("occupations")))
    to = _lib.QdGridThermalOpts(struct_size=ctypes.sizeof(_lib.QdGridThermalOpts) if topts_size is None else topts_size,
                                n_charge_dev=addr(keep[6]), var_dst=addr(dst.get("variance")), ztail_dst=addr(dst.get("ztail")))
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())          # noqa: E731
    rc = env._lib.qd_scan_grid_thermal(env._h, p(keep[0]), nq, nx, ny, p(keep[1]), p(keep[2]), p(keep[3]), p(keep[4]), None, p(keep[5]),
                                       p(dst.get("raw")), p(dst.get("image")), p(dst.get("plohi")), ctypes.byref(o), ctypes.byref(to),
                                       env._stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("nq", [1, 2, 5])
def test_slots_chunks_inert_queries_and_guard_rows(tmp_path, nq):
    """a 4-dot 8 x 8 handle with env_chunk = 2 holds 6 slots of 36 records (test_gpu_scan_grid._slots): nq + 2 queries, two of them
    with env ids outside [0, B), through the C entry point with guard rows on both sides of every destination.  Every live query
    has the bits of the same query alone (a kT of its own each), the inert ones leave their rows untouched, the guards stay"""
    import torch
    N, R, B, seed = 4, 8, 3, 9600
    nx, ny = 9, 4
    n, G = nx * ny, N + 1
    env = _vec(tmp_path, B, N, R, seed, env_chunk=2)
    assert env.chunk_envs() == 2
    rng = np.random.default_rng(seed + nq)
    params, state = _placed_blocks(N, [seed, seed + 1, seed + 2], ("near", "mid", "near"), rng)
    _load(env, params, state)
    tot = nq + 2
    ids = np.array({1: [B, 1, -3], 2: [0, B, 2, -1], 5: [0, B, 2, 1, -1, 2, 0]}[nq], np.int32)
    live = (ids >= 0) & (ids < B)
    assert live.sum() == nq
    envs = np.clip(ids, 0, B - 1)
    qs = [_query(N, params[e], state[e], "physical", rng) for e in envs]
    dirs = np.stack([np.stack([q[0], q[1]]) for q in qs])
    rg = np.array([[*q[2], *q[3]] for q in qs])
    gv, bv = np.stack([q[4][:N] for q in qs]), np.stack([q[4][G:] for q in qs])
    kT = KT_100K * (1.0 + 0.37 * np.arange(tot))
    g0, g1, guard = 2, 3, -12345.678
    full = lambda *s: torch.full(s, guard, dtype=torch.float64, device="cuda")     # noqa: E731

    def buffers(rows):
        d = dict(raw=full(rows, ny, nx), plohi=full(rows, 2), occupations=full(rows, ny, nx, N), variance=full(rows, ny, nx, N),
                 ztail=full(rows, ny, nx))
        d["image"] = torch.full((rows, ny, nx), -7.0, dtype=torch.float32, device="cuda")
        return d

    big = buffers(g0 + tot + g1)
    view = {k: v[g0:] for k, v in big.items()}
    # (the sensor gate of the raw call is NULL: 0.0 for every query)
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
    env.close()


# ------------------------------------------------------------------ 8. nothing else moves
def test_thermal_grids_leave_no_footprint(tmp_path):
    """scan_grid at T = 0 and eval_points(kT=) give the same bits before and after thermal grids on the same handle, two identical
    thermal grids give the same bits, and one step() of a handle that rendered thermal grids equals that of its twin that did not"""
    import torch
    N, R, B, seed = 4, 8, 2, 9700
    plain, poked = [_vec(tmp_path, B, N, R, seed) for _ in range(2)]
    obs0 = [env.reset(seed=seed) for env in (plain, poked)]
    L = layout(N)
    st, _ = poked.get_state()
    gv, bv = st[:, L.s_gate_gt:L.s_gate_gt + N], st[:, L.s_barrier_gt:L.s_barrier_gt + N - 1]
    vg, vb = CH.points(N, np.random.default_rng(seed), 40)
    cold = lambda: poked.scan_grid([0, 1], "e1_2", "U1_2", (-2, 2), (1, -1), 9, 5, gv, bv, occupations=True)      # noqa: E731
    pts = lambda: poked.eval_points([0, 1], np.stack([vg, vg]), np.stack([vb, vb]), kT=[0.01, 0.3],                 # noqa: E731
                                    outputs=("signal", "occupations", "variance", "ztail"))
    hot = lambda **kw: poked.scan_grid_thermal([1, 0], "e1_2", "U1_2", (-2, 2), (1, -1), 9, 5, gv[::-1], bv[::-1], [0.01, 0.3],   # noqa: E731
                                               occupations=True, variance=True, ztail=True, **kw)
    before, before_p = cold(), pts()
    t1, t2 = hot(), hot()
    t3 = poked.scan_grid_thermal([1, 0], "vP1", "vP2", (-2, 2), (1, -1), 7, 3, gv, bv, 0.05, n_charge=3, occupations=True, variance=True)
    t4 = hot(noise=("sensor",), serial=(1 << 63) | 3)
    for key in t1:
        assert PH.same(t1[key], t2[key]), key
        assert np.isfinite(_np(t1[key])).all(), key
    assert np.isfinite(_np(t3["raw"])).all() and np.all(np.abs(_np(t3["occupations"]).sum(axis=-1) - 3.0) <= 1e-9)
    assert PH.same(t4["occupations"], t1["occupations"]) and not PH.same(t4["raw"], t1["raw"])
    assert not PH.same(before["occupations"], t1["occupations"][[1, 0]])                     # the temperature does something
    after, after_p = cold(), pts()
    for a, b in ((before, after), (before_p, after_p)):
        assert a.keys() == b.keys()
        for key in a:
            assert PH.same(a[key], b[key]), key
    act = torch.as_tensor(np.random.default_rng(13).uniform(-1, 1, (B, 2 * N - 1)).astype(np.float32)).cuda()
    res = []
    for env in (plain, poked):
        obs, rew, term, trunc = env.step(act)
        stt, steps = env.get_state()
        res.append(dict(image=_np(obs["image"]).copy(), gv=_np(obs["obs_gate_voltages"]).copy(), bv=_np(obs["obs_barrier_voltages"]).copy(),
                        rew=_np(rew).copy(), raw=env.raw()[0].copy(), plohi=env.raw()[1].copy(), state=stt, steps=steps,
                        params=env._params_host.copy()))
    for key in res[0]:
        assert PH.same(res[0][key], res[1][key]), key
    del obs0
    plain.close(); poked.close()


# ------------------------------------------------------------------ 9. refusals and the facade
def test_refusals(tmp_path):
    import torch
    from qadapt_hip import _lib
    N, R = 3, 8
    q = DM.load_yaml(None, "qarray_config.yaml")
    q["simulator"]["model"]["max_charge_carriers"] = 2
    qp = tmp_path / "qarray_m2.yaml"
    qp.write_text(yaml.safe_dump(q))
    gv, bv = np.zeros((1, N)), np.zeros((1, N - 1))
    grid = lambda env, kT, **kw: env.scan_grid_thermal([0], "e1_2", "vP3", (-1, 1), (-1, 1), 8, 2, gv, bv, kT, **kw)      # noqa: E731
    for kw, word in ((dict(validate=True), "QD_FLAG_VALIDATE"),
                     (dict(num_charge_states="all", qarray_config_path=str(qp)), "full charge-state space")):
        env = _vec(tmp_path, 1, N, R, 77, **kw)
        env.reset(seed=77)
        raw0 = env.raw()[0].copy()
        with pytest.raises(_lib.QdError, match=word) as ei:
            grid(env, 0.01)
        assert f"code {_lib.QD_ERR_STATE}" in str(ei.value) and "qd_scan_grid_thermal" in str(ei.value)
        assert PH.same(env.raw()[0], raw0)
        env.close()
    env = _vec(tmp_path, 1, N, R, 78, noise=("sensor", "latch"))          # (so that noise=True names the latching stage)
    env.reset(seed=78)
    for bad in (0.0, -0.01, float("inf"), float("nan"), [float("nan")]):
        with pytest.raises(ValueError, match="kT"):
            grid(env, bad)
    with pytest.raises(ValueError, match="kT"):
        grid(env, None, variance=True)
    for kw in (dict(kT=0.01), dict(variance=True), dict(ztail=True)):                          # the T = 0 calls are as they were
        with pytest.raises(TypeError):
            env.scan_grid([0], "e1_2", "vP3", (-1, 1), (-1, 1), 8, 2, gv, bv, **kw)
        with pytest.raises(TypeError):
            env.scan_grid_closed([0], "e1_2", "vP3", (-1, 1), (-1, 1), 8, 2, gv, bv, 2, **kw)
    with pytest.raises(ValueError, match="closed regime"):
        grid(env, 0.01, n_charge=2, noise=("sensor",))
    for noise in (("latch",), ("sensor", "latch"), True):
        with pytest.raises(ValueError, match="latch"):
            grid(env, 0.01, noise=noise)
    before = grid(env, 0.02, variance=True, ztail=True, occupations=True)
    # the C entry point: what only the device can tell (a bad kT is read back from it), and the checks that come before
    d = np.stack([np.eye(2 * N)[0], np.eye(2 * N)[1]])[None]
    rg = [[-1, 1, -1, 1]]
    dst = dict(raw=torch.full((1, 2, 8), -5.0, dtype=torch.float64, device="cuda"),
               variance=torch.full((1, 2, 8, N), -5.0, dtype=torch.float64, device="cuda"))
    size_t, size_o = ctypes.sizeof(_lib.QdGridThermalOpts), ctypes.sizeof(_lib.QdScanGridOpts)
    cases = [(dict(kT=[bad]), "kT") for bad in (0.0, -1.0, float("nan"), float("inf"))]
    cases += [(dict(kT=None), "kT_dev"), (dict(kT=[0.02], topts_size=size_t - 8), "struct_size"),
              (dict(kT=[0.02], opts_size=size_o - 8), "struct_size"), (dict(kT=[0.02], flags=_lib.QD_NOISE_LATCH), "QD_NOISE_LATCH"),
              (dict(kT=[0.02], flags=_lib.QD_NOISE_SENSOR, n_charge=[2]), "closed regime"),
              (dict(kT=[0.02], n_charge=[-1]), "0..32767"), (dict(kT=[0.02], n_charge=[32768]), "0..32767")]
    for kw, word in cases:
        rc = _raw_call(env, [0], d, rg, gv, bv, kw.pop("kT"), 1, 8, 2, dst, **kw)
        msg = env._lib.qd_last_error(env._h).decode()
        assert rc == _lib.QD_ERR_ARG and msg.startswith("qd_scan_grid_thermal") and word in msg, (kw, rc, msg)
        assert all(np.all(t.cpu().numpy() == -5.0) for t in dst.values())
        after = grid(env, 0.02, variance=True, ztail=True, occupations=True)               # the handle is usable
        for key in before:
            assert PH.same(before[key], after[key]), (word, key)
    # two queries, the second kT bad: every query's is checked
    rc = _raw_call(env, [0, 0], np.tile(d, (2, 1, 1)), rg * 2, np.tile(gv, (2, 1)), np.tile(bv, (2, 1)), [0.02, 0.0], 2, 8, 2, {})
    assert rc == _lib.QD_ERR_ARG and "kT" in env._lib.qd_last_error(env._h).decode()
    env.close()


def test_facade_thermal_grids(tmp_path):
    """do2d_thermal and do1d_thermal against thermal_state_open / thermal_state_closed at the same points, within the sum of both
    tolerances (the grid and the points run different solvers), and against the backend's scan_grid_thermal bit for bit"""
    from qadapt_hip.env import QuantumDeviceEnv
    N, R = 3, 8
    path = _cfg(tmp_path, num_dots=N, resolution=R)
    backend = _vec(tmp_path, 1, N, R, 9900, config_path=path)
    env = QuantumDeviceEnv(config_path=path, num_dots=N, backend=backend)
    model = env.array.model
    T = float(backend.last_episode.extras["T"][0])
    assert 50.0 <= T <= 200.0 and model.T == T
    par = backend._params_host[0]
    L, G = layout(N), N + 1
    dev = H.dev_view(N, par)
    p0 = par[L.vopt:L.vopt + G]
    nx, ny = 7, 5
    xs, ys = np.linspace(p0[0] - 3, p0[0] + 3, nx), np.linspace(p0[1] + 2, p0[1] - 2, ny)
    sig, occ, var = model.do2d_thermal("P1", xs[0], xs[-1], nx, "P2", ys[0], ys[-1], ny)
    assert sig.shape == (ny, nx, 1) and occ.shape == var.shape == (ny, nx, N) and sig.dtype == occ.dtype == var.dtype == np.float64
    want = backend.scan_grid_thermal([0], 0, 1, (xs[0], xs[-1]), (ys[0], ys[-1]), nx, ny, np.zeros((1, N)), np.zeros((1, N - 1)),
                                     TH.KB_REF * T, 0.0, frame="physical", gamma=float(model.coulomb_peak_width), occupations=True,
                                     variance=True)
    assert PH.same(sig[:, :, 0], want["raw"][0]) and PH.same(occ, want["occupations"][0]) and PH.same(var, want["variance"][0])
    vg = np.zeros((ny, nx, G)); vg[:, :, 0] = xs[None, :]; vg[:, :, 1] = ys[:, None]
    vb = np.zeros((ny, nx, N - 1))
    kT = TH.KB_REF * T
    flat_g, flat_b = vg.reshape(-1, G), vb.reshape(-1, N - 1)
    states, nv = _open_lists(dev, flat_g, flat_b, 32)
    Hs, _ = TH.hamiltonians(dev, flat_g, flat_b, states, nv)
    tol = np.array([2 * TH.tol_occ(Hm, kT, max(float(states[p, :nv[p]].max()), 1.0)) for p, Hm in enumerate(Hs)]).reshape(ny, nx)

    def close_to(got, ref):
        s, o, v = got
        rs, ro, rv = ref
        n_max = max(float(states.max()), 1.0)
        assert np.all(np.abs(o - ro).max(axis=-1) <= tol) and np.all(np.abs(v - rv).max(axis=-1) <= n_max * tol)
        assert np.allclose(s, rs, rtol=1e-9, atol=1e-12)

    close_to((sig, occ, var), model.thermal_state_open(vg, vb))
    hot = model.do2d_thermal("P1", xs[0], xs[-1], nx, "P2", ys[0], ys[-1], ny, T=4 * T)
    assert not PH.same(hot[1], occ) and np.all(var >= 0)
    assert all(PH.same(a, b) for a, b in zip((sig, occ, var), model.do2d_thermal("P1", xs[0], xs[-1], nx, "P2", ys[0], ys[-1], ny, T=T)))
    # one row
    s1, o1, v1 = model.do1d_thermal("P1", xs[0], xs[-1], nx, T=T)
    assert s1.shape == (nx, 1) and o1.shape == v1.shape == (nx, N)
    g1 = np.zeros((nx, G)); g1[:, 0] = xs
    r1 = model.thermal_state_open(g1, np.zeros((nx, N - 1)), T=T)
    st1, nv1 = _open_lists(dev, g1, np.zeros((nx, N - 1)), 32)
    H1, _ = TH.hamiltonians(dev, g1, np.zeros((nx, N - 1)), st1, nv1)
    t1 = np.array([2 * TH.tol_occ(Hm, kT, max(float(st1[p, :nv1[p]].max()), 1.0)) for p, Hm in enumerate(H1)])
    assert np.all(np.abs(o1 - r1[1]).max(axis=-1) <= t1) and np.all(np.abs(v1 - r1[2]).max(axis=-1) <= max(float(st1.max()), 1.0) * t1)
    assert np.allclose(s1, r1[0], rtol=1e-9, atol=1e-12)
    # closed
    s2, o2, v2 = model.do2d_thermal("P1", xs[0], xs[-1], nx, "P2", ys[0], ys[-1], ny, T=T, n_charge=2)
    assert np.all(np.abs(o2.sum(axis=-1) - 2.0) <= 1e-9)
    r2 = model.thermal_state_closed(vg, 2, T=T, vb=vb)
    host = CH.host_closed(N, par, np.concatenate([flat_g, flat_b], axis=1), 2, 32)
    nv2 = np.minimum(host["nvalid"], 32)
    H2, _ = TH.hamiltonians(dev, flat_g, flat_b, host["states"], nv2)
    t2 = np.array([2 * TH.tol_occ(Hm, kT, 2.0) for Hm in H2]).reshape(ny, nx)
    assert np.all(np.abs(o2 - r2[1]).max(axis=-1) <= t2) and np.all(np.abs(v2 - r2[2]).max(axis=-1) <= 2.0 * t2)
    assert np.allclose(s2, r2[0], rtol=1e-9, atol=1e-12)
    s3, o3, v3 = model.do1d_thermal("P2", ys[0], ys[-1], ny, T=T, n_charge=2)
    assert s3.shape == (ny, 1) and np.all(np.abs(o3.sum(axis=-1) - 2.0) <= 1e-9)
    with pytest.raises(NotImplementedError):
        model.do2d_thermal("P1", 0, 1, 3, "vP2", 0, 1, 3)
    # env.array.scan_grid_thermal: one query, the keywords handed through
    out = env.array.scan_grid_thermal(0, 1, (xs[0], xs[-1]), (ys[0], ys[-1]), nx, ny, np.zeros(N), np.zeros(N - 1), kT, 0.0,
                                      frame="physical", gamma=float(model.coulomb_peak_width), occupations=True, variance=True, ztail=True)
    assert PH.same(out["occupations"], occ) and out["ztail"].shape == (ny, nx) and PH.same(out["variance"], var)
    env.close()
