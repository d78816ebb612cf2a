"""Energy levels on grids on the MI355X (run with -m gpu): qd_scan_grid_levels / scan_grid_levels(..., levels=L, n_charge=...)
against eigvalsh of the oracle's Hamiltonian on its kept list cut to the nv valid states (test_gpu_levels._spectrum) at EVERY
point of every grid, at the voltages of the host build of the grid front end (tests/grid_helpers.py); the closed lists, the
per-point route, the image bits against scan_grid / scan_grid_closed, designed scenes, more than one point per block, slots
and launch chunks with guard rows, the absent footprint, the refusals and the facade.

Bound everywhere: |level - eigvalsh| <= 1e-12 ||H||_inf of the oracle's matrix, ||H||_inf itself within rtol 1e-14, +inf exactly
from level nv on, levels non-decreasing (test_gpu_levels._compare, as it is).  In the open regime the kernel
(csrc/qd_levels_blocks.h) tridiagonalises each hop component by itself and is NOT bitwise equal to eval_points(levels=), which
works on the whole block (csrc/qd_levels.h): the two are compared within the sum of both bars, 2e-12 hnorm.  A closed list is
one component and runs the whole-block core: bit for bit the points, in the physical frame."""
import ctypes

import numpy as np
import pytest
import yaml

import closed_helpers as CH
import helpers as H
import points_helpers as PH
import qd_oracle as O
import search_cases as SC
from qadapt_hip import device_model as DM
from qadapt_hip.layout import layout
from test_gpu_levels import BAR, _cfg, _compare, _load, _np, _open_lists, _spectrum, _vec
from test_gpu_thermal_grid import _physical_point, _placed_blocks, _query, _voltages

pytestmark = pytest.mark.gpu


def _scan(env, ids, qs, nx, ny, frame, levels, closed=None, **kw):
    N, G = env.N, env.N + 1
    args = ([list(ids), np.stack([q[0] for q in qs]), np.stack([q[1] for q in qs]), [q[2] for q in qs], [q[3] for q in qs], nx, ny,
             np.stack([q[4][:N] for q in qs]), np.stack([q[4][G:] for q in qs])])
    sv = np.array([q[4][N] for q in qs])
    return env.scan_grid_levels(*args, sv, levels=levels, n_charge=closed, frame=frame, **kw)


def _plain(env, ids, qs, nx, ny, frame, closed=None, **kw):
    """the same queries through scan_grid / scan_grid_closed"""
    N, G = env.N, env.N + 1
    args = ([list(ids), np.stack([q[0] for q in qs]), np.stack([q[1] for q in qs]), [q[2] for q in qs], [q[3] for q in qs], nx, ny,
             np.stack([q[4][:N] for q in qs]), np.stack([q[4][G:] for q in qs])])
    sv = np.array([q[4][N] for q in qs])
    if closed is None:
        return env.scan_grid(*args, sv, frame=frame, **kw)
    return env.scan_grid_closed(*args, closed, sv, frame=frame, **kw)


def _derived(out, q, n):
    """gap and rel_gap of query q are what the docstring says they are"""
    lev, hn = _np(out["levels"][q]).reshape(n, -1), _np(out["hnorm"][q]).reshape(n)
    gap, rel = _np(out["gap"][q]).reshape(n), _np(out["rel_gap"][q]).reshape(n)
    assert PH.same(gap, lev[:, 1] - lev[:, 0]) and PH.same(rel, gap / hn)
    assert np.array_equal(np.isposinf(gap), np.isposinf(lev[:, 1])) and not np.isnan(gap).any()


# ------------------------------------------------------------------ 1. oracle parity, open
@pytest.mark.parametrize("frame", ["virtual", "physical"])
@pytest.mark.parametrize("N,K", [(2, 32), (4, 32), (8, 32), (2, 8), (4, 8), (8, 8)])
def test_open_parity(tmp_path, N, K, frame):
    """R = 8 (P = 64), one env near and two mid (helpers.place); the grids 7 x 5, 16 x 1, 1 x 1 and 8 x 8 = P, one query per env in
    one call, L = 8 and L = 2 alternating.  No env is placed far: tc = tc_base exp(-a), the device and NumPy sum the N + 2
    products of a in different orders, and that round-off of a is a relative error of tc, and of hnorm where the couplings are
    the norm, of up to (N + 2) eps |a| -- 1e-13 at 8 dots and |a| = 45, where the flat 1e-14 of _compare cannot be promised for
    any code (test_gpu_levels.test_large_couplings has that case, with a provision this file does not take over).  Within 6 V of
    the barriers' ground truth |a| stays of order 10."""
    rng = np.random.default_rng(9800 + 10 * N + K + 1000 * (frame == "physical"))
    params, state = _placed_blocks(N, [41, 42, 43], ("near", "mid", "mid"), rng)
    env = _vec(tmp_path, 3, N, 8, 41, num_charge_states=K)
    _load(env, params, state)
    for i, (nx, ny) in enumerate([(7, 5), (16, 1), (1, 1), (8, 8)]):
        nl = (8, 2)[i % 2]
        qs = [_query(N, params[e], state[e], frame, rng) for e in range(3)]
        out = _scan(env, [0, 1, 2], qs, nx, ny, frame, nl)
        assert out["levels"].shape == (3, ny, nx, nl) and out["hnorm"].shape == out["gap"].shape == out["rel_gap"].shape == (3, ny, nx)
        for e, mode in enumerate(("near", "mid", "mid")):
            dev = H.dev_view(N, params[e])
            v = _voltages(N, params[e], state[e], qs[e], nx, ny, frame)
            states, nv = _open_lists(dev, v[:, :N + 1], v[:, N + 1:], K)
            lev_ref, hn_ref, tc = _spectrum(dev, v[:, :N + 1], v[:, N + 1:], states, nv, n_levels=nl)
            _compare(f"grid open N={N} K={K} {frame} {nx}x{ny} L={nl} {mode} (tc up to {tc.max():.1e})", out["levels"][e], out["hnorm"][e],
                     lev_ref, hn_ref)
            _derived(out, e, nx * ny)
    env.close()


# ------------------------------------------------------------------ 2. oracle parity, closed; 3. the per-point route
@pytest.mark.parametrize("N", [2, 4, 8])
def test_closed_parity_and_the_bits_of_the_points(tmp_path, N):
    """three envs, a total charge per query, the kept lists of the host build of the sector search (closed_helpers), as
    test_gpu_levels.test_closed_levels_against_the_sector_lists; in the physical frame the levels and norms are those of
    eval_points(levels=, n_charge=) at the grid's voltages bit for bit"""
    seed = 9810 + N
    rng = np.random.default_rng(seed)
    params, state = _placed_blocks(N, [seed, seed + 1, seed + 2], ("near", "mid", "near"), rng)
    env = _vec(tmp_path, 3, N, 8, seed)
    _load(env, params, state)
    Qv = [1, N, N + 2]
    for frame, (nx, ny), nl in (("physical", (7, 5), 8), ("virtual", (16, 1), 3), ("physical", (8, 8), 2)):
        qs = [_query(N, params[e], state[e], frame, rng) for e in range(3)]
        out = _scan(env, [0, 1, 2], qs, nx, ny, frame, nl, closed=Qv)
        for e, Q in enumerate(Qv):
            dev = H.dev_view(N, params[e])
            v = _voltages(N, params[e], state[e], qs[e], nx, ny, frame)
            host = CH.host_closed(N, params[e], v, Q, 32)
            nv = np.minimum(host["nvalid"], 32)
            lev_ref, hn_ref, _ = _spectrum(dev, v[:, :N + 1], v[:, N + 1:], host["states"], nv, n_levels=nl)
            _compare(f"grid closed N={N} Q={Q} {frame} {nx}x{ny} L={nl}", out["levels"][e], out["hnorm"][e], lev_ref, hn_ref)
            if Q == 1:
                assert nv.max() <= N
            if frame == "physical":
                pts = env.eval_points([e], v[None, :, :N + 1], v[None, :, N + 1:], n_charge=Q, outputs=(), levels=nl)
                assert PH.same(_np(out["levels"][e]).reshape(nx * ny, nl), pts["levels"][0]), (Q, nx, ny)
                assert PH.same(_np(out["hnorm"][e]).reshape(nx * ny), pts["hnorm"][0]), (Q, nx, ny)
    env.close()


@pytest.mark.parametrize("N,K", [(4, 32), (8, 32), (8, 8)])
def test_open_grid_against_eval_points(tmp_path, N, K):
    """scan_grid_levels in the physical frame against eval_points(levels=) at the grid's voltages: within 2e-12 hnorm at every
    point, hnorm bit for bit (the same function of the same record)"""
    rng = np.random.default_rng(9820 + N + K)
    params, state = _placed_blocks(N, [42, 43], ("mid", "far"), rng)
    env = _vec(tmp_path, 2, N, 8, 42, num_charge_states=K)
    _load(env, params, state)
    nx, ny = 7, 9
    qs = [_query(N, params[e], state[e], "physical", rng) for e in range(2)]
    for nl in (2, 8):
        out = _scan(env, [0, 1], qs, nx, ny, "physical", nl)
        for e in range(2):
            v = _voltages(N, params[e], state[e], qs[e], nx, ny, "physical")
            pts = env.eval_points([e], v[None, :, :N + 1], v[None, :, N + 1:], outputs=(), levels=nl)
            a, b = _np(out["levels"][e]).reshape(nx * ny, nl), _np(pts["levels"][0])
            hn = _np(pts["hnorm"][0])
            assert PH.same(_np(out["hnorm"][e]).reshape(-1), hn)
            assert np.array_equal(np.isposinf(a), np.isposinf(b))
            fin = np.isfinite(b)
            d = np.where(fin, np.abs(np.where(fin, a, 0.0) - np.where(fin, b, 0.0)), 0.0) / hn[:, None]
            same = int((a.view(np.uint64) == b.view(np.uint64)).all(axis=1).sum())
            print(f"[levels grid] against eval_points N={N} K={K} L={nl} env {e}: worst difference / hnorm {d.max():.2e}; {same} of "
                  f"{nx * ny} points bitwise equal")
            assert np.all(d <= 2e-12)
    env.close()


# ------------------------------------------------------------------ 4. the image bits
def test_image_bits_are_those_of_scan_grid(tmp_path):
    """raw, image, plohi and occupations of scan_grid_levels are those of scan_grid / scan_grid_closed under the same arguments,
    deterministic and with sensor noise and latching under the same serial and stream base; the levels do not see the noise"""
    N, R, seed, serial, base = 4, 8, 9830, (1 << 63) | 23, 77
    rng = np.random.default_rng(seed)
    params, state = _placed_blocks(N, [seed, seed + 1], ("near", "mid"), rng)
    env = _vec(tmp_path, 2, N, R, seed, noise=("sensor", "latch"))
    _load(env, params, state)
    nx, ny = 9, 5
    keys = ("raw", "image", "plohi", "occupations")
    for frame in ("virtual", "physical"):
        qs = [_query(N, params[e], state[e], frame, rng) for e in range(2)]
        clean = _scan(env, [0, 1], qs, nx, ny, frame, 8, occupations=True)
        want = _plain(env, [0, 1], qs, nx, ny, frame, occupations=True)
        for k in keys:
            assert PH.same(clean[k], want[k]), (frame, k)
        for noise in (("sensor",), ("sensor", "latch"), True):
            noisy = _scan(env, [0, 1], qs, nx, ny, frame, 8, occupations=True, noise=noise, serial=serial, stream_base=base)
            nwant = _plain(env, [0, 1], qs, nx, ny, frame, occupations=True, noise=noise, serial=serial, stream_base=base)
            for k in keys:
                assert PH.same(noisy[k], nwant[k]), (frame, noise, k)
            assert not PH.same(noisy["raw"], clean["raw"])
            for k in ("levels", "hnorm", "gap", "rel_gap"):
                assert PH.same(noisy[k], clean[k]), (frame, noise, k)
        Qv = [2, N + 1]
        closed = _scan(env, [0, 1], qs, nx, ny, frame, 3, closed=Qv, occupations=True)
        cwant = _plain(env, [0, 1], qs, nx, ny, frame, closed=Qv, occupations=True)
        for k in keys:
            assert PH.same(closed[k], cwant[k]), (frame, "closed", k)
        # without the occupations, and again: the same bits
        bare = _scan(env, [0, 1], qs, nx, ny, frame, 8)
        assert "occupations" not in bare and all(PH.same(bare[k], clean[k]) for k in ("raw", "image", "plohi", "levels", "hnorm"))
    env.close()


# ------------------------------------------------------------------ 5. designed scenes
def test_two_level_detuning_line(tmp_path):
    """2 dots, one carrier, a 33 x 1 grid along e1_2 in the virtual frame: H = [[E_10, -t], [-t, E_01]] and the gap is
    sqrt(eps^2 + 4 t^2), within 1e-12 hnorm (the tolerance of test_gpu_levels.test_two_level_anticrossing)"""
    from qadapt_hip.vec_env import scan_axis_vectors
    N, seed, n = 2, 8200, 33
    L = layout(N)
    env = _vec(tmp_path, 1, N, 8, seed)
    env.reset(seed=seed)
    par = env._params_host[0].copy()
    st = env.get_state()[0][0]
    dev = H.dev_view(N, par)
    W0 = np.concatenate([st[L.s_gate_gt:L.s_gate_gt + N], [st[L.s_sensor_gt]], par[L.vbopt:L.vbopt + 1]])
    out = env.scan_grid_levels([0], "e1_2", np.zeros(2 * N), (-0.6, 0.6), (0.0, 0.0), n, 1, W0[None, :N], W0[None, N + 1:], W0[N],
                               levels=3, n_charge=1)
    q = (scan_axis_vectors("e1_2", N, "virtual", 1)[0], np.zeros(2 * N), (-0.6, 0.6), (0.0, 0.0), W0)
    v = _voltages(N, par, st, q, n, 1, "virtual")
    vg, vb = v[:, :N + 1], v[:, N + 1:]
    lev, hn, gap = _np(out["levels"])[0, 0], _np(out["hnorm"])[0, 0], _np(out["gap"])[0, 0]
    stt = np.broadcast_to(np.array([[1, 0], [0, 1]]), (n, 2, 2))
    F = O.free_energy_states(v, dev.cdd_inv_full, dev.cgd_full, stt, N)
    t = O.tunnel_couplings(O.effective_barrier_potential(vg, vb, dev.Cbg, dev.Cbb), dev.tc_base, dev.alpha)[:, 0]
    eps = F[:, 0] - F[:, 1]
    gap_ref = np.sqrt(eps ** 2 + 4 * t ** 2)
    hn_ref = np.abs(F).max(axis=1) + t
    err = np.abs(gap - gap_ref) / hn_ref
    print(f"[levels grid] detuning line: eps {eps.min():.3e}..{eps.max():.3e}, t {t.min():.3e}..{t.max():.3e}, "
          f"worst |gap - sqrt(eps^2 + 4 t^2)| / hnorm {err.max():.2e}")
    assert np.ptp(eps) > 0 and np.all(err <= BAR) and np.all(np.isposinf(lev[:, 2])) and np.all(np.abs(hn - hn_ref) <= 1e-14 * hn_ref)
    assert PH.same(gap, lev[:, 1] - lev[:, 0])
    env.close()


def test_all_couplings_zero_gives_the_sorted_energies(tmp_path):
    """tc_base = 0: every state a component of its own, the levels are the sorted oracle energies of the valid kept states"""
    N, seed = 4, 8300
    L = layout(N)
    rng = np.random.default_rng(seed)
    params, state = _placed_blocks(N, [seed], ("mid",), rng)
    params[0, L.scal] = 0.0
    env = _vec(tmp_path, 1, N, 8, seed)
    _load(env, params, state)
    dev = H.dev_view(N, params[0])
    for frame, (nx, ny) in (("physical", (8, 8)), ("virtual", (7, 5))):
        q = _query(N, params[0], state[0], frame, rng)
        out = _scan(env, [0], [q], nx, ny, frame, 8)
        v = _voltages(N, params[0], state[0], q, nx, ny, frame)
        states, nv = _open_lists(dev, v[:, :N + 1], v[:, N + 1:], 32)
        lev_ref, hn_ref, tc = _spectrum(dev, v[:, :N + 1], v[:, N + 1:], states, nv)
        assert not tc.any()
        F = np.sort(O.free_energy_states(v, dev.cdd_inv_full, dev.cgd_full, states.astype(np.int64), N), axis=1)
        full = nv == 32
        assert full.any() and np.allclose(lev_ref[full], F[full, :8], rtol=0, atol=1e-12 * hn_ref[full, None])
        _compare(f"grid, all couplings zero, {frame}", out["levels"][0], out["hnorm"][0], lev_ref, hn_ref)
    env.close()


def test_mirror_symmetric_device_has_bitwise_equal_pairs(tmp_path):
    """A designed 4-dot device (search_cases.build: cdd_inv = I / 4, cgd = [I 0], dyadic voltages, so every energy is exact) that
    is its own mirror image: plungers at (1.5, 1.25, 1.25, 1.5) + x, the outer barriers at 800 V (tc[0] and tc[2] underflow to
    exactly 0), the middle one coupled.  Only dots 1 and 2 exchange carriers, so a component is (a; n_1 + n_2; d) with the outer
    occupations a, d frozen, and its mirror image is (d; n_1 + n_2; a).  The energies are sums over the dots and dots 0 and 3
    sit at the same voltage, so the two components hold equal energies and equal couplings in the same local order (the order
    of the middle digits): their tridiagonals are equal bit for bit and every level of one is a level of the other --
    degenerate pairs, bitwise equal.  (With the MIDDLE barrier cut instead, a component is a product of two chains, equal
    energies occur inside it, and the index order of such ties is not mirror-symmetric: the pairs then agree to an ulp only.)"""
    N, R = 4, 8
    L = layout(N)
    gates = np.array([1.5, 1.25, 1.25, 1.5])
    par, st = SC.build(dict(r=0.0, gate=gates, step=1 / 8, zero_cbg=True), N, R, tc_base=0.05)
    par[L.alpha:L.alpha + N - 1] = 1.0
    env = _vec(tmp_path, 1, N, R, 9840)
    _load(env, par[None], st[None])
    dev = H.dev_view(N, par)
    n = 5
    dx = np.concatenate([np.ones(N), np.zeros(N)])
    vbar = np.array([800.0, 0.0, 800.0])
    out = env.scan_grid_levels([0], dx, np.zeros(2 * N), (-0.25, 0.25), (0.0, 0.0), n, 1, gates[None], vbar[None], 0.25, levels=8,
                               frame="physical")
    v = _voltages(N, par, st, (dx, np.zeros(2 * N), (-0.25, 0.25), (0.0, 0.0), np.concatenate([gates, [0.25], vbar])), n, 1, "physical")
    assert np.array_equal(v[:, :N], gates[None, :] + np.linspace(-0.25, 0.25, n)[:, None])
    states, nv = _open_lists(dev, v[:, :N + 1], v[:, N + 1:], 32)
    lev_ref, hn_ref, tc = _spectrum(dev, v[:, :N + 1], v[:, N + 1:], states, nv)
    assert np.all(tc[:, 0] == 0.0) and np.all(tc[:, 2] == 0.0) and np.all(tc[:, 1] > 0)
    _compare("mirror-symmetric device", out["levels"][0], out["hnorm"][0], lev_ref, hn_ref)
    lev = _np(out["levels"])[0, 0]
    pairs = 0
    for p in range(n):
        for k in range(7):
            if abs(lev_ref[p, k + 1] - lev_ref[p, k]) <= 1e-13 * hn_ref[p]:        # equal by symmetry: eigvalsh splits them by round-off
                assert lev[p, k] == lev[p, k + 1], (p, k, lev[p])
                pairs += 1
    print(f"[levels grid] mirror-symmetric device: {pairs} degenerate pairs among the 8 lowest levels of {n} points, all bitwise equal")
    assert pairs >= n
    env.close()


# ------------------------------------------------------------------ 6. more than one point per block
def test_second_point_of_a_block_keeps_nothing_from_the_first(tmp_path):
    """3 dots on an R = 72 handle: one grid of 72 x 72 = 5184 points has more points than the 4096 blocks of its slot, so 1088
    blocks solve a second point on the workspace of the first; two grids of 72 x 36 over the same points have one point per
    block.  Levels, hnorm and raw bit for bit, and 256 of the points against the reference"""
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
    whole = (ux, uy, (-12.0, 12.0), (ys[0], ys[-1]), W0)
    halves = [(ux, uy, (-12.0, 12.0), (ys[0], ys[R // 2 - 1]), W0), (ux, uy, (-12.0, 12.0), (ys[R // 2], ys[-1]), W0)]
    one = _scan(env, [0], [whole], R, R, "physical", 8)
    two = _scan(env, [0, 0], halves, R, R // 2, "physical", 8)
    v1 = _voltages(N, par, st, whole, R, R, "physical")
    v2 = np.concatenate([_voltages(N, par, st, h, R, R // 2, "physical") for h in halves])
    keep = (v1.view(np.uint64) == v2.view(np.uint64)).all(axis=1)
    assert keep.sum() >= R * R // 2, "too few points of the two halves have the bits of the whole grid"
    for key in ("levels", "hnorm", "raw"):
        a = np.ascontiguousarray(_np(one[key]).reshape(R * R, -1))[keep]
        b = np.ascontiguousarray(_np(two[key]).reshape(R * R, -1))[keep]
        diff = np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)).any(axis=1))
        assert diff.size == 0, (key, diff.size, diff[:8])
    second = np.arange(4096, R * R)                                         # the points a block solves after another
    pick = np.concatenate([second[:: max(1, second.size // 128)][:128], np.arange(0, 4096, 32)])
    assert pick.size == 256
    dev = H.dev_view(N, par)
    states, nv = _open_lists(dev, v1[pick, :G], v1[pick, G:], 32)
    assert len(set(nv.tolist())) > 1, "every picked list has the same length"
    lev_ref, hn_ref, _ = _spectrum(dev, v1[pick, :G], v1[pick, G:], states, nv)
    _compare(f"second trip N={N} R={R}", _np(one["levels"]).reshape(R * R, 8)[pick], _np(one["hnorm"]).reshape(R * R)[pick], lev_ref, hn_ref)
    env.close()


# ------------------------------------------------------------------ 7. slots, launch chunks, guard rows
def _raw_call(env, ids, dirs, rg, gv, bv, nq, nx, ny, dst, n_levels=2, n_charge=None, flags=0, lopts_size=None, opts_size=None,
              no_lopts=False):
    import torch
    from qadapt_hip import _lib
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dt)).cuda()      # noqa: E731
    keep = [t(ids, np.int32), t(dirs, np.float64), t(rg, np.float64), t(gv, np.float64), t(bv, np.float64),
            None if n_charge is None else t(n_charge, np.int32)]
    addr = lambda x: None if x is None else x.data_ptr()                        # noqa: E731
    o = _lib.QdScanGridOpts(struct_size=ctypes.sizeof(_lib.QdScanGridOpts) if opts_size is None else opts_size, frame=_lib.QD_SCAN_PHYSICAL,
                            noise_flags=flags, serial=(1 << 63) | 5, occ_dst=addr(dst.get("occupations")))
    lo = _lib.QdGridLevelsOpts(struct_size=ctypes.sizeof(_lib.QdGridLevelsOpts) if lopts_size is None else lopts_size, n_levels=n_levels,
                               n_charge_dev=addr(keep[5]), levels_dst=addr(dst.get("levels")), hnorm_dst=addr(dst.get("hnorm")))
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())          # noqa: E731
    rc = env._lib.qd_scan_grid_levels(env._h, p(keep[0]), nq, nx, ny, p(keep[1]), p(keep[2]), p(keep[3]), p(keep[4]), None,
                                      p(dst.get("raw")), p(dst.get("image")), p(dst.get("plohi")), ctypes.byref(o),
                                      None if no_lopts else ctypes.byref(lo), env._stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("nq", [1, 2, 5])
def test_slots_chunks_inert_queries_and_guard_rows(tmp_path, nq):
    """a 4-dot 8 x 8 handle with env_chunk = 2 holds 6 slots of 36 records: nq + 2 queries, two of them with env ids outside
    [0, B), through the C entry point with guard rows on both sides of every destination, levels_dst and hnorm_dst among them.
    Every live query has the bits of the same query alone, the inert ones leave their rows untouched, the guards stay; and a
    handle with env_chunk = 3, which cuts the call into launches differently, gives the same bits"""
    import torch
    N, R, B, seed = 4, 8, 3, 9850
    nx, ny, nl = 9, 4, 3
    G = N + 1
    rng = np.random.default_rng(seed + nq)
    params, state = _placed_blocks(N, [seed, seed + 1, seed + 2], ("near", "mid", "near"), rng)
    tot = nq + 2
    ids = np.array({1: [B, 1, -3], 2: [0, B, 2, -1], 5: [0, B, 2, 1, -1, 2, 0]}[nq], np.int32)
    live = (ids >= 0) & (ids < B)
    assert live.sum() == nq
    envs = np.clip(ids, 0, B - 1)
    qs = [_query(N, params[e], state[e], "physical", rng) for e in envs]
    dirs = np.stack([np.stack([q[0], q[1]]) for q in qs])
    rg = np.array([[*q[2], *q[3]] for q in qs])
    gv, bv = np.stack([q[4][:N] for q in qs]), np.stack([q[4][G:] for q in qs])
    g0, g1, guard = 2, 3, -12345.678
    full = lambda *s: torch.full(s, guard, dtype=torch.float64, device="cuda")     # noqa: E731

    def buffers(rows):
        d = dict(raw=full(rows, ny, nx), plohi=full(rows, 2), occupations=full(rows, ny, nx, N), levels=full(rows, ny, nx, nl),
                 hnorm=full(rows, ny, nx))
        d["image"] = torch.full((rows, ny, nx), -7.0, dtype=torch.float32, device="cuda")
        return d

    results = []
    for chunk in (2, 3):
        env = _vec(tmp_path, B, N, R, seed, env_chunk=chunk)
        assert env.chunk_envs() == chunk
        _load(env, params, state)
        big = buffers(g0 + tot + g1)
        view = {k: v[g0:] for k, v in big.items()}
        assert _raw_call(env, ids, dirs, rg, gv, bv, tot, nx, ny, view, n_levels=nl) == 0
        got = {k: v.cpu().numpy() for k, v in big.items()}
        for k, a in got.items():
            gval = -7.0 if k == "image" else guard
            assert np.all(a[:g0] == gval) and np.all(a[g0 + tot:] == gval), k
            assert np.all(a[g0:g0 + tot][~live] == gval), k
            assert not np.isnan(a[g0:g0 + tot][live]).any() and not np.any(a[g0:g0 + tot][live] == gval), k
        if chunk == 2:
            for q in np.flatnonzero(live):
                alone = buffers(1)
                assert _raw_call(env, ids[q:q + 1], dirs[q:q + 1], rg[q:q + 1], gv[q:q + 1], bv[q:q + 1], 1, nx, ny, alone, n_levels=nl) == 0
                for k in alone:
                    assert PH.same(alone[k].cpu().numpy()[0], got[k][g0 + q]), (k, q)
            # hnorm_dst NULL and no image destinations: the levels alone, the same bits
            only = dict(levels=full(tot, ny, nx, nl))
            assert _raw_call(env, ids, dirs, rg, gv, bv, tot, nx, ny, only, n_levels=nl) == 0
            assert PH.same(only["levels"].cpu().numpy(), got["levels"][g0:g0 + tot])
        results.append(got)
        env.close()
    for k in results[0]:
        assert PH.same(results[0][k], results[1][k]), k


# ------------------------------------------------------------------ 8. nothing else moves
def test_levels_grids_leave_no_footprint(tmp_path):
    """scan_grid and eval_points(levels=) give the same bits before and after levels grids on the same handle, two identical
    levels grids give the same bits, the observation serial of the RNG stays, and one step() of a handle that rendered levels
    grids equals that of its twin that did not"""
    import torch
    N, R, B, seed = 4, 8, 2, 9860
    plain, poked = [_vec(tmp_path, B, N, R, seed) for _ in range(2)]
    for env in (plain, poked):
        env.reset(seed=seed)
    L = layout(N)
    st, steps0 = poked.get_state()
    gv, bv = st[:, L.s_gate_gt:L.s_gate_gt + N], st[:, L.s_barrier_gt:L.s_barrier_gt + N - 1]
    vg, vb = CH.points(N, np.random.default_rng(seed), 40)

    def serial(env):
        s = ctypes.c_uint64(0)
        assert env._lib.qd_get_rng_state(env._h, ctypes.byref(s)) == 0
        return int(s.value)

    cold = lambda: poked.scan_grid([0, 1], "e1_2", "U1_2", (-2, 2), (1, -1), 9, 5, gv, bv, occupations=True)      # noqa: E731
    pts = lambda: poked.eval_points([0, 1], np.stack([vg, vg]), np.stack([vb, vb]), levels=4)                        # noqa: E731
    lv = lambda **kw: poked.scan_grid_levels([1, 0], "e1_2", "U1_2", (-2, 2), (1, -1), 9, 5, gv[::-1], bv[::-1], levels=4,   # noqa: E731
                                             occupations=True, **kw)
    ser0 = serial(poked)
    before, before_p = cold(), pts()
    t1, t2 = lv(), lv()
    t3 = poked.scan_grid_levels([1, 0], "vP1", "vP2", (-2, 2), (1, -1), 7, 3, gv, bv, levels=8, n_charge=3, occupations=True)
    t4 = lv(noise=("sensor",), serial=(1 << 63) | 3)
    for key in t1:
        assert PH.same(t1[key], t2[key]), key
    assert PH.same(t1["raw"][[1, 0]], before["raw"]) and PH.same(t1["occupations"][[1, 0]], before["occupations"])
    assert np.all(np.abs(_np(t3["occupations"]).sum(axis=-1) - 3.0) <= 1e-9) and np.isfinite(_np(t3["levels"])[..., 0]).all()
    assert PH.same(t4["levels"], t1["levels"]) and not PH.same(t4["raw"], t1["raw"])
    after, after_p = cold(), pts()
    for a, b in ((before, after), (before_p, after_p)):
        assert a.keys() == b.keys()
        for key in a:
            assert PH.same(a[key], b[key]), key
    st1, steps1 = poked.get_state()
    assert PH.same(st, st1) and np.array_equal(steps0, steps1) and serial(poked) == ser0 == serial(plain)
    act = torch.as_tensor(np.random.default_rng(13).uniform(-1, 1, (B, 2 * N - 1)).astype(np.float32)).cuda()
    res = []
    for env in (plain, poked):
        obs, rew, term, trunc = env.step(act)
        stt, steps = env.get_state()
        res.append(dict(image=_np(obs["image"]).copy(), gv=_np(obs["obs_gate_voltages"]).copy(), bv=_np(obs["obs_barrier_voltages"]).copy(),
                        rew=_np(rew).copy(), raw=env.raw()[0].copy(), plohi=env.raw()[1].copy(), state=stt, steps=steps,
                        params=env._params_host.copy(), serial=serial(env)))
    for key in res[0]:
        assert PH.same(res[0][key], res[1][key]) if key != "serial" else res[0][key] == res[1][key], key
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
    grid = lambda env, **kw: env.scan_grid_levels([0], "e1_2", "vP3", (-1, 1), (-1, 1), 8, 2, gv, bv, **kw)      # noqa: E731
    for kw, word in ((dict(validate=True), "QD_FLAG_VALIDATE"),
                     (dict(num_charge_states="all", qarray_config_path=str(qp)), "full charge-state space")):
        env = _vec(tmp_path, 1, N, R, 77, **kw)
        env.reset(seed=77)
        raw0 = env.raw()[0].copy()
        with pytest.raises(_lib.QdError, match=word) as ei:
            grid(env)
        assert f"code {_lib.QD_ERR_STATE}" in str(ei.value) and "qd_scan_grid_levels" in str(ei.value)
        assert PH.same(env.raw()[0], raw0)
        env.close()
    env = _vec(tmp_path, 1, N, R, 78, noise=("sensor", "latch"))
    env.reset(seed=78)
    for bad in (0, 9, -2):
        with pytest.raises(ValueError, match="levels"):
            grid(env, levels=bad)
    with pytest.raises(ValueError, match="closed regime"):
        grid(env, n_charge=2, noise=("sensor",))
    with pytest.raises(ValueError, match="closed regime"):
        grid(env, n_charge=2, noise=True)
    with pytest.raises(ValueError, match="radial"):
        grid(env, noise=("radial",))
    for kw in (dict(levels=2),):                                                               # the siblings are as they were
        with pytest.raises(TypeError):
            env.scan_grid([0], "e1_2", "vP3", (-1, 1), (-1, 1), 8, 2, gv, bv, **kw)
        with pytest.raises(TypeError):
            env.scan_grid_closed([0], "e1_2", "vP3", (-1, 1), (-1, 1), 8, 2, gv, bv, 2, **kw)
    before = grid(env, levels=3, occupations=True)
    d = np.stack([np.eye(2 * N)[0], np.eye(2 * N)[1]])[None]
    rg = [[-1, 1, -1, 1]]
    dst = dict(raw=torch.full((1, 2, 8), -5.0, dtype=torch.float64, device="cuda"),
               levels=torch.full((1, 2, 8, 8), -5.0, dtype=torch.float64, device="cuda"),
               hnorm=torch.full((1, 2, 8), -5.0, dtype=torch.float64, device="cuda"))
    size_l, size_o = ctypes.sizeof(_lib.QdGridLevelsOpts), ctypes.sizeof(_lib.QdScanGridOpts)
    cases = [(dict(no_lopts=True), "lopts is NULL"), (dict(lopts_size=size_l - 8), "struct_size"), (dict(opts_size=size_o - 8), "struct_size"),
             (dict(n_levels=0), "n_levels"), (dict(n_levels=9), "n_levels"),
             (dict(flags=_lib.QD_NOISE_SENSOR, n_charge=[2]), "closed regime"), (dict(flags=_lib.QD_NOISE_RADIAL), "noise_flags"),
             (dict(n_charge=[-1]), "0..32767"), (dict(n_charge=[32768]), "0..32767")]
    for kw, word in cases:
        rc = _raw_call(env, [0], d, rg, gv, bv, 1, 8, 2, dst, **kw)
        msg = env._lib.qd_last_error(env._h).decode()
        assert rc == _lib.QD_ERR_ARG and msg.startswith("qd_scan_grid_levels") and word in msg, (kw, rc, msg)
        assert all(np.all(t.cpu().numpy() == -5.0) for t in dst.values())
        after = grid(env, levels=3, occupations=True)                                          # the handle is usable
        for key in before:
            assert PH.same(before[key], after[key]), (word, key)
    rc = _raw_call(env, [0], d, rg, gv, bv, 1, 8, 2, dict(raw=dst["raw"]))
    assert rc == _lib.QD_ERR_ARG and "levels_dst" in env._lib.qd_last_error(env._h).decode()
    rc = _raw_call(env, [0], d, rg, gv, bv, 1, 9, 8, dst)
    assert rc == _lib.QD_ERR_ARG and "nx*ny" in env._lib.qd_last_error(env._h).decode()
    env.close()


def test_facade_levels_grids(tmp_path):
    """do2d_levels and do1d_levels against the backend's scan_grid_levels bit for bit, and against energy_levels_open /
    energy_levels_closed at numpy's linspace of the same ranges within 2e-12 hnorm (the sum of both bars; the grid's own
    linspace need not have numpy's bits, so nothing bitwise is claimed against the points here)"""
    from qadapt_hip.env import QuantumDeviceEnv
    N, R = 3, 8
    path = _cfg(tmp_path, num_dots=N, resolution=R)
    backend = _vec(tmp_path, 1, N, R, 9900, config_path=path)
    env = QuantumDeviceEnv(config_path=path, num_dots=N, backend=backend)
    model = env.array.model
    par = backend._params_host[0]
    L, G = layout(N), N + 1
    p0 = par[L.vopt:L.vopt + G]
    nx, ny = 7, 5
    xs, ys = np.linspace(p0[0] - 3, p0[0] + 3, nx), np.linspace(p0[1] + 2, p0[1] - 2, ny)
    lev, hn = model.do2d_levels("P1", xs[0], xs[-1], nx, "P2", ys[0], ys[-1], ny, n_levels=4)
    assert lev.shape == (ny, nx, 4) and hn.shape == (ny, nx) and lev.dtype == hn.dtype == np.float64
    want = backend.scan_grid_levels([0], 0, 1, (xs[0], xs[-1]), (ys[0], ys[-1]), nx, ny, np.zeros((1, N)), np.zeros((1, N - 1)), 0.0,
                                    levels=4, frame="physical", gamma=float(model.coulomb_peak_width))
    assert PH.same(lev, want["levels"][0]) and PH.same(hn, want["hnorm"][0])
    vg = np.zeros((ny, nx, G)); vg[:, :, 0] = xs[None, :]; vg[:, :, 1] = ys[:, None]
    vb = np.zeros((ny, nx, N - 1))
    rl, rh = model.energy_levels_open(vg, vb, n_levels=4)
    fin = np.isfinite(rl)
    assert np.array_equal(np.isfinite(lev), fin) and np.all(np.abs(hn - rh) <= 1e-13 * rh)
    assert np.all(np.abs(np.where(fin, lev, 0.0) - np.where(fin, rl, 0.0)) <= 2e-12 * rh[..., None])
    l1, h1 = model.do1d_levels("P1", xs[0], xs[-1], nx)
    assert l1.shape == (nx, 2) and h1.shape == (nx,)
    w1 = backend.scan_grid_levels([0], 0, np.zeros(2 * N), (xs[0], xs[-1]), (0.0, 0.0), nx, 1, np.zeros((1, N)), np.zeros((1, N - 1)), 0.0,
                                  levels=2, frame="physical", gamma=float(model.coulomb_peak_width))
    assert PH.same(l1, want_row := _np(w1["levels"])[0, 0]) and want_row.shape == (nx, 2) and PH.same(h1, _np(w1["hnorm"])[0, 0])
    l2, h2 = model.do2d_levels("P1", xs[0], xs[-1], nx, "P2", ys[0], ys[-1], ny, n_levels=3, n_charge=2)
    r2, rh2 = model.energy_levels_closed(vg, 2, n_levels=3, vb=vb)
    f2 = np.isfinite(r2)
    assert np.array_equal(np.isfinite(l2), f2) and np.all(np.abs(h2 - rh2) <= 1e-13 * rh2)
    assert np.all(np.abs(np.where(f2, l2, 0.0) - np.where(f2, r2, 0.0)) <= 2e-12 * rh2[..., None])
    l3, h3 = model.do1d_levels("P2", ys[0], ys[-1], ny, n_levels=3, n_charge=2)
    assert l3.shape == (ny, 3) and np.isfinite(l3[:, 0]).all()
    with pytest.raises(NotImplementedError):
        model.do2d_levels("P1", 0, 1, 3, "vP2", 0, 1, 3)
    out = env.array.scan_grid_levels(0, 1, (xs[0], xs[-1]), (ys[0], ys[-1]), nx, ny, np.zeros(N), np.zeros(N - 1), 0.0, levels=4,
                                     frame="physical", gamma=float(model.coulomb_peak_width))
    assert PH.same(out["levels"], lev) and out["gap"].shape == out["rel_gap"].shape == (ny, nx)
    assert PH.same(out["gap"], lev[..., 1] - lev[..., 0])
    env.close()
