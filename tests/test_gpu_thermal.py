"""The thermal state per point on the MI355X (run with -m gpu): qd_eval_points_thermal / eval_points(kT=...) against the reference
of tests/thermal_helpers.py -- eigh of the oracle's Hamiltonian on its kept list cut to the nv valid states, P = V^2 softmax(-w / kT)
-- open and closed, the classical and the low-temperature limit, a point on a charge-transition line, slots and launch chunks,
the absent footprint on everything else, the refusals and the facade.

Bound everywhere (thermal_helpers): occupations within tol_occ = n_max 4 (1e-12 hs + 1e-13 hn) min(1 / kT, 1 / g) + 1e-12,
variances within n_max tol_occ, ztail within the same expression without n_max and with 1e-300 for 1e-12.  EVERY point is
compared: the thermal state needs no gap exemption (the one place the exemption appears is the comparison with the T = 0 path).
Worst err / tol measured over this file on an MI355X (also in DESIGN 7, "Finite temperature"): occupations 4.7e-4 and variance
7.6e-4 (open, 2 dots, far, kT = the median gap), ztail 8.3e-5 (open, 8 dots, K = 8, mid); closed lists 3.3e-4; the signal within
1.5e-14 relative of the sensor expression at the device's own occupations."""
import ctypes

import numpy as np
import pytest
import yaml

import closed_helpers as CH
import gs_cases as GC
import helpers as H
import points_helpers as PH
import qd_oracle as O
import search_cases as SC
import thermal_helpers as TH
from qadapt_hip import device_model as DM
from qadapt_hip.layout import layout
from test_gpu_levels import SPANS, _cfg, _load, _np, _open_lists, _physical, _vec

pytestmark = pytest.mark.gpu

ALL = ("signal", "occupations", "variance", "ztail")
KT_100K = TH.KB_REF * 100


def _signal_from(N, par, v_ext, occ, gamma):
    """the sensor stage alone, in numpy: c0 = 2 b + a (2 (Ns - v''_s) + 1) from the given occupations, then the ten Lorentzians"""
    L, G = layout(N), N + 1
    A = par[L.cdd_inv:L.cdd_inv + G * G].reshape(G, G)
    vpp = PH.point_front(N, par, v_ext)["vpp"]
    b = ((occ - vpp[:, :N]) * A[N, :N][None, :]).sum(axis=1)
    a, vs = A[N, N], vpp[:, N]
    c0 = 2.0 * b + a * (2.0 * (np.rint(vs) - vs) + 1.0)
    rr = (c0[:, None] + 2.0 * a * np.arange(-5, 5)[None, :]) / gamma
    return (1.0 / (rr * rr + 1.0)).sum(axis=1)


def _gaps(Hs):
    """w[1] - w[0] per point, nan where a point has one state"""
    return np.array([np.diff(np.linalg.eigvalsh(Hm)[:2])[0] if Hm is not None and Hm.shape[0] > 1 else np.nan for Hm in Hs])


def _check(tag, N, par, vg, vb, Hs, states, nv, kT, out, e, gamma=None):
    """occupations, variance, ztail of env slot e against the reference, and the signal against the sensor expression at the
    device's own occupations to 1e-12 relative; returns the worst err / tol"""
    occ, var, zt, sig = (_np(out[k][e]) for k in ("occupations", "variance", "ztail", "signal"))
    worst = TH.compare_points(tag, Hs, states, nv, kT, occ, var, zt)
    L = layout(N)
    want = _signal_from(N, par, np.concatenate([vg, vb], axis=1), occ, par[L.scal + 1] if gamma is None else gamma)
    rel = np.abs(sig - want) / np.abs(want)
    print(f"[thermal] {tag}: worst signal difference from the sensor expression at the device's occupations {rel.max():.2e} relative")
    assert np.all(rel <= 1e-12), (tag, float(rel.max()))
    return worst


# ------------------------------------------------------------------ 1. oracle parity, open
@pytest.mark.parametrize("N,K", [(2, 32), (3, 32), (4, 32), (8, 32), (8, 20), (8, 16), (8, 8)])
def test_open_parity(tmp_path, N, K):
    """64 points on each of three envs, spread near, mid and far as in test_gpu_levels.py, at kT = 1e-2 and 1 times the median gap of
    the env's points and at the kT of 100 K.  Measured: worst err / tol 7.6e-4 (N = 2, K = 32: the variance on the far env at
    kT = the median gap), 2.0e-4 .. 3.7e-4 at 8 dots, 4.5e-5 and 5.3e-5 at 3 and 4 dots."""
    L, C = layout(N), N - 1
    eb = H.sample_blocks(N, [41, 42, 43])
    rng = np.random.default_rng(9000 + 10 * N + K)
    vg, vb, lists, gap = [], [], [], []
    for e, mode in enumerate(("near", "mid", "far")):
        s, t = SPANS[mode]
        par, st = eb.params[e], eb.state[e]
        vg.append(_physical(L, par, st, st[L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-s, s, (64, N))))
        vb.append(st[L.s_barrier_gt:L.s_barrier_gt + C] + rng.uniform(-t, t, (64, C)))
        dev = H.dev_view(N, par)
        states, nv = _open_lists(dev, vg[e], vb[e], K)
        assert nv.min() >= 1
        Hs, tc = TH.hamiltonians(dev, vg[e], vb[e], states, nv)
        lists.append((states, nv, Hs, float(tc.max())))
        gap.append(float(np.nanmedian(_gaps(Hs))))
    assert min(gap) > 0
    env = _vec(tmp_path, 3, N, 8, 41, num_charge_states=K)
    _load(env, eb.params, eb.state)
    worst = 0.0
    for name, kT in (("1e-2 gap", 1e-2 * np.array(gap)), ("gap", np.array(gap)), ("100 K", np.full(3, KT_100K))):
        out = env.eval_points([0, 1, 2], np.stack(vg), np.stack(vb), kT=kT, outputs=ALL)
        assert set(out) == set(ALL) and out["variance"].shape == (3, 64, N) and out["ztail"].shape == (3, 64)
        for e, mode in enumerate(("near", "mid", "far")):
            states, nv, Hs, tcmax = lists[e]
            worst = max(worst, _check(f"open N={N} K={K} {mode} kT={kT[e]:.2e} ({name}; tc up to {tcmax:.1e})", N, eb.params[e],
                                      vg[e], vb[e], Hs, states, nv, kT[e], out, e))
    print(f"[thermal] open N={N} K={K}: worst err / tol {worst:.2e}")
    env.close()


# ------------------------------------------------------------------ 2. oracle parity, closed
@pytest.mark.parametrize("N", [4, 8])
def test_closed_parity(tmp_path, N):
    """three envs, a total charge per env, the kept lists of the host build of the sector search (closed_helpers)"""
    seed = 9100 + N
    env = _vec(tmp_path, 3, N, 8, seed)
    env.reset(seed=seed)
    vg, vb = CH.points(N, np.random.default_rng(seed + 1), 64)
    Qv = [1, N, N + 2]
    lists, gap = [], []
    for e, Q in enumerate(Qv):
        par = env._params_host[e]
        host = CH.host_closed(N, par, np.concatenate([vg, vb], axis=1), Q, 32)
        nv = np.minimum(host["nvalid"], 32)
        Hs, _ = TH.hamiltonians(H.dev_view(N, par), vg, vb, host["states"], nv)
        lists.append((host["states"], nv, Hs))
        gap.append(float(np.nanmedian(_gaps(Hs))))
    worst = 0.0
    for name, kT in (("1e-2 gap", 1e-2 * np.array(gap)), ("gap", np.array(gap)), ("100 K", np.full(3, KT_100K))):
        out = env.eval_points([0, 1, 2], np.stack([vg] * 3), np.stack([vb] * 3), n_charge=Qv, kT=kT, outputs=ALL)
        for e, Q in enumerate(Qv):
            states, nv, Hs = lists[e]
            worst = max(worst, _check(f"closed N={N} Q={Q} kT={kT[e]:.2e} ({name})", N, env._params_host[e], vg, vb, Hs, states, nv,
                                      kT[e], out, e))
            tot = _np(out["occupations"][e]).sum(axis=1)
            assert np.all(np.abs(tot[nv > 0] - Q) <= 1e-9), (Q, float(np.abs(tot[nv > 0] - Q).max()))
    print(f"[thermal] closed N={N}: worst err / tol {worst:.2e}")
    env.close()


# ------------------------------------------------------------------ 3. the classical limit
def test_zero_couplings_give_the_boltzmann_distribution_over_the_oracles_energies(tmp_path):
    """the all_sizes scene of gs_cases.py (5 dots, components of every size) with tc_base = 0: all couplings exactly zero, the
    occupations are the softmax over the oracle's free energies of the kept states"""
    N, R, name = 5, 16, "all_sizes"
    L = layout(N)
    par, st = GC.make(name, N, R)
    par[L.scal] = 0.0
    env = _vec(tmp_path, 1, N, R, 9200)
    _load(env, par[None], st[None])
    dev = H.dev_view(N, par)
    vs, sts = [], []
    for ch in (0, 3):
        pix = np.arange(0, R * R, 8)
        vs.append(PH.scan_voltages(N, par, st, ch, R)[0][pix])
        sts.append(np.asarray(GC.census(name, N, R, ch)["states"])[pix])
    v, states = np.concatenate(vs), np.concatenate(sts)
    vg, vb = v[:, :N + 1], v[:, N + 1:]
    nv = np.full(v.shape[0], 32)
    Hs, tc = TH.hamiltonians(dev, vg, vb, states, nv)
    assert not tc.any()
    for kT in (0.004, 0.05):
        out = env.eval_points([0], vg[None], vb[None], kT=kT, outputs=ALL)
        occ = _np(out["occupations"][0])
        worst = 0.0
        for p, Hm in enumerate(Hs):
            F = np.diag(Hm)
            with np.errstate(under="ignore"):
                want = TH.softmax(-(F - F.min()) / kT) @ states[p].astype(np.float64)
            worst = max(worst, float(np.abs(occ[p] - want).max() / TH.tol_occ(Hm, kT, float(states[p].max()))))
        print(f"[thermal] zero couplings kT={kT}: worst |occ - softmax(-F / kT) . states| / tol_occ {worst:.2e}")
        assert worst <= 1.0
        _check(f"zero couplings kT={kT}", N, par, vg, vb, Hs, states, nv, kT, out, 0)
    env.close()


def test_lead_transition_follows_the_fermi_function(tmp_path):
    """2 dots without coupling, plunger 0 scanned through its 1 -> 2 transition: <n_0> = n_low + 1 / (1 + exp(dE / kT)) with
    |dE| = levels[1] - levels[0] of the device's own levels and its sign from the T = 0 occupation.  Tolerance: the levels are
    within 1e-12 hnorm each (their bar), so dE / kT within 2e-12 hnorm / kT, and the slope of the Fermi function is at most 1/4;
    the third level lies more than 40 kT up (asserted), so the 14 other states carry less than 16 exp(-40) = 7e-17; 8 eps for
    the arithmetic of the formula itself."""
    N, R, kT = 2, 8, 0.002
    par, st = SC.build(dict(r=0.05, gate=np.array([1.3, 0.8]), step=1 / 8), N, R, tc_base=0.0)
    env = _vec(tmp_path, 1, N, R, 9300)
    _load(env, par[None], st[None])
    n = 65
    vg = np.stack([np.linspace(1.3, 1.7, n), np.full(n, 0.8), np.full(n, 0.25)], axis=1)
    vb = np.zeros((n, 1))
    lev = env.eval_points([0], vg[None], vb[None], outputs=("occupations",), levels=3)
    cold = _np(lev["occupations"][0])
    levels, hn = _np(lev["levels"][0]), _np(lev["hnorm"][0])
    out = env.eval_points([0], vg[None], vb[None], kT=kT, outputs=ALL)
    occ, var = _np(out["occupations"][0]), _np(out["variance"][0])
    assert set(np.unique(cold[:, 0])) == {1.0, 2.0} and np.all(cold[:, 1] == 1.0)
    assert np.all(levels[:, 2] - levels[:, 0] > 40 * kT)
    dE = (levels[:, 1] - levels[:, 0]) * np.where(cold[:, 0] == 1.0, 1.0, -1.0)
    f = 1.0 / (1.0 + np.exp(dE / kT))
    tol = 0.25 * 2e-12 * hn / kT + 16 * np.exp(-40.0) + 8 * np.finfo(np.float64).eps
    err = np.abs(occ[:, 0] - (1.0 + f))
    print(f"[thermal] lead transition: dE / kT {dE.min() / kT:.1f}..{dE.max() / kT:.1f}, <n_0> {occ[:, 0].min():.6f}..{occ[:, 0].max():.6f}, "
          f"worst |<n_0> - 1 - f| / tol {np.max(err / tol):.2e}")
    assert np.all(err <= tol) and np.all(np.abs(var[:, 0] - f * (1.0 - f)) <= 3 * tol)
    assert np.all(np.abs(occ[:, 1] - 1.0) <= tol) and (np.abs(dE) < kT).any() and (np.abs(dE) > 10 * kT).any()
    env.close()


# ------------------------------------------------------------------ 4. the low-temperature limit
@pytest.mark.parametrize("N,K", [(4, 32), (8, 16)])
def test_low_temperature_limit_is_the_ground_state(tmp_path, N, K):
    """kT = (w[1] - w[0]) / 800 per point (a group per point): every excited weight underflows, and the occupations equal those of
    eval_points without kT within 1e-6 at every point with rel_gap > 1e-9 -- the project's rule for the T = 0 path, and the only
    place the exemption appears"""
    L, C = layout(N), N - 1
    eb = H.sample_blocks(N, [42])
    par, st = eb.params[0], eb.state[0]
    rng = np.random.default_rng(9400 + N)
    s, t = SPANS["mid"]
    vg = _physical(L, par, st, st[L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-s, s, (64, N)))
    vb = st[L.s_barrier_gt:L.s_barrier_gt + C] + rng.uniform(-t, t, (64, C))
    dev = H.dev_view(N, par)
    states, nv = _open_lists(dev, vg, vb, K)
    Hs, _ = TH.hamiltonians(dev, vg, vb, states, nv)
    gap = _gaps(Hs)
    keep = np.nonzero(gap > 0)[0]
    rel = gap[keep] / np.array([TH.hnorm(Hs[p]) for p in keep])
    assert keep.size >= 48
    env = _vec(tmp_path, 1, N, 8, 42, num_charge_states=K)
    _load(env, eb.params, eb.state)
    ids = np.zeros(keep.size, np.int32)
    out = env.eval_points(ids, vg[keep][:, None, :], vb[keep][:, None, :], kT=gap[keep] / 800.0, outputs=("occupations", "ztail"))
    cold = env.eval_points(ids, vg[keep][:, None, :], vb[keep][:, None, :], outputs=("occupations",))
    d = np.abs(_np(out["occupations"]) - _np(cold["occupations"])).reshape(keep.size, N).max(axis=1)
    ok = rel > 1e-9
    print(f"[thermal] low temperature N={N} K={K}: {int(ok.sum())} of {keep.size} points with rel_gap > 1e-9, worst difference from "
          f"the T = 0 occupations {d[ok].max():.2e}")
    assert ok.sum() >= 40 and np.all(d[ok] <= 1e-6)
    many = np.array([Hs[p].shape[0] > 1 for p in keep])
    assert np.all(_np(out["ztail"]).reshape(-1)[many] == 0.0)                 # the last weight has underflown
    env.close()


# ------------------------------------------------------------------ 5. on a line
def test_exact_degeneracy_gives_the_equal_mixture(tmp_path):
    """the dyadic scene of search_cases.py (cdd_inv = I / 4, exact energies) with tc_base = 0.  Point A: dot 0 at 1.5, the others at
    integers: |1 ..> and |2 ..> tie exactly, weight 1/2 each.  Point B: every dot at 1.5 (the family's own voltages),
    a 16-fold tie.  The T = 0 path returns one of the tied states; the thermal state is defined."""
    N, R, kT = 4, 8, 0.005
    par, st = SC.make("dyadic", N, R, tc_base=0.0)
    env = _vec(tmp_path, 1, N, R, 9500)
    _load(env, par[None], st[None])
    dev = H.dev_view(N, par)
    vg = np.array([[1.5, 2.0, 1.0, 1.0, 0.25], [1.5, 1.5, 1.5, 1.5, 0.25]])
    vb = np.zeros((2, N - 1))
    states, nv = _open_lists(dev, vg, vb, 32)
    Hs, tc = TH.hamiltonians(dev, vg, vb, states, nv)
    assert not tc.any()
    E = [np.sort(np.diag(Hm)) for Hm in Hs]
    assert E[0][0] == E[0][1] < E[0][2] and E[1][0] == E[1][15] < E[1][16]
    out = env.eval_points([0], vg[None], vb[None], kT=kT, outputs=ALL)
    _check("on a line", N, par, vg, vb, Hs, states, nv, kT, out, 0)
    occ, var = _np(out["occupations"][0]), _np(out["variance"][0])
    tol = [TH.tol_occ(Hm, kT, 2.0) for Hm in Hs]
    assert np.abs(occ[0] - [1.5, 2.0, 1.0, 1.0]).max() <= tol[0] and abs(var[0, 0] - 0.25) <= 2 * tol[0]
    assert np.abs(occ[1] - 1.5).max() <= tol[1] and np.abs(var[1] - 0.25).max() <= 2 * tol[1]
    cold = _np(env.eval_points([0], vg[None], vb[None], outputs=("occupations",))["occupations"][0])
    assert cold[0, 0] in (1.0, 2.0) and np.all(np.isin(cold[1], (1.0, 2.0)))
    env.close()


# ------------------------------------------------------------------ 6. slots, launch chunks
def test_groups_across_slot_and_chunk_boundaries(tmp_path):
    """N = 2, R = 8: a slot holds C P = 64 points and env_chunk = 2 puts two slots in a launch.  Groups of 1, 63, 64, 65 and 200
    points (ten slots, five launches) with two different kT in one call against every group alone, bit for bit; then the C call
    with guard rows and without options."""
    import torch
    from qadapt_hip import _lib
    N, R, B, seed = 2, 8, 3, 9600
    L, G, C = layout(N), N + 1, N - 1
    env = _vec(tmp_path, B, N, R, seed, env_chunk=2)
    assert env.chunk_envs() == 2
    env.load_new_devices(seed=seed)
    st, _ = env.get_state()
    sizes, envs = [1, 63, 64, 65, 200], np.array([0, 2, 1, 2, 0], np.int32)
    kT = np.array([0.01, 0.2, 0.01, 0.2, 0.2])
    rng = np.random.default_rng(98)
    vgs, vbs = [], []
    for n, e in zip(sizes, envs):
        virt = st[e, L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-3, 3, (n, N))
        vgs.append(_physical(L, env._params_host[e], st[e], virt))
        vbs.append(st[e, L.s_barrier_gt:L.s_barrier_gt + C] + rng.uniform(-3, 3, (n, C)))
    vgs, vbs = [torch.as_tensor(v).cuda() for v in vgs], [torch.as_tensor(v).cuda() for v in vbs]
    out = env.eval_points(envs, vgs, vbs, kT=kT, outputs=ALL)
    assert [tuple(t.shape) for t in out["variance"]] == [(n, N) for n in sizes]
    assert [tuple(t.shape) for t in out["ztail"]] == [(n,) for n in sizes]
    for g, (n, e) in enumerate(zip(sizes, envs)):
        alone = env.eval_points([int(e)], vgs[g][None], vbs[g][None], kT=kT[g], outputs=ALL)
        for key in ALL:
            assert PH.same(alone[key][0], out[key][g]), (key, g)
        if n >= 63:
            other = env.eval_points([int(e)], vgs[g][None], vbs[g][None], kT=0.07, outputs=("occupations",))
            assert not PH.same(other["occupations"][0], out["occupations"][g])           # kT is the group's own
    # the C entry point with guard rows on both sides of the caller's buffers
    g0, g1, npts = 5, 7, sum(sizes)
    start = (g0 + np.concatenate([[0], np.cumsum(sizes)])).astype(np.int64)
    vg_all = torch.full((g0 + npts + g1, G), float("nan"), dtype=torch.float64, device="cuda")
    vb_all = torch.full((g0 + npts + g1, C), float("nan"), dtype=torch.float64, device="cuda")
    vg_all[g0:g0 + npts] = torch.cat(vgs); vb_all[g0:g0 + npts] = torch.cat(vbs)
    guard = -12345.678
    dst = {k: torch.full((g0 + npts + g1,) + ((N,) if k in ("occupations", "variance") else ()), guard, dtype=torch.float64, device="cuda")
           for k in ALL}
    opts = _lib.QdThermalOpts(struct_size=ctypes.sizeof(_lib.QdThermalOpts), var_dst=dst["variance"].data_ptr(),
                              ztail_dst=dst["ztail"].data_ptr())

    def call(o, sig, occ):
        return env._lib.qd_eval_points_thermal(env._h, envs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                               start.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(sizes),
                                               ctypes.c_void_p(vg_all.data_ptr()), ctypes.c_void_p(vb_all.data_ptr()),
                                               kT.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), sig, occ, o, env._stream())

    assert call(ctypes.byref(opts), ctypes.c_void_p(dst["signal"].data_ptr()), ctypes.c_void_p(dst["occupations"].data_ptr())) == 0
    for k in ALL:
        a = dst[k].cpu().numpy()
        assert np.all(a[:g0] == guard) and np.all(a[g0 + npts:] == guard), k
        assert PH.same(a[g0:g0 + npts], torch.cat(out[k])), k
    # no options: the open regime, the env's own width; no signal and no occupations: only the options' outputs
    s2 = torch.full_like(dst["signal"], guard)
    assert call(None, ctypes.c_void_p(s2.data_ptr()), None) == 0 and PH.same(s2, dst["signal"])
    z2 = torch.full_like(dst["ztail"], guard)
    opts2 = _lib.QdThermalOpts(struct_size=ctypes.sizeof(_lib.QdThermalOpts), ztail_dst=z2.data_ptr())
    assert call(ctypes.byref(opts2), None, None) == 0 and PH.same(z2, dst["ztail"])
    env.close()


# ------------------------------------------------------------------ 7. nothing else moves
def test_thermal_calls_leave_no_footprint(tmp_path):
    """eval_points without kT and with levels = 2 give the same bits before and after a thermal call on the same handle, two
    identical thermal calls give the same bits, and one step() of a handle that answered thermal calls equals that of its twin
    that did not: observation, rewards, raw signal and state blocks"""
    import torch
    N, R, B, seed = 4, 8, 2, 9700
    C = N - 1
    plain, poked = [_vec(tmp_path, B, N, R, seed) for _ in range(2)]
    obs0 = [env.reset(seed=seed) for env in (plain, poked)]
    vg, vb = CH.points(N, np.random.default_rng(seed), 200)             # 200 points: two slots of C P = 192
    vg, vb = np.stack([vg, vg[::-1]]), np.stack([vb, vb[::-1]])
    before = poked.eval_points([0, 1], vg, vb)
    before_l = poked.eval_points([0, 1], vg, vb, levels=2)
    before_c = poked.eval_points([0, 1], vg, vb, n_charge=[2, 5])
    t1 = poked.eval_points([1, 0], vg, vb, kT=[0.01, 0.3], outputs=ALL)
    t2 = poked.eval_points([1, 0], vg, vb, kT=[0.01, 0.3], outputs=ALL)
    t3 = poked.eval_points([1, 0], vg, vb, kT=0.05, n_charge=3, outputs=ALL)
    for key in ALL:
        assert PH.same(t1[key], t2[key]), key
        assert np.isfinite(_np(t3[key])).all(), key
    some = poked.eval_points([1, 0], vg, vb, kT=[0.01, 0.3], outputs=("occupations",))
    assert set(some) == {"occupations"} and PH.same(some["occupations"], t1["occupations"])
    after = poked.eval_points([0, 1], vg, vb)
    after_l = poked.eval_points([0, 1], vg, vb, levels=2)
    after_c = poked.eval_points([0, 1], vg, vb, n_charge=[2, 5])
    for a, b in ((before, after), (before_l, after_l), (before_c, after_c)):
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


# ------------------------------------------------------------------ 8. refusals and the facade
def test_refusals(tmp_path):
    import torch
    from qadapt_hip import _lib
    N, R = 3, 8
    q = DM.load_yaml(None, "qarray_config.yaml")
    q["simulator"]["model"]["max_charge_carriers"] = 2
    qp = tmp_path / "qarray_m2.yaml"
    qp.write_text(yaml.safe_dump(q))
    zg, zb = np.zeros((1, 4, N + 1)), np.zeros((1, 4, N - 1))
    for kw, word in ((dict(validate=True), "QD_FLAG_VALIDATE"),
                     (dict(num_charge_states="all", qarray_config_path=str(qp)), "full charge-state space")):
        env = _vec(tmp_path, 1, N, R, 77, **kw)
        env.reset(seed=77)
        raw0 = env.raw()[0].copy()
        for more in ({}, {"n_charge": 2}):
            with pytest.raises(_lib.QdError, match=word) as ei:
                env.eval_points([0], zg, zb, kT=0.01, **more)
            assert f"code {_lib.QD_ERR_STATE}" in str(ei.value) and "qd_eval_points_thermal" in str(ei.value)
        assert _lib.QD_ERR_STATE == 3 and PH.same(env.raw()[0], raw0)
        env.close()
    env = _vec(tmp_path, 1, N, R, 78)
    env.reset(seed=78)
    for bad in (0.0, -0.01, float("inf"), float("nan"), [float("nan")]):
        with pytest.raises(ValueError, match="kT"):
            env.eval_points([0], zg, zb, kT=bad)
    with pytest.raises(ValueError, match="kT"):
        env.eval_points([0], zg, zb, kT=0.01, levels=2)
    with pytest.raises(ValueError, match="kT"):
        env.eval_points([0], zg, zb, kT=0.01, n_charge=2, states=True)
    with pytest.raises(ValueError, match="outputs"):
        env.eval_points([0], zg, zb, kT=0.01, outputs=("levels",))
    with pytest.raises(ValueError, match="outputs"):
        env.eval_points([0], zg, zb, outputs=("variance",))                              # thermal outputs need kT
    vg, vb = CH.points(N, np.random.default_rng(5), 4)
    before = env.eval_points([0], vg[None], vb[None], kT=0.02, outputs=ALL)
    g_d, b_d = torch.as_tensor(vg).cuda(), torch.as_tensor(vb).cuda()
    dst = torch.zeros(64, dtype=torch.float64, device="cuda")
    ids, start = np.array([0], np.int32), np.array([0, 4], np.int64)
    size = ctypes.sizeof(_lib.QdThermalOpts)
    for fields, kT, word in ((dict(struct_size=size - 8), 0.02, "struct_size"), (dict(struct_size=size), 0.0, "kT"),
                             (dict(struct_size=size), float("nan"), "kT"), (dict(struct_size=size), -1.0, "kT"),
                             (dict(struct_size=size), float("inf"), "kT")):
        opts = _lib.QdThermalOpts(var_dst=dst.data_ptr(), **fields)
        k = (ctypes.c_double * 1)(kT)
        rc = env._lib.qd_eval_points_thermal(env._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                             start.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1, ctypes.c_void_p(g_d.data_ptr()),
                                             ctypes.c_void_p(b_d.data_ptr()), k, ctypes.c_void_p(dst.data_ptr()), None,
                                             ctypes.byref(opts), env._stream())
        msg = env._lib.qd_last_error(env._h).decode()
        assert rc == _lib.QD_ERR_ARG and msg.startswith("qd_eval_points_thermal") and word in msg, (fields, kT, rc, msg)
        assert not _np(dst).any()
        after = env.eval_points([0], vg[None], vb[None], kT=0.02, outputs=ALL)           # the handle is usable
        for key in before:
            assert PH.same(before[key], after[key]), (word, key)
    env.close()


def test_facade_thermal_state(tmp_path):
    from qadapt_hip.env import QuantumDeviceEnv
    N, R = 3, 8
    path = _cfg(tmp_path, num_dots=N, resolution=R)
    backend = _vec(tmp_path, 1, N, R, 9900, config_path=path)
    env = QuantumDeviceEnv(config_path=path, num_dots=N, backend=backend)
    model = env.array.model
    T = float(backend.last_episode.extras["T"][0])
    assert 50.0 <= T <= 200.0 and model.T == T == backend._T_host[0]
    gamma = float(model.coulomb_peak_width)
    vg, vb = CH.points(N, np.random.default_rng(6), 12)
    for lead in ((12,), (3, 4), ()):
        g = vg.reshape(lead + (N + 1,)) if lead else vg[0]
        b = vb.reshape(lead + (N - 1,)) if lead else vb[0]
        n = 12 if lead else 1
        sig, occ, var = model.thermal_state_open(g, b)
        assert sig.shape == lead + (1,) and occ.shape == var.shape == lead + (N,) and sig.dtype == occ.dtype == var.dtype == np.float64
        want = backend.eval_points([0], vg[None, :n], vb[None, :n], gamma=gamma, kT=TH.KB_REF * T, outputs=ALL)
        for got, key in ((sig, "signal"), (occ, "occupations"), (var, "variance")):
            assert PH.same(got.reshape(_np(want[key][0]).shape), want[key][0]), key
        explicit = model.thermal_state_open(g, b, T=T)
        assert all(PH.same(x, y) for x, y in zip((sig, occ, var), explicit))
        hot = model.thermal_state_open(g, b, T=4 * T)
        assert not PH.same(hot[1], occ) and np.all(var >= 0)
        sig, occ, var = model.thermal_state_closed(g, 2, vb=b)
        want = backend.eval_points([0], vg[None, :n], vb[None, :n], gamma=gamma, kT=TH.KB_REF * T, n_charge=2, outputs=ALL)
        assert PH.same(occ.reshape(n, N), want["occupations"][0]) and PH.same(var.reshape(n, N), want["variance"][0])
        assert np.all(np.abs(occ.sum(axis=-1) - 2.0) <= 1e-9)
        assert all(PH.same(x, y) for x, y in zip((sig, occ, var), model.thermal_state_closed(g, 2, T=T, vb=b)))
    with pytest.raises(NotImplementedError):
        model.thermal_state_open(vg)
    # a device loaded from raw blocks carries no temperature
    ck = backend.get_checkpoint()
    assert np.array_equal(ck["T"], [T])
    del ck["T"]
    backend.set_checkpoint(ck)
    assert np.isnan(backend._T_host).all()
    with pytest.raises(ValueError, match="raw"):
        model.thermal_state_open(vg, vb)
    assert model.thermal_state_open(vg, vb, T=T)[1].shape == (12, N)
    env.close()


# ------------------------------------------------------------------ 9. more than one point per block
def test_second_point_of_a_block_keeps_nothing_from_the_first(tmp_path):
    """the slot of C P = 4608 points of test_gpu_levels.py, whose first 512 blocks solve a list of 32 states and then one of 27 on
    the same workspace (V, the upper triangle and the zeroed idle row and column of the point before are still in it), against
    the same points in two slots with one point per block: occupations, variance, ztail and signal bit for bit, and 256 of them
    against the reference"""
    from test_gpu_levels import _second_trip_points, _subsample
    N, R = 3, 48
    params, state, dev, vg, vb, states, nv = _second_trip_points(N, R)
    CP = vg.shape[0]
    env = _vec(tmp_path, 1, N, R, 61)
    _load(env, params, state)
    one = env.eval_points([0], vg[None], vb[None], kT=KT_100K, outputs=ALL)
    half = CP // 2
    two = env.eval_points([0, 0], vg.reshape(2, half, N + 1), vb.reshape(2, half, N - 1), kT=KT_100K, outputs=ALL)
    for key in ALL:
        a, b = np.ascontiguousarray(_np(one[key]).reshape(CP, -1)), np.ascontiguousarray(_np(two[key]).reshape(CP, -1))
        diff = np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)).any(axis=1))
        assert diff.size == 0, (key, diff.size, diff[:8], nv[diff[:8]])
    pick = _subsample(CP)
    Hs, _ = TH.hamiltonians(dev, vg[pick], vb[pick], states[pick], nv[pick])
    flat = {k: _np(two[k]).reshape((CP,) + _np(two[k]).shape[2:])[pick][None] for k in ALL}
    _check(f"two trips N={N} R={R} kT={KT_100K:.2e}", N, params[0], vg[pick], vb[pick], Hs, states[pick], nv[pick], KT_100K, flat, 0)
    env.close()
