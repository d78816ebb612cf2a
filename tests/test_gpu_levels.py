"""Energy levels per point on the MI355X (run with -m gpu): qd_eval_points_ex / eval_points(levels=L) against eigvalsh of the
oracle's Hamiltonian on its kept list cut to the nv valid states (open and closed), the two-level anticrossing, zero and very
large couplings, slots and launch chunks, the absent footprint on everything else, the refusals and the facade.

Bound everywhere: |level - eigvalsh| <= 1e-12 ||H||_inf of the oracle's matrix (the project's eigenvalue bar), ||H||_inf itself
within rtol 1e-14, +inf exactly from level nv on.  Every point is compared: eigenvalues need no gap exemption."""
import ctypes

import numpy as np
import pytest
import yaml

import closed_helpers as CH
import gs_cases as GC
import helpers as H
import points_helpers as PH
import qd_oracle as O
from qadapt_hip import device_model as DM
from qadapt_hip.layout import layout

pytestmark = pytest.mark.gpu

BAR, EPS = 1e-12, np.finfo(np.float64).eps
SPANS = {"near": (3.0, 3.0), "mid": (10.0, 6.0), "far": (40.0, 12.0)}          # helpers.place


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


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _physical(L, par, st, virt):
    G = L.N + 1
    vgm = st[L.s_vgm:L.s_vgm + G * G].reshape(G, G)
    full = np.concatenate([virt, np.full((virt.shape[0], 1), st[L.s_sensor_gt])], axis=1)
    return full @ vgm.T + par[L.origin:L.origin + G]


def _spectrum(dev, vg, vb, states, nv, n_levels=8):
    """per point: eigvalsh of diag(F) + oracle.tunnel_hamiltonian on the first nv states -> (levels (n, L) with +inf from nv
    on, hnorm (n,), tc (n, N - 1))"""
    N = dev.n_dot
    v_ext = np.concatenate([vg, vb], axis=1)
    with np.errstate(under="ignore"):
        tc = O.tunnel_couplings(O.effective_barrier_potential(vg, vb, dev.Cbg, dev.Cbb), dev.tc_base, dev.alpha)
    lev = np.full((vg.shape[0], n_levels), np.inf); hn = np.zeros(vg.shape[0])
    for k in np.unique(nv):
        sel = np.nonzero(nv == k)[0]
        if k == 0:
            continue
        st = states[sel, :k].astype(np.int64)
        F = O.free_energy_states(v_ext[sel], dev.cdd_inv_full, dev.cgd_full, st, N)
        with np.errstate(under="ignore"):
            Hm = F[:, :, None] * np.eye(k) + O.tunnel_hamiltonian(tc[sel], st)
        w = np.linalg.eigvalsh(Hm)
        m = min(k, n_levels)
        lev[sel, :m] = w[:, :m]
        hn[sel] = np.abs(Hm).sum(axis=2).max(axis=1)
    return lev, hn, tc


def _open_lists(dev, vg, vb, K):
    """the oracle's kept list of K states and the number of valid ones"""
    N = dev.n_dot
    v_ext = np.concatenate([vg, vb], axis=1)
    states, n_cont = O.candidate_states(v_ext, dev.cdd_inv_full, dev.cgd_full, N, k=K)
    cfg = O._delta_table(N)[None] + np.floor(n_cont)[:, None, :]
    return states, np.minimum(np.all(cfg >= 0, axis=-1).sum(axis=1), K)


def _compare(tag, lev, hn, lev_ref, hn_ref, hn_rtol=1e-14):
    """the module's bound at every point; prints the worst figures first"""
    lev, hn = _np(lev).reshape(lev_ref.shape), _np(hn).reshape(hn_ref.shape)
    fin = np.isfinite(lev_ref)
    assert np.array_equal(np.isposinf(lev), ~fin), tag                       # +inf exactly from nv on
    err = np.where(fin, np.abs(np.where(fin, lev, 0.0) - np.where(fin, lev_ref, 0.0)), 0.0) / hn_ref[:, None]
    dh = np.abs(hn - hn_ref) / hn_ref
    print(f"[levels] {tag}: worst |level - eigvalsh| / hnorm {err.max():.2e}, worst hnorm rel. difference {dh.max():.2e}, "
          f"valid levels per point {int(fin.sum(axis=1).min())}..{int(fin.sum(axis=1).max())}")
    assert np.isfinite(hn).all() and np.all(dh <= hn_rtol), (tag, float(dh.max()), hn_rtol)
    assert np.all(err <= BAR), (tag, float(err.max()))
    with np.errstate(invalid="ignore"):
        d = np.diff(np.where(fin, lev, np.inf), axis=1)
    assert not np.any(d < 0), tag                                            # in order (inf - inf = nan compares false)


# ------------------------------------------------------------------ 1. oracle parity, open
@pytest.mark.parametrize("N,K", [(2, 32), (3, 32), (4, 32), (8, 32), (8, 20), (8, 16), (8, 8)])
def test_open_levels_against_the_oracle(tmp_path, N, K):
    """64 points on each of three envs, spread around the ground truth as helpers.place spreads near, mid and far states.
    Measured: levels within 7.2e-15 hnorm, hnorm within 7.2e-15 (8 dots, far, tc up to 4e16); at 2 dots at most 16 states are
    valid, so all 8 levels are finite here and the +inf rule is met on the closed lists below."""
    L, C = layout(N), N - 1
    eb = H.sample_blocks(N, [41, 42, 43])
    rng = np.random.default_rng(8000 + 10 * N + K)
    vg, vb = [], []
    for e, mode in enumerate(("near", "mid", "far")):
        s, t = SPANS[mode]
        par, st = eb.params[e], eb.state[e]
        vg.append(_physical(L, par, st, st[L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-s, s, (64, N))))
        vb.append(st[L.s_barrier_gt:L.s_barrier_gt + C] + rng.uniform(-t, t, (64, C)))
    env = _vec(tmp_path, 3, N, 8, 41, num_charge_states=K)
    _load(env, eb.params, eb.state)
    out = env.eval_points([0, 1, 2], np.stack(vg), np.stack(vb), outputs=(), levels=8)
    assert set(out) == {"levels", "hnorm"} and out["levels"].shape == (3, 64, 8) and out["hnorm"].shape == (3, 64)
    for e, mode in enumerate(("near", "mid", "far")):
        dev = H.dev_view(N, eb.params[e])
        states, nv = _open_lists(dev, vg[e], vb[e], K)
        if N == 2:
            assert nv.max() <= 16
        lev_ref, hn_ref, tc = _spectrum(dev, vg[e], vb[e], states, nv)
        _compare(f"open N={N} K={K} {mode} (tc up to {tc.max():.1e})", out["levels"][e], out["hnorm"][e], lev_ref, hn_ref)
    env.close()


# ------------------------------------------------------------------ 2. the closed lists
@pytest.mark.parametrize("N", [2, 4, 8])
def test_closed_levels_against_the_sector_lists(tmp_path, N):
    seed = 8100 + N
    env = _vec(tmp_path, 2, N, 8, seed)
    env.reset(seed=seed)
    par = env._params_host[0].copy()
    dev = H.dev_view(N, par)
    vg, vb = CH.points(N, np.random.default_rng(seed + 1), 64)
    Qv = [1, N]
    out = env.eval_points([0, 0], np.stack([vg, vg]), np.stack([vb, vb]), n_charge=Qv, outputs=(), levels=8)
    for g, Q in enumerate(Qv):
        host = CH.host_closed(N, par, np.concatenate([vg, vb], axis=1), Q, 32)
        nv = np.minimum(host["nvalid"], 32)
        lev_ref, hn_ref, _ = _spectrum(dev, vg, vb, host["states"], nv)
        _compare(f"closed N={N} Q={Q}", out["levels"][g], out["hnorm"][g], lev_ref, hn_ref)
        if Q == 1:
            assert nv.max() <= N                                             # one carrier: N states at the most
    env.close()


# ------------------------------------------------------------------ 3. the known answer
def test_two_level_anticrossing(tmp_path):
    """2 dots, one carrier: H = [[E_10, -t], [-t, E_01]], level[1] - level[0] = sqrt(eps^2 + 4 t^2) along a detuning line"""
    N, seed = 2, 8200
    L = layout(N)
    env = _vec(tmp_path, 1, N, 8, seed)
    env.reset(seed=seed)
    par = env._params_host[0].copy()
    dev = H.dev_view(N, par)
    d = np.linspace(-0.6, 0.6, 33)
    vg = par[L.vopt:L.vopt + N + 1][None, :] + d[:, None] * np.array([1.0, -1.0, 0.0])[None, :]
    vb = np.broadcast_to(par[L.vbopt:L.vbopt + 1], (33, 1)).copy()
    out = env.eval_points([0], vg[None], vb[None], n_charge=1, outputs=(), levels=3)
    lev, hn = _np(out["levels"])[0], _np(out["hnorm"])[0]
    v_ext = np.concatenate([vg, vb], axis=1)
    st = np.broadcast_to(np.array([[1, 0], [0, 1]]), (33, 2, 2))
    F = O.free_energy_states(v_ext, dev.cdd_inv_full, dev.cgd_full, st, N)
    t = O.tunnel_couplings(O.effective_barrier_potential(vg, vb, dev.Cbg, dev.Cbb), dev.tc_base, dev.alpha)[:, 0]
    eps = F[:, 0] - F[:, 1]
    gap_ref = np.sqrt(eps ** 2 + 4 * t ** 2)
    hn_ref = np.abs(F).max(axis=1) + t
    err = np.abs((lev[:, 1] - lev[:, 0]) - gap_ref) / hn_ref
    print(f"[levels] anticrossing: eps {eps.min():.3e}..{eps.max():.3e}, t {t.min():.3e}..{t.max():.3e}, "
          f"worst |gap - sqrt(eps^2 + 4 t^2)| / hnorm {err.max():.2e}")
    assert np.all(err <= BAR) and np.all(np.isposinf(lev[:, 2])) and np.all(np.abs(hn - hn_ref) <= 1e-14 * hn_ref)
    mean_err = np.abs(0.5 * (lev[:, 0] + lev[:, 1]) - 0.5 * (F[:, 0] + F[:, 1])) / hn_ref
    assert np.all(mean_err <= BAR)
    env.close()


# ------------------------------------------------------------------ 4. zero couplings
def test_all_couplings_zero_gives_the_sorted_energies(tmp_path):
    """tc_base = 0: the levels are the sorted valid E.  Closed lists, whose E the host build of the same source hands out: within
    2 eps hnorm (the shift out and the shift in).  Open lists against the oracle's free energies: the module's bound."""
    N, seed = 4, 8300
    L = layout(N)
    env = _vec(tmp_path, 1, N, 8, seed)
    env.reset(seed=seed)
    params = env._params_host.copy()
    params[0, L.scal] = 0.0
    st, _ = env.get_state()
    _load(env, params, st)
    par = params[0]
    dev = H.dev_view(N, par)
    vg, vb = CH.points(N, np.random.default_rng(seed + 1), 64)
    for Q in (1, 3, N + 2):
        out = env.eval_points([0], vg[None], vb[None], n_charge=Q, outputs=(), levels=8)
        lev, hn = _np(out["levels"])[0], _np(out["hnorm"])[0]
        host = CH.host_closed(N, par, np.concatenate([vg, vb], axis=1), Q, 32)
        worst = 0.0
        for p in range(64):
            nv = int(min(host["nvalid"][p], 32))
            E = np.sort(host["E"][p, :nv])
            m = min(nv, 8)
            hn_ref = np.abs(E).max()
            assert abs(hn[p] - hn_ref) <= 1e-14 * hn_ref and np.all(np.isposinf(lev[p, m:]))
            worst = max(worst, float(np.abs(lev[p, :m] - E[:m]).max() / hn_ref))
        print(f"[levels] all couplings zero, closed Q={Q}: worst |level - sorted E| / hnorm {worst:.2e} (bound {2 * EPS:.2e})")
        assert worst <= 2 * EPS
    out = env.eval_points([0], vg[None], vb[None], outputs=(), levels=8)
    states, nv = _open_lists(dev, vg, vb, 32)
    lev_ref, hn_ref, tc = _spectrum(dev, vg, vb, states, nv)
    assert not tc.any()
    _compare("all couplings zero, open", out["levels"][0], out["hnorm"][0], lev_ref, hn_ref)
    env.close()


@pytest.mark.parametrize("name", ["cut_pair", "cut_two"])
def test_cut_pairs_follow_the_oracle(tmp_path, name):
    """designed 5-dot devices whose sector falls apart along the pairs with tc == 0 exactly: the levels of disconnected
    components cross along the scan and come back in order"""
    N, R = 5, 16
    par, st = GC.make(name, N, R)
    env = _vec(tmp_path, 1, N, R, 8400)
    _load(env, par[None], st[None])
    dev = H.dev_view(N, par)
    vs, refs = [], []
    for ch in (0, 3):
        c = GC.census(name, N, R, ch)
        pix = np.arange(0, R * R, 4)                                            # 64 pixels of the channel
        v_ext = PH.scan_voltages(N, par, st, ch, R)[0][pix]
        assert all((c["tc"][:, b] == 0.0).all() for b in GC.CUT[name]) and (np.delete(c["tc"], GC.CUT[name], axis=1) != 0).all()
        vs.append(v_ext)
        refs.append(_spectrum(dev, v_ext[:, :N + 1], v_ext[:, N + 1:], np.asarray(c["states"])[pix], np.full(pix.size, 32)))
    v = np.concatenate(vs)
    out = env.eval_points([0], v[None, :, :N + 1], v[None, :, N + 1:], outputs=(), levels=8)
    lev_ref, hn_ref = np.concatenate([r[0] for r in refs]), np.concatenate([r[1] for r in refs])
    _compare(name, out["levels"][0], out["hnorm"][0], lev_ref, hn_ref)
    env.close()


# ------------------------------------------------------------------ 5. large couplings
@pytest.mark.parametrize("N", [4, 8])
def test_large_couplings(tmp_path, N):
    """Barrier voltages that put tc between 1e30 and 1e45 (and, on the last barrier, back at O(1)): finite output, the same bound
    on the levels.  The norm is all couplings here, and tc = tc_base exp(-a) with a = alpha (vb + Cbg . vg) up to 110: the device
    and NumPy sum the N + 2 products of a in different orders, each within (N + 2) eps / 2 of the sum of their magnitudes (a
    itself, to a factor of order one), and exp turns an absolute error of a into a relative error of tc.  So hnorm is compared
    within 1e-14 + (N + 2) eps max|a| (8 dots at |a| = 105: 2.4e-13; measured 1.4e-14 at one point of 64, 0 at most)."""
    L, C = layout(N), N - 1
    eb = H.sample_blocks(N, [51])
    par, st = eb.params[0], eb.state[0]
    dev = H.dev_view(N, par)
    rng = np.random.default_rng(8500 + N)
    n = 64
    vg = _physical(L, par, st, st[L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-3, 3, (n, N)))
    want = 10.0 ** rng.uniform(30, 45, (n, C))
    want[:, -1] = 10.0 ** rng.uniform(-2, 1, n)
    base = O.tunnel_couplings(O.effective_barrier_potential(vg, np.zeros((n, C)), dev.Cbg, dev.Cbb), dev.tc_base, dev.alpha)
    vb = -np.log(want / base) / dev.alpha[None, :]
    env = _vec(tmp_path, 1, N, 8, 51)
    _load(env, eb.params, eb.state)
    out = env.eval_points([0], vg[None], vb[None], outputs=(), levels=8)
    states, nv = _open_lists(dev, vg, vb, 32)
    lev_ref, hn_ref, tc = _spectrum(dev, vg, vb, states, nv)
    assert tc.max() > 1e30 and tc[:, :-1].min() > 1e29
    assert np.isfinite(_np(out["levels"])[0][np.isfinite(lev_ref)]).all()
    a_max = float(np.abs(np.log(tc / dev.tc_base)).max())
    _compare(f"large couplings N={N} (tc up to {tc.max():.1e}, |a| up to {a_max:.0f})", out["levels"][0], out["hnorm"][0], lev_ref, hn_ref,
             hn_rtol=1e-14 + (N + 2) * EPS * a_max)
    env.close()


# ------------------------------------------------------------------ 6. slots, launch chunks, padding
def test_groups_across_slot_and_chunk_boundaries(tmp_path):
    """N = 4, R = 4: a slot holds C P = 48 points and env_chunk = 2 puts two slots in a launch.  Groups of 1, 48, 49 and 243
    points and two empty ones in one call against every group alone, bit for bit; then the C call with guard rows."""
    import torch
    from qadapt_hip import _lib
    N, R, B, seed = 4, 4, 3, 8600
    L, G, C = layout(N), N + 1, N - 1
    env = _vec(tmp_path, B, N, R, seed, env_chunk=2)
    assert env.chunk_envs() == 2
    env.load_new_devices(seed=seed)
    st, _ = env.get_state()
    CP = C * R * R
    sizes, envs = [1, 0, CP, CP + 1, 0, 5 * CP + 3], np.array([0, 2, 1, 2, 1, 0], np.int32)
    rng = np.random.default_rng(99)
    vgs, vbs = [], []
    for n, e in zip(sizes, envs):
        virt = st[e, L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-3, 3, (n, N))
        vgs.append(_physical(L, env._params_host[e], st[e], virt))
        vbs.append(st[e, L.s_barrier_gt:L.s_barrier_gt + C] + rng.uniform(-3, 3, (n, C)))
    vgs, vbs = [torch.as_tensor(v).cuda() for v in vgs], [torch.as_tensor(v).cuda() for v in vbs]
    out = env.eval_points(envs, vgs, vbs, levels=8)
    assert [tuple(t.shape) for t in out["levels"]] == [(n, 8) for n in sizes]
    assert [tuple(t.shape) for t in out["hnorm"]] == [(n,) for n in sizes]
    keys = ("levels", "hnorm", "signal", "occupations")
    for g, (n, e) in enumerate(zip(sizes, envs)):
        if n == 0:
            continue
        alone = env.eval_points([int(e)], vgs[g][None], vbs[g][None], levels=8)
        for key in keys:
            assert PH.same(alone[key][0], out[key][g]), (key, g)
        assert np.isfinite(_np(out["levels"][g][:, 0])).all() and np.all(_np(out["hnorm"][g]) > 0)
    only = env.eval_points(envs, vgs, vbs, outputs=(), levels=8)
    again = env.eval_points(envs, vgs, vbs, outputs=(), levels=8)
    for key in ("levels", "hnorm"):
        assert PH.same(torch.cat(only[key]), torch.cat(out[key])) and PH.same(torch.cat(again[key]), torch.cat(out[key])), key
    # the C entry point with guard rows on both sides of the caller's buffers; three levels: another row length
    g0, g1, npts, nl = 5, 7, sum(sizes), 3
    start = (g0 + np.concatenate([[0], np.cumsum(sizes)])).astype(np.int64)
    vg_all = torch.full((g0 + npts + g1, G), float("nan"), dtype=torch.float64, device="cuda")
    vb_all = torch.full((g0 + npts + g1, C), float("nan"), dtype=torch.float64, device="cuda")
    vg_all[g0:g0 + npts] = torch.cat(vgs); vb_all[g0:g0 + npts] = torch.cat(vbs)
    guard = -12345.678
    l_dst = torch.full((g0 + npts + g1, nl), guard, dtype=torch.float64, device="cuda")
    h_dst = torch.full((g0 + npts + g1,), guard, dtype=torch.float64, device="cuda")
    opts = _lib.QdPointsOpts(struct_size=ctypes.sizeof(_lib.QdPointsOpts), n_levels=nl, levels_dst=l_dst.data_ptr(),
                             hnorm_dst=h_dst.data_ptr())
    rc = env._lib.qd_eval_points_ex(env._h, envs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                    start.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(sizes),
                                    ctypes.c_void_p(vg_all.data_ptr()), ctypes.c_void_p(vb_all.data_ptr()), None, None,
                                    ctypes.byref(opts), env._stream())
    assert rc == 0
    l_h, h_h = l_dst.cpu().numpy(), h_dst.cpu().numpy()
    for a in (l_h, h_h):
        assert np.all(a[:g0] == guard) and np.all(a[g0 + npts:] == guard)
    assert PH.same(h_h[g0:g0 + npts], torch.cat(out["hnorm"]))
    full = _np(torch.cat(out["levels"]))
    assert np.abs(l_h[g0:g0 + npts] - full[:, :nl]).max() <= 2 * BAR * h_h[g0:g0 + npts].max()      # (other sections, same eigenvalues)
    # hnorm_dst may be NULL
    opts.hnorm_dst = None
    l2 = torch.full_like(l_dst, guard)
    opts.levels_dst = l2.data_ptr()
    rc = env._lib.qd_eval_points_ex(env._h, envs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                    start.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(sizes),
                                    ctypes.c_void_p(vg_all.data_ptr()), ctypes.c_void_p(vb_all.data_ptr()), None, None,
                                    ctypes.byref(opts), env._stream())
    assert rc == 0 and PH.same(l2, l_dst)
    env.close()


# ------------------------------------------------------------------ 7. nothing else moves
@pytest.mark.parametrize("K", [32, 20])
def test_signal_and_occupations_keep_their_bits(tmp_path, K):
    """eval_points(levels=2) against eval_points(), open and closed; a levels-only call between two plain calls changes
    neither; the options struct without levels is the plain call"""
    import torch
    from qadapt_hip import _lib
    N, R, seed = 4, 8, 8700 + K
    L, C = layout(N), N - 1
    env = _vec(tmp_path, 2, N, R, seed, num_charge_states=K)
    env.reset(seed=seed)
    vg, vb = CH.points(N, np.random.default_rng(seed), 200)             # 200 points: two slots of C P = 192
    vg, vb = np.stack([vg, vg[::-1]]), np.stack([vb, vb[::-1]])
    for kw in ({}, {"n_charge": [2, 5]}):
        plain = env.eval_points([0, 1], vg, vb, **kw)
        only = env.eval_points([1, 0], vg, vb, outputs=(), levels=8, **kw)
        assert set(only) == {"levels", "hnorm"}
        after = env.eval_points([0, 1], vg, vb, **kw)
        both = env.eval_points([0, 1], vg, vb, levels=2, **kw)
        for key in ("signal", "occupations"):
            assert PH.same(plain[key], after[key]) and PH.same(plain[key], both[key]), (key, kw)
        sig_only = env.eval_points([0, 1], vg, vb, outputs=("signal",), levels=2, **kw)
        assert PH.same(sig_only["signal"], plain["signal"]) and PH.same(sig_only["levels"], both["levels"])
        # n_levels == 0 through the new entry point: the plain call
        g_all = torch.as_tensor(vg.reshape(-1, N + 1)).cuda(); b_all = torch.as_tensor(vb.reshape(-1, C)).cuda()
        s_dst = torch.zeros(400, dtype=torch.float64, device="cuda"); o_dst = torch.zeros((400, N), dtype=torch.float64, device="cuda")
        ids, start = np.array([0, 1], np.int32), np.array([0, 200, 400], np.int64)
        opts = _lib.QdPointsOpts(struct_size=ctypes.sizeof(_lib.QdPointsOpts), n_levels=0)
        q = np.array(kw.get("n_charge", [0, 0]), np.int32)
        if kw:
            opts.n_charge_host = q.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        for o in (ctypes.byref(opts), None) if not kw else (ctypes.byref(opts),):
            s_dst.zero_(); o_dst.zero_()
            rc = env._lib.qd_eval_points_ex(env._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                            start.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 2, ctypes.c_void_p(g_all.data_ptr()),
                                            ctypes.c_void_p(b_all.data_ptr()), ctypes.c_void_p(s_dst.data_ptr()),
                                            ctypes.c_void_p(o_dst.data_ptr()), o, env._stream())
            assert rc == 0 and PH.same(s_dst.reshape(2, 200), plain["signal"]) and PH.same(o_dst.reshape(2, 200, N), plain["occupations"])
    env.close()


def test_levels_leave_no_footprint_on_a_noisy_run(tmp_path):
    """the footprint test of test_gpu_points.py with levels calls interleaved: all stochastic stages on, env_chunk = 2, a rollout
    of 3 steps through a truncation with automatic resets; state blocks, parameter blocks, raw signal, percentiles,
    observations and the observation serial are byte-identical with and without the calls"""
    import torch
    N, R, B, seed, max_steps = 4, 16, 3, 2719, 2
    L, C = layout(N), N - 1
    path = _cfg(tmp_path, max_steps=max_steps)
    plain, poked = [_vec(tmp_path, B, N, R, seed, config_path=path, noise=("sensor", "radial", "latch"), env_chunk=2)
                    for _ in range(2)]
    prng = np.random.default_rng(8)
    calls = [0]

    def poke():
        n = (2, 1, B)[calls[0] % 3]
        m = (800, 1, 130)[calls[0] % 3]                             # more than a slot (C P = 768), one point, a part of a slot
        k = calls[0]
        calls[0] += 1
        ids = prng.integers(0, B, n)
        par = poked._params_host[ids]
        vg = par[:, None, L.vopt:L.vopt + N + 1] + prng.uniform(-4, 4, (n, m, N + 1))
        vb = par[:, None, L.vbopt:L.vbopt + C] + prng.uniform(-3, 3, (n, m, C))
        kw = dict(outputs=((), ("signal",), ("signal", "occupations"))[k % 3], levels=(8, 2, 3)[k % 3])
        if k % 2:
            kw["n_charge"] = 3
        out = poked.eval_points(ids, vg, vb, **kw)
        assert np.isfinite(_np(out["hnorm"])).all() and np.isfinite(_np(out["levels"])[..., 0]).all()

    def snapshot(env, obs, rew=None, trunc=None):
        st, steps = env.get_state()
        raw, plohi = env.raw()
        ser = ctypes.c_uint64(0)
        assert env._lib.qd_get_rng_state(env._h, ctypes.byref(ser)) == 0
        d = {k: obs[k].cpu().numpy().copy() for k in ("image", "obs_gate_voltages", "obs_barrier_voltages")}
        d.update(state=st, steps=steps, raw=raw, plohi=plohi, serial=np.array([ser.value], np.uint64),
                 params=env._params_host.copy())
        if rew is not None:
            d.update(rew=rew.cpu().numpy().copy(), trunc=trunc.cpu().numpy().astype(np.uint8))
        return d

    trace = [[], []]
    for k, env in enumerate((plain, poked)):
        trace[k].append(snapshot(env, env.reset(seed=seed)))
    poke()
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
    plain.close(); poked.close()


# ------------------------------------------------------------------ 8. refusals on the device
def test_refusals_on_the_device(tmp_path):
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
        for more in ({}, {"n_charge": 2}, {"outputs": ()}):
            with pytest.raises(_lib.QdError, match=word) as ei:
                env.eval_points([0], zg, zb, levels=2, **more)
            assert f"code {_lib.QD_ERR_STATE}" in str(ei.value) and "qd_eval_points_ex" in str(ei.value)
        assert PH.same(env.raw()[0], raw0)
        env.close()
    env = _vec(tmp_path, 1, N, R, 78)
    env.reset(seed=78)
    for bad in (-1, 9):
        with pytest.raises(ValueError, match="levels"):
            env.eval_points([0], zg, zb, levels=bad)
    with pytest.raises(ValueError, match="outputs"):
        env.eval_points([0], zg, zb, outputs=())
    vg, vb = CH.points(N, np.random.default_rng(5), 4)
    before = env.eval_points([0], vg[None], vb[None], levels=4)
    g_d, b_d = torch.as_tensor(vg).cuda(), torch.as_tensor(vb).cuda()
    dst = torch.zeros(64, dtype=torch.float64, device="cuda")
    ids, start = np.array([0], np.int32), np.array([0, 4], np.int64)
    size = ctypes.sizeof(_lib.QdPointsOpts)
    cases = [(dict(struct_size=size - 8, n_levels=2, levels_dst=dst.data_ptr()), "struct_size"),
             (dict(struct_size=size, n_levels=-1, levels_dst=dst.data_ptr()), "n_levels"),
             (dict(struct_size=size, n_levels=9, levels_dst=dst.data_ptr()), "n_levels"),
             (dict(struct_size=size, n_levels=2), "levels_dst"),
             (dict(struct_size=size, n_levels=2, levels_dst=dst.data_ptr(), states_dst=dst.data_ptr()), "states_dst")]
    for fields, word in cases:
        opts = _lib.QdPointsOpts(**fields)
        rc = env._lib.qd_eval_points_ex(env._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                        start.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1, ctypes.c_void_p(g_d.data_ptr()),
                                        ctypes.c_void_p(b_d.data_ptr()), None, None, ctypes.byref(opts), env._stream())
        msg = env._lib.qd_last_error(env._h).decode()
        assert rc == _lib.QD_ERR_ARG and msg.startswith("qd_eval_points_ex") and word in msg, (fields, rc, msg)
        assert not _np(dst).any()
        after = env.eval_points([0], vg[None], vb[None], levels=4)                    # the handle is usable
        for key in before:
            assert PH.same(before[key], after[key]), (word, key)
    env.close()


# ------------------------------------------------------------------ 9. the facade
def test_facade_energy_levels(tmp_path):
    from qadapt_hip.env import QuantumDeviceEnv
    N, R = 3, 8
    path = _cfg(tmp_path, num_dots=N, resolution=R)
    backend = _vec(tmp_path, 1, N, R, 8900, config_path=path)
    env = QuantumDeviceEnv(config_path=path, num_dots=N, backend=backend)
    model = env.array.model
    vg, vb = CH.points(N, np.random.default_rng(6), 12)
    for lead in ((12,), (3, 4), ()):
        g = vg.reshape(lead + (N + 1,)) if lead else vg[0]
        b = vb.reshape(lead + (N - 1,)) if lead else vb[0]
        n = 12 if lead else 1
        lev, hn = model.energy_levels_open(g, b)
        assert lev.shape == lead + (2,) and hn.shape == lead and lev.dtype == hn.dtype == np.float64
        want = backend.eval_points([0], vg[None, :n], vb[None, :n], outputs=(), levels=2)
        assert PH.same(lev.reshape(n, 2), want["levels"][0]) and PH.same(hn.reshape(n), want["hnorm"][0])
        lev, hn = model.energy_levels_closed(g, 2, n_levels=5, vb=b)
        assert lev.shape == lead + (5,) and hn.shape == lead
        want = backend.eval_points([0], vg[None, :n], vb[None, :n], outputs=(), levels=5, n_charge=2)
        assert PH.same(lev.reshape(n, 5), want["levels"][0]) and PH.same(hn.reshape(n), want["hnorm"][0])
        assert np.all((lev[..., 1] - lev[..., 0]) / hn >= 0)
    with pytest.raises(NotImplementedError):
        model.energy_levels_open(vg)
    env.close()


# ------------------------------------------------------------------ 10. more than one point per block
TRIP_BLOCKS = 4096                                       # blocks per slot of qd_k_levels / qd_k_thermal, at most


def _second_trip_points(N, R):
    """C P points on one 3-dot device (R = 48: C P = 4608, the smallest slot above 4096), ordered for a launch whose blocks stride
    over a full slot: block j solves point j and, for j < C P - 4096, point j + 4096 on the same __shared__ workspace.  Around the
    optimum the oracle keeps 32 valid states where a floor is above zero and 27 (the deltas 0, 1, 2 of every dot) where the array
    is empty: the first trip of those blocks gets lists of 32, their second trip lists of 27, the odd size whose idle index the
    Jacobi ordering needs zeroed.  -> (params, state, dev, vg, vb, states, nv) with the oracle's kept lists"""
    CP = (N - 1) * R * R
    assert CP > TRIP_BLOCKS
    eb = H.sample_blocks(N, [61])
    par = eb.params[0]
    L = layout(N)
    dev = H.dev_view(N, par)
    rng = np.random.default_rng(8950)
    vg = par[L.vopt:L.vopt + N + 1] + rng.uniform(-4, 4, (CP, N + 1))
    vb = par[L.vbopt:L.vbopt + N - 1] + rng.uniform(-3, 3, (CP, N - 1))
    states, nv = _open_lists(dev, vg, vb, 32)
    again = CP - TRIP_BLOCKS
    big, small = np.flatnonzero(nv == nv.max()), np.flatnonzero(nv < nv.max())
    assert big.size >= again and small.size >= again, (big.size, small.size)
    head, tail = big[:again], small[-again:]
    rest = np.setdiff1d(np.arange(CP), np.concatenate([head, tail]))
    order = np.concatenate([head, rest, tail])
    vg, vb, states, nv = vg[order], vb[order], states[order], nv[order]
    first, second = nv[:again], nv[TRIP_BLOCKS:]
    assert np.sum(second < first) >= 100, "too few blocks that see a smaller block after a larger one"
    assert np.any((second % 2 == 1) & (first % 2 == 0) & (first > second)), "no block sees an odd size after a larger even one"
    return eb.params, eb.state, dev, vg, vb, states, nv


def _subsample(CP):
    """256 points of the slot: of the first and of the second trip, and from the blocks that take one trip"""
    pick = np.concatenate([np.arange(0, 64), np.arange(TRIP_BLOCKS, TRIP_BLOCKS + 64),
                           np.random.default_rng(8951).choice(np.arange(64, TRIP_BLOCKS), 128, replace=False)])
    assert pick.size == 256 and pick.max() < CP
    return pick


def test_second_point_of_a_block_keeps_nothing_from_the_first(tmp_path):
    """one group of exactly C P points fills one slot, whose 4096 blocks stride over it: 512 of them solve a second point.  The
    same points as two groups of half the size (two slots, one point per block): the same levels and norm, bit for bit, and 256
    of those within the module's bound of the oracle, so that the equality is not one of two wrong answers"""
    N, R = 3, 48
    params, state, dev, vg, vb, states, nv = _second_trip_points(N, R)
    CP = vg.shape[0]
    env = _vec(tmp_path, 1, N, R, 61)
    _load(env, params, state)
    one = env.eval_points([0], vg[None], vb[None], outputs=(), levels=8)
    half = CP // 2
    two = env.eval_points([0, 0], vg.reshape(2, half, N + 1), vb.reshape(2, half, N - 1), outputs=(), levels=8)
    lev1, hn1 = _np(one["levels"]).reshape(CP, 8), _np(one["hnorm"]).reshape(CP)
    lev2, hn2 = _np(two["levels"]).reshape(CP, 8), _np(two["hnorm"]).reshape(CP)
    diff = np.flatnonzero((lev1.view(np.uint64) != lev2.view(np.uint64)).any(axis=1) | (hn1.view(np.uint64) != hn2.view(np.uint64)))
    assert diff.size == 0, (diff.size, diff[:8], nv[diff[:8]])
    pick = _subsample(CP)
    lev_ref, hn_ref, tc = _spectrum(dev, vg[pick], vb[pick], states[pick], nv[pick])
    _compare(f"two trips N={N} R={R} (tc up to {tc.max():.1e})", lev2[pick], hn2[pick], lev_ref, hn_ref)
    env.close()
