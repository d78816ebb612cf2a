"""Point evaluation on the MI355X (run with -m gpu): qd_eval_points at the voltages of a scan's pixels against the scan path
bit for bit, slot and launch-chunk boundaries with padded groups, free points with a barrier setting per point against the
oracle, its absent footprint on a noisy auto-resetting run, and the refusals."""
import ctypes

import numpy as np
import pytest
import yaml

import helpers as H
import points_helpers as PH
import qd_oracle as O
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


def _physical(L, par, st, virt):
    """virtual plunger voltages (n, N) with the sensor at its ground truth -> physical gate voltages (n, N+1)"""
    G = L.N + 1
    vgm = st[L.s_vgm:L.s_vgm + G * G].reshape(G, G)
    full = np.concatenate([virt, np.full((virt.shape[0], 1), st[L.s_sensor_gt])], axis=1)
    return full @ vgm.T + par[L.origin:L.origin + G]


# ------------------------------------------------------------------ 1. the bits of the scan path
SCAN_CASES = [(4, 8, 32, False), (8, 8, 32, False), (8, 8, 16, False), (8, 8, 20, False), (2, 8, 32, False), (3, 8, 32, False),
              (4, 8, 32, True)]
_SCAN = {}


def _scan_case(tmp_path, N, R, K, linear):
    """One case of SCAN_CASES, rendered once for its two tests.  Two envs, "near" and "far"; both handles run the per-pixel
    search (pixel_search=True) with a constant peak width.  The points are the v_ext of every pixel of every channel, from
    the host build of qd_pixel_voltages.  Returns the points' signal and occupations (product handle), that handle's probe
    at the same state, and the occupations of a validate handle after set_state + observe."""
    key = (N, R, K, linear)
    if key not in _SCAN:
        B, seed, L, C, P = 2, 5200 + 10 * N + K, layout(N), N - 1, R * R
        kw = dict(pixel_search=True, num_charge_states=K)
        if linear:
            kw["voltage_capacitance_model"] = "linear"
        env = _vec(tmp_path, B, N, R, seed, **kw)
        val = _vec(tmp_path, B, N, R, seed, validate=True, **kw)
        for e in (env, val):
            e.load_new_devices(seed=seed)
        params = env._params_host.copy()
        assert np.array_equal(params, val._params_host) and bool(params[0, L.scal + 4] != 0.0) == linear
        st, steps = env.get_state()
        rng = np.random.default_rng(seed)
        for e, mode in enumerate(("near", "far")):
            st[e] = H.place(N, st[e], mode, rng)
        env.set_state(st, steps)
        v_ext = np.stack([PH.scan_points(N, params[e], st[e], R) for e in range(B)])             # (B, C P, 2N)
        out = env.eval_points(np.arange(B), v_ext[..., :N + 1], v_ext[..., N + 1:])
        assert out["signal"].shape == (B, C * P) and out["occupations"].shape == (B, C * P, N)
        raw = env.probe(np.arange(B), st[:, L.s_gate_v:L.s_gate_v + N], st[:, L.s_barrier_v:L.s_barrier_v + C],
                        sensor_voltage=st[:, L.s_sensor_gt])["raw"]
        val.set_state(st, steps)
        val.observe()
        _SCAN[key] = dict(sig=out["signal"].cpu().numpy(), occ=out["occupations"].cpu().numpy(),
                          raw=raw.cpu().numpy().reshape(B, C * P), occ_val=val.occupations().reshape(B, C * P, N))
        env.close(); val.close()
    return _SCAN[key]


@pytest.mark.parametrize("N,R,K,linear", SCAN_CASES)
def test_points_at_the_pixels_of_a_scan_have_the_probe_signal_bits(tmp_path, N, R, K, linear):
    """K = 20 runs the kept-set size 32 and hands over the first 20 of the ordered list; 2 and 3 dots have fewer than 32
    valid candidates (|0..0> padding) and no tile search, so the redo instantiation of the search runs for them here only."""
    c = _scan_case(tmp_path, N, R, K, linear)
    assert np.isfinite(c["sig"]).all() and np.ptp(c["sig"]) > 0
    assert PH.same(c["sig"], c["raw"]), int((PH.bits(c["sig"]) != PH.bits(c["raw"])).sum())


@pytest.mark.parametrize("N,R,K,linear", SCAN_CASES)
def test_points_at_the_pixels_of_a_scan_have_the_validate_occupation_bits(tmp_path, N, R, K, linear):
    """The points' occupations (product handle) against `occupations()` of a validate handle after set_state + observe, as
    64-bit patterns.  With K == KC (32, 16) a product handle's search leaves the kept set in search order, which is what its
    signal is solved from, and a validate handle orders it by (E, index); the structure kernel ranks a component's states by
    record slot, so the two orders give eigenvectors that differ by rounding (measured before the points sorted their
    records: (4, 8, 32) 327 of 384 rows, up to 6.5e-10; (8, 8, 32) 757 of 896, up to 1.1e-9).  qd_eval_points therefore
    brings the records into the reference order (qd_k_points_sort) and solves again for the occupations."""
    c = _scan_case(tmp_path, N, R, K, linear)
    nd = int((PH.bits(c["occ"]) != PH.bits(c["occ_val"])).any(axis=-1).sum())
    print(f"[points vs validate] N={N} R={R} K={K} linear={linear}: occupation rows that differ {nd} of {c['occ'].shape[0] * c['occ'].shape[1]}, "
          f"largest difference {np.abs(c['occ'] - c['occ_val']).max():.3e}")
    assert PH.same(c["occ"], c["occ_val"]), nd


# ------------------------------------------------------------------ 2. slots, launch chunks, padding
def test_groups_across_slot_and_chunk_boundaries(tmp_path):
    """N = 4, R = 8: a slot holds C P = 192 points and env_chunk = 2 puts two slots in a launch.  Groups of 1, 191, 192, 193
    and 500 points (1 + 1 + 1 + 2 + 3 slots, four launches) on three envs in one call against every point alone."""
    import torch
    N, R, B, seed = 4, 8, 3, 4711
    L, G, C = layout(N), N + 1, N - 1
    env = _vec(tmp_path, B, N, R, seed, env_chunk=2)
    assert env.chunk_envs() == 2
    env.load_new_devices(seed=seed)
    st, _ = env.get_state()
    sizes, envs = [1, 191, 192, 193, 500], np.array([0, 1, 2, 1, 0], np.int32)
    rng = np.random.default_rng(99)
    vgs, vbs = [], []
    for n, e in zip(sizes, envs):
        virt = st[e, L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-3, 3, (n, N))
        vgs.append(_physical(L, env._params_host[e], st[e], virt))
        vbs.append(st[e, L.s_barrier_gt:L.s_barrier_gt + C] + rng.uniform(-3, 3, (n, C)))
    # ragged lists through the Python entry point
    out = env.eval_points(envs, vgs, vbs)
    assert [tuple(t.shape) for t in out["signal"]] == [(n,) for n in sizes]
    assert [tuple(t.shape) for t in out["occupations"]] == [(n, N) for n in sizes]
    sig = torch.cat(out["signal"]).cpu().numpy(); occ = torch.cat(out["occupations"]).cpu().numpy()
    assert np.isfinite(sig).all() and np.isfinite(occ).all() and np.ptp(sig) > 0
    # every point alone
    vg_d = [torch.as_tensor(v).cuda() for v in vgs]; vb_d = [torch.as_tensor(v).cuda() for v in vbs]
    alone_s, alone_o = [], []
    for g, (n, e) in enumerate(zip(sizes, envs)):
        for i in range(n):
            o = env.eval_points([int(e)], vg_d[g][i:i + 1][None], vb_d[g][i:i + 1][None])
            alone_s.append(o["signal"].reshape(1)); alone_o.append(o["occupations"].reshape(1, N))
    assert PH.same(torch.cat(alone_s), sig) and PH.same(torch.cat(alone_o), occ)
    # the C entry point with guard rows on both sides of the caller's buffers
    g0, g1, npts = 5, 7, sum(sizes)
    start = (g0 + np.concatenate([[0], np.cumsum(sizes)])).astype(np.int64)
    vg_all = torch.full((g0 + npts + g1, G), float("nan"), dtype=torch.float64, device="cuda")
    vb_all = torch.full((g0 + npts + g1, C), float("nan"), dtype=torch.float64, device="cuda")
    vg_all[g0:g0 + npts] = torch.cat(vg_d); vb_all[g0:g0 + npts] = torch.cat(vb_d)
    guard = -12345.678
    s_dst = torch.full((g0 + npts + g1,), guard, dtype=torch.float64, device="cuda")
    o_dst = torch.full((g0 + npts + g1, N), guard, dtype=torch.float64, device="cuda")
    gam = np.full(len(sizes), 0.31)
    rc = env._lib.qd_eval_points(env._h, envs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                 start.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(sizes),
                                 ctypes.c_void_p(vg_all.data_ptr()), ctypes.c_void_p(vb_all.data_ptr()),
                                 gam.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                 ctypes.c_void_p(s_dst.data_ptr()), ctypes.c_void_p(o_dst.data_ptr()), env._stream())
    assert rc == 0
    s_h, o_h = s_dst.cpu().numpy(), o_dst.cpu().numpy()
    for a in (s_h, o_h):
        assert np.all(a[:g0] == guard) and np.all(a[g0 + npts:] == guard)
    assert PH.same(o_h[g0:g0 + npts], occ)                             # the peak width does not reach the occupations
    wide = env.eval_points(envs, vgs, vbs, gamma=0.31)
    assert PH.same(torch.cat(wide["signal"]), s_h[g0:g0 + npts]) and not PH.same(s_h[g0:g0 + npts], sig)
    # either destination may be NULL
    s_dst.fill_(guard)
    rc = env._lib.qd_eval_points(env._h, envs.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                 start.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(sizes),
                                 ctypes.c_void_p(vg_all.data_ptr()), ctypes.c_void_p(vb_all.data_ptr()), None,
                                 ctypes.c_void_p(s_dst.data_ptr()), None, env._stream())
    assert rc == 0 and PH.same(s_dst[g0:g0 + npts], sig)
    env.close()


# ------------------------------------------------------------------ 3. what a scan cannot do, against the oracle
ORACLE_MODES = {"near": (3.0, 3.0), "mid": (10.0, 6.0)}
_ORACLE = {}


def _oracle_case(N, mode):
    """Devices of seeds 41, 42, 43; per env 64 points gate_gt + U(-s, s)^N (virtual, sensor at its ground truth, through the
    state's VGM and origin) with a different vb = barrier_gt + U(-t, t) at every point; the oracle's occupations, signal and
    relative gap per point.  Computed once per case."""
    if (N, mode) not in _ORACLE:
        s, t = ORACLE_MODES[mode]
        L, C = layout(N), N - 1
        eb = H.sample_blocks(N, [41, 42, 43])
        rng = np.random.default_rng(7000 + 10 * N + len(mode))
        vg, vb, ref = [], [], []
        for e in range(3):
            par, st = eb.params[e], eb.state[e]
            virt = st[L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-s, s, (64, N))
            vg.append(_physical(L, par, st, virt))
            vb.append(st[L.s_barrier_gt:L.s_barrier_gt + C] + rng.uniform(-t, t, (64, C)))
            dev = H.dev_view(N, par)
            n, states, F, tc = O.ground_state_open(dev, vg[e], vb[e], return_states=True)
            sig, _ = O.charge_sensor_open(dev, vg[e], vb[e], n_open=n)
            Hm = F[:, :, None] * np.eye(states.shape[1]) + O.tunnel_hamiltonian(tc, states)
            w = np.linalg.eigvalsh(Hm)
            hn = np.abs(Hm).sum(axis=2).max(axis=1)
            ref.append(dict(occ=n, sig=sig[:, 0], rel_gap=(w[:, 1] - w[:, 0]) / hn))
        _ORACLE[(N, mode)] = (eb, np.stack(vg), np.stack(vb), ref)
    return _ORACLE[(N, mode)]


@pytest.mark.parametrize("mode", ["near", "mid"])
@pytest.mark.parametrize("N", [4, 6, 8])
def test_free_points_against_the_oracle(tmp_path, N, mode):
    """The rule of test_gpu_parity._check_channel without its eigenvalue lines (product handles keep none)."""
    eb, vg, vb, ref = _oracle_case(N, mode)
    unres = sum(int((r["rel_gap"] <= H.GAP_MIN).sum()) for r in ref)
    assert unres <= 0.05 * 192, f"the oracle alone leaves {unres} of 192 points unresolved"
    env = _vec(tmp_path, 3, N, 8, 41)
    _load(env, eb.params, eb.state)
    out = env.eval_points([0, 1, 2], vg, vb)
    occ, sig = out["occupations"].cpu().numpy(), out["signal"].cpu().numpy()
    for e in range(3):
        r = ref[e]
        ok = r["rel_gap"] > H.GAP_MIN
        d_occ = np.abs(occ[e] - r["occ"]).max(axis=1)
        d_sig = np.abs(sig[e] - r["sig"]) / np.maximum(np.abs(r["sig"]), 1e-3)
        print(f"[points vs oracle] N={N} {mode} env {e}: worst occupation {d_occ[ok].max():.3e}, worst signal {d_sig[ok].max():.3e}, "
              f"unresolved {int((~ok).sum())}")
        assert np.all(r["rel_gap"][d_occ > 1e-6] <= H.GAP_MIN), (e, d_occ[ok].max())
        assert np.all(r["rel_gap"][d_sig > 1e-6] <= H.GAP_MIN), (e, d_sig[ok].max())
        tot = occ[e].sum(axis=1)                                   # hopping conserves the total charge
        assert np.all(np.abs(tot - np.round(tot))[ok] < 1e-6), e
    env.close()


# ------------------------------------------------------------------ 4. nothing else moves
def test_points_leave_no_footprint_on_a_noisy_run(tmp_path):
    """All stochastic stages on, env_chunk = 2 (an observe of the 3 envs runs two chunks over the two launch lanes; the points
    run on lane 0's scratch), a rollout of 3 steps through a truncation with automatic resets."""
    import torch
    N, R, B, seed, max_steps = 4, 16, 3, 2718, 2
    L, C = layout(N), N - 1
    path = _cfg(tmp_path, max_steps=max_steps)
    plain, poked = [_vec(tmp_path, B, N, R, seed, config_path=path, noise=("sensor", "radial", "latch"), env_chunk=2)
                    for _ in range(2)]
    prng = np.random.default_rng(8)
    calls = [0]

    def poke():
        n = (2, 1, B)[calls[0] % 3]
        m = (800, 1, 130)[calls[0] % 3]                             # more than a slot (C P = 768), one point, a part of a slot
        calls[0] += 1
        ids = prng.integers(0, B, n)
        par = poked._params_host[ids]
        vg = par[:, None, L.vopt:L.vopt + N + 1] + prng.uniform(-4, 4, (n, m, N + 1))
        vb = par[:, None, L.vbopt:L.vbopt + C] + prng.uniform(-3, 3, (n, m, C))
        out = poked.eval_points(ids, vg, vb, gamma=None if calls[0] % 2 else 0.2)
        assert np.isfinite(out["signal"].cpu().numpy()).all() and np.isfinite(out["occupations"].cpu().numpy()).all()

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

    def a_probe(env):
        par = env._params_host
        st, _ = env.get_state()
        return env.probe(np.arange(B), st[:, L.s_gate_gt:L.s_gate_gt + N] + 1.5, par[:, L.vbopt:L.vbopt + C],
                         normalised=True)

    trace = [[], []]
    for k, env in enumerate((plain, poked)):
        trace[k].append(snapshot(env, env.reset(seed=seed)))
    before = a_probe(poked)
    poke()
    after = a_probe(poked)
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
    plain.close(); poked.close()


# ------------------------------------------------------------------ 5. refusals on the device
def test_validate_and_full_space_handles_refuse(tmp_path):
    from qadapt_hip import _lib
    N, R = 3, 8
    q = DM.load_yaml(None, "qarray_config.yaml")
    q["simulator"]["model"]["max_charge_carriers"] = 2
    qp = tmp_path / "qarray_m2.yaml"
    qp.write_text(yaml.safe_dump(q))
    for kw, word in ((dict(validate=True), "QD_FLAG_VALIDATE"),
                     (dict(num_charge_states="all", qarray_config_path=str(qp)), "full charge-state space")):
        env = _vec(tmp_path, 1, N, R, 77, **kw)
        env.reset(seed=77)
        raw0 = env.raw()[0].copy()
        with pytest.raises(_lib.QdError, match=word) as ei:
            env.eval_points([0], np.zeros((1, 4, N + 1)), np.zeros((1, 4, N - 1)))
        assert f"code {_lib.QD_ERR_STATE}" in str(ei.value)
        assert PH.same(env.raw()[0], raw0)
        env.close()
