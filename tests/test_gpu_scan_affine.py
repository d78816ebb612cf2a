"""Affine axis scans on the MI355X (run with -m gpu): qd_scan_affine on unit axes against qd_scan2d bit for bit, on
combination axes against qd_eval_points at the voltages of the host front end, the tile search on combination axes against
the per-pixel search, NumPy-built grids against the oracle, zero-vector axes, the absent footprint on a noisy auto-resetting
run, and the guards."""
import ctypes

import numpy as np
import pytest
import yaml

import affine_helpers as AH
import helpers as H
import points_helpers as PH
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


def _dense_pair(N, rng):
    """two dense directions: normal coefficients, the sensor component x0.1 and the barrier components x0.5"""
    d = rng.normal(size=(2, 2 * N))
    d[:, N] *= 0.1
    d[:, N + 1:] *= 0.5
    return d


# ------------------------------------------------------------------ 1. unit axes = scan2d
# (N, K, R): from 4 dots on a default handle runs the tile search at R >= 32, R = 36 cuts the last tiles; 2 and 3 dots run the
# per-pixel search
@pytest.mark.parametrize("N,K,R", [(4, 32, 32), (8, 16, 36), (2, 32, 8), (3, 32, 8)])
def test_unit_axes_equal_scan2d(tmp_path, N, K, R):
    """Default handle, one env near and one far from the ground truth; dx = e_ax, dy = e_ay with 0 at those two controls of
    the base point, gamma passed explicitly: raw, percentiles, float32 image and occupations have the bits of scan2d(ax, ay)
    -- plunger pairs, plunger against barrier, sensor gate against plunger, in both frames; and with sensor noise and
    latching under the same serial and stream base."""
    B, L = 2, layout(N)
    env = _vec(tmp_path, B, N, R, 7100 + N + K, num_charge_states=K)
    st = _placed(env, N, 7100 + N + K, ("near", "far"))
    gv, bv, sv = _volts(N, st)
    pairs = [(0, 1), (N - 1, 0), (0, N + 1), (N, 1)]
    ids = np.repeat(np.arange(B), len(pairs))
    ax = np.tile([p[0] for p in pairs], B); ay = np.tile([p[1] for p in pairs], B)
    nq = len(ids)
    gamma = 0.8 * env._params_host[ids, L.scal + 1]
    for frame in ("virtual", "physical"):
        W0 = np.zeros((nq, 2 * N))
        for q, e in enumerate(ids):
            phys = _physical_point(N, st[e], env._params_host[e])
            W0[q] = np.concatenate([phys if frame == "physical" else np.concatenate([gv[e], [sv[e]]]), bv[e]])
        ctr = W0.copy()
        rows = np.arange(nq)
        W0[rows, ax] = 0.0; W0[rows, ay] = 0.0
        xr = np.stack([ctr[rows, ax] - 1.0, ctr[rows, ax] + 2.0], 1)
        yr = np.stack([ctr[rows, ay] + 1.5, ctr[rows, ay] - 1.5], 1)                 # y sweeps downwards
        dx = np.stack([AH.unit(N, a) for a in ax]); dy = np.stack([AH.unit(N, a) for a in ay])
        for kw in (dict(), dict(noise=("sensor", "latch"), serial=(1 << 63) | 91, stream_base=4321)):
            kw = dict(kw, frame=frame, gamma=gamma, normalised=True, occupations=True, sensor_voltage=W0[:, N])
            ref = env.scan2d(ids, ax, ay, xr, yr, W0[:, :N], W0[:, N + 1:], **kw)
            got = env.scan_affine(ids, dx, dy, xr, yr, W0[:, :N], W0[:, N + 1:], **kw)
            rraw = ref["raw"].cpu().numpy()
            assert np.isfinite(rraw).all() and all(np.ptp(r) > 0 for r in rraw)
            for key in ("raw", "plohi", "image", "occupations"):
                a, b = got[key].cpu().numpy(), ref[key].cpu().numpy()
                assert PH.same(a, b), (frame, "noise" in kw, key, int((PH.bits(a) != PH.bits(b)).sum()))
        clean = env.scan_affine(ids, dx, dy, xr, yr, W0[:, :N], W0[:, N + 1:], frame=frame, gamma=gamma, sensor_voltage=W0[:, N])
        assert not PH.same(clean["raw"], got["raw"])                               # the noise really ran
    env.close()


# ------------------------------------------------------------------ 2. combination axes = points (per-pixel search)
def _combination_queries(N, st, par, seed):
    """(x, y, x_range, y_range, frame, base W0) per query: e x U, e x barrier, dense random directions in the virtual and in the
    physical frame.  The base point is the env's own voltages (its physical working point in the physical frame)."""
    L = layout(N)
    gv = st[L.s_gate_v:L.s_gate_v + N]; bvv = st[L.s_barrier_v:L.s_barrier_v + N - 1]; sv = st[L.s_sensor_gt]
    virt = np.concatenate([gv, [sv], bvv])
    phys = np.concatenate([_physical_point(N, st, par), bvv])
    rng = np.random.default_rng(seed)
    dv, dp = _dense_pair(N, rng), _dense_pair(N, rng)
    return [(f"e1_{N}", f"U1_{N}", (-1.5, 1.5), (-1.0, 2.0), "virtual", virt),
            ("e2_1", "B1", (2.0, -1.0), (-1.5, 1.5), "virtual", virt),
            (dv[0], dv[1], (-1.2, 1.2), (-0.8, 1.6), "virtual", virt),
            (dp[0], dp[1], (-1.2, 1.2), (1.6, -0.8), "physical", phys),
            ("e1_2", {"P1": 0.5, "B1": -1.0}, (-1.0, 2.0), (-1.0, 1.0), "physical", phys)]


_COMB = {}


def _combination_case(tmp_path, N, K, R, pixel_search=True, steep=False):
    """One env "near", one "mid"; the queries of _combination_queries on each (plus, with `steep`, an e axis over +-40 V).
    Returns per query the scan's raw and occupations and the host front end's v_ext; on a pixel_search handle eval_points
    there too."""
    from qadapt_hip.vec_env import scan_axis_vector
    key = (N, K, R, pixel_search, steep)
    if key in _COMB:
        return _COMB[key]
    B, G = 2, N + 1
    seed = 7300 + 10 * N + K
    env = _vec(tmp_path, B, N, R, seed, pixel_search=pixel_search, num_charge_states=K)
    st = _placed(env, N, seed, ("near", "mid"))
    res = []
    for e in range(B):
        par = env._params_host[e]
        qs = _combination_queries(N, st[e], par, seed + 1 + e)
        if steep:
            qs.append((f"e1_{N}", f"U1_{N}", (-40.0, 40.0), (-1.0, 2.0), "virtual", qs[0][5]))
        for x, y, xr, yr, frame, W0 in qs:
            out = env.scan_affine([e], x, y, xr, yr, W0[None, :N], W0[None, G:], sensor_voltage=W0[N], frame=frame,
                                  occupations=True)
            qst = SH.query_state(N, st[e], W0[:N], W0[G:], float(W0[N]))
            v_ext, _, _ = AH.affine_voltages(N, par, qst, scan_axis_vector(x, N, frame), scan_axis_vector(y, N, frame),
                                             list(xr) + list(yr), R, AH.PHYSICAL if frame == "physical" else AH.VIRTUAL)
            res.append(dict(e=e, x=x if isinstance(x, str) else "dense", y=y if isinstance(y, str) else "dense", xr=xr, frame=frame,
                            v_ext=v_ext, raw=out["raw"].cpu().numpy()[0], occ=out["occupations"].cpu().numpy()[0]))
    if pixel_search and not steep:
        for r in res:
            pts = env.eval_points([r["e"]], r["v_ext"][None, :, :G], r["v_ext"][None, :, G:])
            r["sig_pts"] = pts["signal"].cpu().numpy()[0]; r["occ_pts"] = pts["occupations"].cpu().numpy()[0]
    env.close()
    _COMB[key] = res
    return res


@pytest.mark.parametrize("N,K,R", [(4, 32, 12), (8, 32, 8), (2, 32, 8), (8, 20, 8)])
def test_combination_axes_equal_points(tmp_path, N, K, R):
    """pixel_search handle, envs "near" and "mid": the raw signal of e x U, e x barrier, a mixed dict axis and dense random
    directions has the bits of eval_points(signal) at the v_ext of the host front end (tests/hosttest_affine); the occupations
    have the bits of eval_points(occupations) where K is not 8, 16 or 32 (there the points solve the occupations from the
    reference order and the scan from the search order: rtol 1e-9, atol 1e-12, the rule of test_general_axes_equal_points)."""
    res = _combination_case(tmp_path, N, K, R)
    assert {r["frame"] for r in res} == {"virtual", "physical"} and len(res) == 10
    for r in res:
        tag = (r["e"], r["x"], r["y"], r["frame"])
        assert np.isfinite(r["raw"]).all() and np.ptp(r["raw"]) > 0, tag
        d = float(np.abs(r["raw"].reshape(-1) - r["sig_pts"]).max())
        do = float(np.abs(r["occ"].reshape(-1, N) - r["occ_pts"]).max())
        print(f"[affine vs points] N={N} K={K} R={R} {tag}: raw diff {d:.3e}, occupation diff {do:.3e}")
        assert PH.same(r["raw"].reshape(-1), r["sig_pts"]), (tag, d)
        if K in (8, 16, 32):
            assert np.allclose(r["occ"].reshape(-1, N), r["occ_pts"], rtol=1e-9, atol=1e-12), (tag, do)
        else:
            assert PH.same(r["occ"].reshape(-1, N), r["occ_pts"]), (tag, do)


# ------------------------------------------------------------------ 3. the tile search on combination axes
@pytest.mark.parametrize("N,K,R", [(4, 32, 32), (8, 32, 32), (8, 16, 36)])
def test_tile_search_on_combination_axes_equals_pixel_search(tmp_path, N, K, R):
    """The same queries on a default handle (tile search + exact redo pass with the affine front end) and on a pixel_search
    handle, "near" and "mid": rtol 1e-9, atol 1e-12 on raw (the numbers and regime of
    test_tile_search_on_general_axes_equals_pixel_search).  R = 36: the last tiles are cut.  One steep query per env, an e axis
    over +-40 V: the floors of a tile span more than its 8 digits, so whole tiles go to the redo pass; same bound."""
    tile = _combination_case(tmp_path, N, K, R, pixel_search=False, steep=True)
    pix = _combination_case(tmp_path, N, K, R, pixel_search=True, steep=True)
    assert len(tile) == len(pix) == 12 and sum(1 for a in tile if a["xr"] == (-40.0, 40.0)) == 2
    for a, b in zip(tile, pix):
        tag = (a["e"], a["x"], a["y"], a["frame"], a["xr"])
        assert PH.same(a["v_ext"], b["v_ext"])
        assert np.isfinite(b["raw"]).all() and np.ptp(b["raw"]) > 0, tag
        d = np.abs(a["raw"] - b["raw"])
        print(f"[affine tile vs pixel] N={N} K={K} R={R} {tag}: worst {d.max():.3e}, pixels with other bits {int((PH.bits(a['raw']) != PH.bits(b['raw'])).sum())}")
        assert np.allclose(a["raw"], b["raw"], rtol=1e-9, atol=1e-12), (tag, float(d.max()))


# ------------------------------------------------------------------ 4. the oracle on NumPy-built grids
ORACLE_SEEDS = {2: 50, 4: 50, 6: 51}


def _oracle_queries(N):
    from qadapt_hip.vec_env import scan_axis_vector as vec
    q = [(vec("e1_2", N), vec("U1_2", N), (-1.5, 1.5, -1.0, 2.0), "virtual"),
         (vec(f"e1_{N}", N), vec("B1", N), (-1.0, 2.0, 1.5, -1.5), "virtual")]
    if N > 2:
        q.append((vec("U2_3", N), vec(f"e{N}_1", N), (2.0, -1.0, -1.5, 1.5), "virtual"))
    d = _dense_pair(N, np.random.default_rng(1000 + N))
    q.append((d[0], d[1], (-1.2, 1.2, -0.8, 1.6), "physical"))
    return q


_ORACLE = {}


def _oracle_case(N):
    """The device of seed ORACLE_SEEDS[N] "near" its ground truth (rng of that seed, vgm_noise = 0); per query an 8 x 8 grid
    built in NumPy (affine_helpers.numpy_grid) around the env's own voltages (its physical working point in the physical
    frame) and the oracle's occupations, signal and relative gap there.  CPU only, computed once."""
    if N not in _ORACLE:
        R, L, G = 8, layout(N), N + 1
        seed = ORACLE_SEEDS[N]
        eb = H.sample_blocks(N, [seed])
        rng = np.random.default_rng(seed)
        par, st = eb.params[0], H.place(N, eb.state[0], "near", rng, vgm_noise=0.0)
        dev = H.dev_view(N, par)
        bv = st[L.s_barrier_v:L.s_barrier_v + N - 1]
        virt = AH.base_point(N, st)
        phys = np.concatenate([_physical_point(N, st, par), bv])
        cases = []
        for dx, dy, rg, frame in _oracle_queries(N):
            base = phys if frame == "physical" else virt
            qst = SH.query_state(N, st, base[:N], bv, base[N])
            grid = AH.numpy_grid(N, qst, par[L.origin:L.origin + G], dx, dy, rg, R,
                                 AH.PHYSICAL if frame == "physical" else AH.VIRTUAL).reshape(R * R, 2 * N)
            vg, vb = grid[:, :G], grid[:, G:]
            n, states, F, tc = O.ground_state_open(dev, vg, vb, return_states=True)
            sig, _ = O.charge_sensor_open(dev, vg, vb, n_open=n)
            Hm = F[:, :, None] * np.eye(states.shape[1]) + O.tunnel_hamiltonian(tc, states)
            w = np.linalg.eigvalsh(Hm)
            hn = np.abs(Hm).sum(axis=2).max(axis=1)
            cases.append(dict(dx=dx, dy=dy, rg=np.array(rg), frame=frame, gv=base[:N], sv=base[N], bv=bv, occ=n, sig=sig[:, 0],
                              rel_gap=(w[:, 1] - w[:, 0]) / hn))
        _ORACLE[N] = (eb.params[:1], st[None], cases)
    return _ORACLE[N]


@pytest.mark.parametrize("N", [2, 4, 6])
def test_affine_scans_against_the_oracle(tmp_path, N):
    """O.ground_state_open / O.charge_sensor_open at NumPy-built 8 x 8 grids: e1_2 x U1_2, e1_N x B1 (y downwards), for N > 2
    U2_3 x eN_1 (x downwards), and a dense physical pair.  The per-pixel rule of test_scans_against_the_oracle: where the
    oracle's relative gap is above GAP_MIN, occupations and signal agree within 1e-6; at most 1 % of an image (0 of 64
    pixels) may be excused.  Checked on the CPU beforehand: the oracle alone leaves 0 of 64 pixels unresolved in each of the
    11 images (smallest relative gap: N = 2 8.9e-05, N = 4 2.0e-04, N = 6 6.5e-05); the total charge varies by up to 10
    carriers across an image (N = 4, e1_2 x U1_2: 10 to 20), so the grids cross many transitions."""
    params, state, cases = _oracle_case(N)
    assert len(cases) == (3 if N == 2 else 4)
    for c in cases:
        unres = int((c["rel_gap"] <= H.GAP_MIN).sum())
        assert unres <= 0.01 * 64, f"the oracle alone leaves {unres} of 64 pixels unresolved"
    env = _vec(tmp_path, 1, N, 8, ORACLE_SEEDS[N])
    _load(env, params, state)
    for k, c in enumerate(cases):
        out = env.scan_affine([0], c["dx"], c["dy"], c["rg"][:2], c["rg"][2:], c["gv"][None], c["bv"][None], sensor_voltage=c["sv"],
                              frame=c["frame"], occupations=True)
        occ = out["occupations"].cpu().numpy().reshape(64, N); sig = out["raw"].cpu().numpy().reshape(64)
        ok = c["rel_gap"] > H.GAP_MIN
        d_occ = np.abs(occ - c["occ"]).max(axis=1)
        d_sig = np.abs(sig - c["sig"]) / np.maximum(np.abs(c["sig"]), 1e-3)
        print(f"[affine vs oracle] N={N} query {k} {c['frame']}: worst occupation {d_occ[ok].max():.3e}, "
              f"worst signal {d_sig[ok].max():.3e}, unresolved {int((~ok).sum())}, total charge {c['occ'].sum(axis=1).min():.2f}.."
              f"{c['occ'].sum(axis=1).max():.2f}")
        assert np.all(c["rel_gap"][d_occ > 1e-6] <= H.GAP_MIN), d_occ[ok].max()
        assert np.all(c["rel_gap"][d_sig > 1e-6] <= H.GAP_MIN), d_sig[ok].max()
        assert int((~ok).sum()) <= 0.01 * 64
    env.close()


# ------------------------------------------------------------------ 5. a zero-vector axis
@pytest.mark.parametrize("N,R,K", [(4, 32, 32), (2, 8, 32)])
def test_zero_vector_axis_repeats_a_sweep(tmp_path, N, R, K):
    """dy = 0: every row has the bits of row 0, in raw and in occupations; dx = 0: every column those of column 0.  A default
    handle at (4 dots, R = 32) runs the tile search, whose plane then has slope 0 along that axis; 2 dots run the per-pixel
    search."""
    from qadapt_hip.vec_env import scan_axis_vector as vec
    env = _vec(tmp_path, 1, N, R, 7600 + N, num_charge_states=K)
    st = _placed(env, N, 7600 + N, ("near",))
    gv, bv, sv = _volts(N, st)
    zero = np.zeros(2 * N)
    for axis in ("e1_2", f"U1_{N}", {"vP1": 1.0, "B1": -0.5}):
        d = vec(axis, N)
        out = env.scan_affine([0, 0], np.stack([d, zero]), np.stack([zero, d]), [[-1.5, 1.5], [0.3, 0.9]], [[0.2, -0.7], [2.0, -1.0]],
                              gv[[0, 0]], bv[[0, 0]], sensor_voltage=sv[[0, 0]], occupations=True)
        raw, occ = out["raw"].cpu().numpy(), out["occupations"].cpu().numpy()
        assert np.ptp(raw[0]) > 0 and np.ptp(raw[1]) > 0, axis
        assert PH.same(raw[0], np.broadcast_to(raw[0][:1, :], (R, R))) and PH.same(occ[0], np.broadcast_to(occ[0][:1], (R, R, N)))
        assert PH.same(raw[1], np.broadcast_to(raw[1][:, :1], (R, R))) and PH.same(occ[1], np.broadcast_to(occ[1][:, :1], (R, R, N)))
    both = env.scan_affine([0], zero, zero, (0, 1), (0, 1), gv, bv, sensor_voltage=sv)["raw"].cpu().numpy()
    assert np.isfinite(both).all() and PH.same(both, np.broadcast_to(both[:, :1, :1], both.shape))
    env.close()


# ------------------------------------------------------------------ 6. nothing else moves
def test_affine_scans_leave_no_footprint_on_a_noisy_run(tmp_path):
    """Two handles with all stochastic stages on, env_chunk = 2, a rollout of 3 steps through a truncation with automatic
    reloads; one of them calls scan_affine between all calls: observations, rewards, state blocks, raw signal, percentiles,
    parameter blocks and the observation serial stay byte-identical.  A probe, a scan2d and an eval_points call before and after
    are byte-equal."""
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
        n = (5, 1, 3)[k]
        ids = prng.integers(0, B, n)
        par = poked._params_host[ids]
        st, _ = poked.get_state()
        gv = st[ids, L.s_gate_gt:L.s_gate_gt + N] + prng.uniform(-2, 2, (n, N))
        bv = par[:, L.vbopt:L.vbopt + C] + prng.uniform(-2, 2, (n, C))
        x, y = (("e1_2", "U1_2"), (_dense_pair(N, prng)[0], "B2"), ({"vP3": 1.0, "B2": -0.4}, "e4_1"))[k]
        out = poked.scan_affine(ids, x, y, (-1.5, 1.5), (2.0, -1.0), gv, bv,
                                noise=("sensor", "latch") if k != 1 else None, occupations=k == 2, normalised=True,
                                vgm=None if k else np.broadcast_to(-np.eye(G), (n, G, G)), gamma=None if k != 2 else 0.2)
        assert np.isfinite(out["raw"].cpu().numpy()).all() and np.isfinite(out["image"].cpu().numpy()).all()

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
        out = dict(env.probe(np.arange(B), gt + 1.5, par[:, L.vbopt:L.vbopt + C], normalised=True))
        out["scan2d"] = env.scan2d(np.arange(B), 0, N + 1, (-1, 2), (1, -1), gt, par[:, L.vbopt:L.vbopt + C])["raw"]
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
    plain.close(); poked.close()


# ------------------------------------------------------------------ 7. guards
def _raw_call(env, ids, dirs, rg, gv, bv, nq, raw, image=None, plohi=None, occ=None, flags=0):
    import torch
    from qadapt_hip import _lib
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dt)).cuda()      # noqa: E731
    keep = [t(ids, np.int32), t(dirs, np.float64), t(rg, np.float64), t(gv, np.float64), t(bv, np.float64)]
    o = _lib.QdScanAffineOpts(struct_size=ctypes.sizeof(_lib.QdScanAffineOpts), noise_flags=flags, serial=(1 << 63) | 5,
                              occ_dst=None if occ is None else occ.data_ptr())
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())          # noqa: E731
    rc = env._lib.qd_scan_affine(env._h, p(keep[0]), nq, p(keep[1]), p(keep[2]), p(keep[3]), p(keep[4]), None, p(raw), p(image),
                                 p(plohi), ctypes.byref(o), env._stream())
    torch.cuda.synchronize()
    return rc


def test_guards_inert_queries_and_chunks(tmp_path):
    """7 queries on 3 envs through the C entry point with sensor noise and latching, guard rows on both sides of every
    destination: the same bits with env_chunk = 2 (four launch chunks) and env_chunk = 3; then env ids outside [0, B) leave
    their pre-filled slots untouched while the live queries beside them keep their bits."""
    import torch
    from qadapt_hip.vec_env import scan_axis_vector as vec
    N, R, B, seed = 4, 8, 3, 7500
    P = R * R
    ids = np.array([0, 1, 2, 1, 0, 2, 2], np.int32)
    nq, g0, g1, guard = 7, 2, 3, -12345.678
    full = lambda *s: torch.full(s, guard, dtype=torch.float64, device="cuda")     # noqa: E731
    rng = np.random.default_rng(seed)
    dense = [_dense_pair(N, rng) for _ in range(2)]
    dirs = np.stack([np.stack([vec("e1_2", N), vec("U1_2", N)]), np.stack([vec("e1_4", N), vec("B1", N)]), dense[0],
                     np.stack([vec("U2_3", N), vec("e4_1", N)]), np.stack([vec("vP1", N), np.zeros(2 * N)]), dense[1],
                     np.stack([vec({"vP2": 1.0, "B2": -0.5}, N), vec("S", N)])])
    rg = np.tile([-1.5, 1.5, 2.0, -1.0], (nq, 1)) + rng.uniform(-0.3, 0.3, (nq, 4))
    flags = 1 | 4
    results = {}
    for chunk in (2, 3):
        env = _vec(tmp_path, B, N, R, seed, env_chunk=chunk)
        assert env.chunk_envs() == chunk
        st = _placed(env, N, seed, ("near", "mid", "near"))
        gv, bv, _ = _volts(N, st)
        raw, plohi, occ = full(g0 + nq + g1, P), full(g0 + nq + g1, 2), full(g0 + nq + g1, P, N)
        img = torch.full((g0 + nq + g1, P), -7.0, dtype=torch.float32, device="cuda")
        assert _raw_call(env, ids, dirs, rg, gv[ids], bv[ids], nq, raw[g0:], img[g0:], plohi[g0:], occ[g0:], flags) == 0
        out = [a.cpu().numpy() for a in (raw, plohi, occ, img)]
        for a, gval in zip(out, (guard, guard, guard, -7.0)):
            assert np.all(a[:g0] == gval) and np.all(a[g0 + nq:] == gval)
            assert np.isfinite(a[g0:g0 + nq]).all() and not np.any(a[g0:g0 + nq] == gval)
        results[chunk] = out
        if chunk == 2:
            # inert queries: their slots keep the pre-fill, the live ones keep their bits (same query index = same streams)
            bad_ids = np.array([0, B, -1, 1, B + 5, 2, -7], np.int32)
            live = (bad_ids >= 0) & (bad_ids < B)
            r2, p2, o2 = full(nq, P), full(nq, 2), full(nq, P, N)
            i2 = torch.full((nq, P), -7.0, dtype=torch.float32, device="cuda")
            assert _raw_call(env, bad_ids, dirs, rg, gv[ids], bv[ids], nq, r2, i2, p2, o2, flags) == 0
            for a, b, gval in zip((r2, p2, o2, i2), out, (guard, guard, guard, -7.0)):
                a = a.cpu().numpy()
                assert np.all(a[~live] == gval)
                assert PH.same(a[live], b[g0:g0 + nq][live])
        env.close()
    for a, b in zip(results[2], results[3]):
        assert PH.same(a, b)


def test_refusals(tmp_path):
    import torch
    from qadapt_hip import _lib
    N, R = 3, 8
    q = DM.load_yaml(None, "qarray_config.yaml")
    q["simulator"]["model"]["max_charge_carriers"] = 2
    qp = tmp_path / "qarray_m2.yaml"
    qp.write_text(yaml.safe_dump(q))
    gv, bv = np.zeros((1, N)), np.zeros((1, N - 1))
    for kw, word in ((dict(validate=True), "QD_FLAG_VALIDATE"),
                     (dict(num_charge_states="all", qarray_config_path=str(qp)), "full charge-state space")):
        env = _vec(tmp_path, 1, N, R, 77, **kw)
        env.reset(seed=77)
        raw0 = env.raw()[0].copy()
        with pytest.raises(_lib.QdError, match=word) as ei:
            env.scan_affine([0], "e1_2", "U1_2", (-1, 1), (-1, 1), gv, bv)
        assert f"code {_lib.QD_ERR_STATE}" in str(ei.value)
        assert PH.same(env.raw()[0], raw0)
        env.close()
    env = _vec(tmp_path, 1, N, R, 78)
    env.reset(seed=78)
    with pytest.raises(ValueError, match="radial"):
        env.scan_affine([0], "e1_2", "U1_2", (-1, 1), (-1, 1), gv, bv, noise=("sensor", "radial"))
    raw = torch.full((1, R * R), -5.0, dtype=torch.float64, device="cuda")
    dirs = np.stack([AH.unit(N, 0), AH.unit(N, 1)])[None]
    rc = _raw_call(env, [0], dirs, [[-1, 1, -1, 1]], gv, bv, 1, raw, flags=_lib.QD_NOISE_RADIAL)
    assert rc == _lib.QD_ERR_ARG and b"radial" in env._lib.qd_last_error(env._h)
    assert np.all(raw.cpu().numpy() == -5.0)
    with pytest.raises(ValueError):
        env.scan_affine([0], "e1_1", "U1_2", (-1, 1), (-1, 1), gv, bv)
    env.close()
