"""Axis scans on the MI355X (run with -m gpu): qd_scan2d on adjacent virtual plungers against qd_probe / qd_probe_ex bit for
bit, on general axes against qd_eval_points at the voltages of the host front end, the tile search on general axes against
the per-pixel search, NumPy-built grids against the oracle, the absent footprint on a noisy auto-resetting run, degenerate
axes, and the refusals."""
import ctypes

import numpy as np
import pytest
import yaml

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


# ------------------------------------------------------------------ 1. adjacent virtual plungers = a probe
# (N, K, R, vary_peak_width): from 4 dots on a default handle runs the tile search at R >= 32; R = 36 cuts the last tiles
ADJ_CASES = [(2, 32, 8, False), (2, 32, 12, False), (4, 32, 32, False), (8, 32, 32, False), (8, 16, 36, False),
             (4, 32, 32, True), (4, 32, 8, False)]


@pytest.mark.parametrize("N,K,R,vary", ADJ_CASES)
def test_adjacent_scan_equals_probe(tmp_path, N, K, R, vary):
    """Default handle, one env near and one far from the ground truth, every channel c as the scan (c, c+1) over
    fl(v + (-w)), fl(v + w): raw has the bits of the probe's channel c -- at the env's own window and at one unlike it, and on
    a vary_peak_width handle (the rule of qd_peak_width on the two plungers).  For C = 1 image and percentiles too.  With
    sensor noise and latching, same serial and stream base, channel 0 (the Philox channel word of a scan) has the probe's
    raw and occupation bits."""
    B, C, L = 2, N - 1, layout(N)
    env = _vec(tmp_path, B, N, R, 6100 + N + K, num_charge_states=K, vary_peak_width=vary, peak_width_alpha=0.004)
    st = _placed(env, N, 6100 + N + K, ("near", "far"))
    gv, bv, sv = _volts(N, st)
    assert bool(env._params_host[0, L.scal + 3] >= 0.0) == vary
    ids = np.repeat(np.arange(B), C)                                    # query q = e C + c
    chan = np.tile(np.arange(C), B)
    for w in (None, 0.41 * float(env._params_host[0, L.scal + 2])):
        wins = env._params_host[:, L.scal + 2] if w is None else np.full(B, w)
        rg = np.stack([SH.adjacent_ranges(gv[e], c, wins[e]) for e, c in zip(ids, chan)])
        probe = env.probe(np.arange(B), gv, bv, sensor_voltage=sv, window=w, normalised=True)
        scan = env.scan2d(ids, chan, chan + 1, rg[:, :2], rg[:, 2:], gv[ids], bv[ids], sensor_voltage=sv[ids], normalised=True)
        praw = probe["raw"].cpu().numpy()
        assert np.isfinite(praw).all() and np.ptp(praw) > 0
        assert PH.same(scan["raw"].cpu().numpy().reshape(B, C, R, R), praw), (w, int((PH.bits(scan["raw"].cpu().numpy().reshape(B, C, R, R)) != PH.bits(praw)).sum()))
        if C == 1:
            assert PH.same(scan["image"].cpu().numpy(), probe["image"].cpu().numpy()[..., 0])
            assert PH.same(scan["plohi"], probe["plohi"])
    # the stochastic stages: channel 0 of each env, query q = env q
    kw = dict(noise=("sensor", "latch"), serial=(1 << 63) | 77, stream_base=1234)
    probe = env.probe(np.arange(B), gv, bv, sensor_voltage=sv, occupations=True, **kw)
    rg = np.stack([SH.adjacent_ranges(gv[e], 0, env._params_host[e, L.scal + 2]) for e in range(B)])
    scan = env.scan2d(np.arange(B), 0, 1, rg[:, :2], rg[:, 2:], gv, bv, sensor_voltage=sv, occupations=True, **kw)
    clean = env.scan2d(np.arange(B), 0, 1, rg[:, :2], rg[:, 2:], gv, bv, sensor_voltage=sv)
    assert not PH.same(scan["raw"], clean["raw"])                        # the noise really ran
    assert PH.same(scan["raw"], probe["raw"][:, 0])
    assert PH.same(scan["occupations"], probe["occupations"][:, 0])
    env.close()


# ------------------------------------------------------------------ 2. general axes = points (per-pixel search)
def _general_queries(N, st, par, rng):
    """(ax, ay, ranges, frame, vgm) per query: plunger vs barrier, barrier vs barrier (N >= 4), non-adjacent plungers, sensor
    gate vs plunger, a physical-frame scan, a vgm override; asymmetric and reversed ranges throughout"""
    L = layout(N); G = N + 1
    gv = st[L.s_gate_v:L.s_gate_v + N]; bvv = st[L.s_barrier_v:L.s_barrier_v + N - 1]; sv = st[L.s_sensor_gt]

    def rng_of(i):
        c = gv[i] if i < N else (sv if i == N else bvv[i - N - 1])
        return [c - rng.uniform(0.5, 2.0), c + rng.uniform(2.0, 4.0)]

    q = [(0, N + 1, "virtual", None), (N - 1, 0, "virtual", None), (N, 1, "virtual", None), (1, N, "virtual", None),
         (0, 2 * N - 1, "physical", None), (0, 1, "virtual", "override")]
    if N >= 4:
        q += [(N + 1, 2 * N - 1, "virtual", None), (2, 0, "virtual", None), (N + 2, 1, "physical", None)]
    out = []
    for k, (ax, ay, frame, vg) in enumerate(q):
        rx, ry = rng_of(ax), rng_of(ay)
        if k % 3 == 1:
            rx = rx[::-1]                                               # a reversed range
        if frame == "physical":
            # physical plunger voltages live around VGM v + origin, not around v
            vgm = st[L.s_vgm:L.s_vgm + G * G].reshape(G, G)
            phys = vgm @ np.concatenate([gv, [sv]]) + par[L.origin:L.origin + G]
            if ax < G:
                rx = [phys[ax] - 1.0, phys[ax] + 3.0]
            if ay < G:
                ry = [phys[ay] + 2.0, phys[ay] - 1.5]
        vm = None
        if vg == "override":
            vm = st[L.s_vgm:L.s_vgm + G * G].reshape(G, G) + rng.normal(0, 0.03, (G, G))
        out.append((ax, ay, np.array(rx + ry), frame, vm))
    return out


GEN_CASES = [(2, 32, 8), (4, 32, 12), (8, 32, 8), (4, 20, 8), (8, 20, 12), (8, 16, 8)]
_GEN = {}


def _general_case(tmp_path, N, K, R, pixel_search=True):
    """One env "near", one "mid"; the queries of _general_queries on each, one call per frame / vgm kind (frame and vgm are
    per call).  Returns per query the scan's raw and occupations, the host front end's v_ext and eval_points there."""
    key = (N, K, R, pixel_search)
    if key in _GEN:
        return _GEN[key]
    B, L, G = 2, layout(N), N + 1
    seed = 6300 + 10 * N + K
    env = _vec(tmp_path, B, N, R, seed, pixel_search=pixel_search, num_charge_states=K)
    st = _placed(env, N, seed, ("near", "mid"))
    rng = np.random.default_rng(seed + 1)
    res = []
    for e in range(B):
        par = env._params_host[e]
        gv, bv, sv = _volts(N, st[e:e + 1])
        for ax, ay, rg, frame, vm in _general_queries(N, st[e], par, rng):
            if frame == "physical":
                # the query's gate voltages ARE physical here: start from the env's physical working point
                vgm = st[e, L.s_vgm:L.s_vgm + G * G].reshape(G, G)
                phys = vgm @ np.concatenate([gv[0], sv]) + par[L.origin:L.origin + G]
                qg, qs = phys[None, :N], phys[N:]
            else:
                qg, qs = gv, sv
            out = env.scan2d([e], ax, ay, rg[:2], rg[2:], qg, bv, sensor_voltage=qs, frame=frame,
                             vgm=None if vm is None else vm[None], occupations=True, normalised=True)
            qst = SH.query_state(N, st[e], qg[0], bv[0], float(qs[0]), vm)
            v_ext, _, _ = SH.scan_voltages(N, par, qst, ax, ay, rg, R, SH.PHYSICAL if frame == "physical" else SH.VIRTUAL)
            res.append(dict(e=e, ax=ax, ay=ay, frame=frame, vgm=vm is not None, v_ext=v_ext,
                            raw=out["raw"].cpu().numpy()[0], occ=out["occupations"].cpu().numpy()[0],
                            image=out["image"].cpu().numpy()[0], plohi=out["plohi"].cpu().numpy()[0]))
    if pixel_search:
        for r in res:
            pts = env.eval_points([r["e"]], r["v_ext"][None, :, :G], r["v_ext"][None, :, G:])
            r["sig_pts"] = pts["signal"].cpu().numpy()[0]; r["occ_pts"] = pts["occupations"].cpu().numpy()[0]
    env.close()
    _GEN[key] = res
    return res


@pytest.mark.parametrize("N,K,R", GEN_CASES)
def test_general_axes_equal_points(tmp_path, N, K, R):
    """pixel_search handle: raw has the bits of eval_points(signal) at the v_ext of the host front end; the occupations
    have the bits of eval_points(occupations) where K is not 8, 16 or 32 (there the points solve the occupations from the
    reference order and the scan from the search order: rtol 1e-9, atol 1e-12, the numbers of
    test_product_mode_tile_search_equals_validate_mode).  The image is the raw signal under its own percentiles."""
    res = _general_case(tmp_path, N, K, R)
    kinds = {(r["ax"] < N, r["ay"] < N, r["frame"], r["vgm"]) for r in res}
    assert len(kinds) >= 5
    for r in res:
        tag = (r["e"], r["ax"], r["ay"], r["frame"], r["vgm"])
        assert np.isfinite(r["raw"]).all() and np.ptp(r["raw"]) > 0, tag
        d = float(np.abs(r["raw"].reshape(-1) - r["sig_pts"]).max())
        do = float(np.abs(r["occ"].reshape(-1, N) - r["occ_pts"]).max())
        print(f"[scan vs points] N={N} K={K} R={R} {tag}: raw diff {d:.3e}, occupation diff {do:.3e}")
        assert PH.same(r["raw"].reshape(-1), r["sig_pts"]), (tag, d)
        if K in (8, 16, 32):
            assert np.allclose(r["occ"].reshape(-1, N), r["occ_pts"], rtol=1e-9, atol=1e-12), (tag, do)
        else:
            assert PH.same(r["occ"].reshape(-1, N), r["occ_pts"]), (tag, do)
        lo, hi = np.percentile(r["raw"], [0.5, 99.5])
        assert abs(r["plohi"][0] - lo) <= 1e-12 * abs(lo) + 1e-300 and abs(r["plohi"][1] - hi) <= 1e-12 * abs(hi) + 1e-300, tag
        want = np.clip((r["raw"] - r["plohi"][0]) / (r["plohi"][1] - r["plohi"][0]), 0, 1).astype(np.float32)
        assert np.array_equal(r["image"], want), tag


# ------------------------------------------------------------------ 3. the tile search on general axes
@pytest.mark.parametrize("N,K,R", [(4, 32, 32), (8, 32, 32), (8, 16, 36)])
def test_tile_search_on_general_axes_equals_pixel_search(tmp_path, N, K, R):
    """The same queries on a default handle (tile search + exact redo pass with the scan front end) and on a pixel_search
    handle, "near" and "mid": rtol 1e-9, atol 1e-12 on raw (test_product_mode_tile_search_equals_validate_mode's numbers and
    regime).  R = 36: the last tiles are cut."""
    tile = _general_case(tmp_path, N, K, R, pixel_search=False)
    pix = _general_case(tmp_path, N, K, R, pixel_search=True)
    assert len(tile) == len(pix)
    for a, b in zip(tile, pix):
        tag = (a["e"], a["ax"], a["ay"], a["frame"])
        d = np.abs(a["raw"] - b["raw"])
        print(f"[scan tile vs pixel] N={N} K={K} R={R} {tag}: worst {d.max():.3e}, pixels with other bits {int((PH.bits(a['raw']) != PH.bits(b['raw'])).sum())}")
        assert np.allclose(a["raw"], b["raw"], rtol=1e-9, atol=1e-12), (tag, float(d.max()))


# ------------------------------------------------------------------ 4. the oracle on NumPy-built grids
ORACLE_SEEDS = {2: 50, 4: 50, 6: 51}


def _oracle_queries(N):
    return [(0, N + 1, "virtual"), (N - 1, 0, "virtual"), (N, 0, "virtual"), (0, 2 * N - 1, "physical")]


_ORACLE = {}


def _oracle_case(N):
    """The device of seed ORACLE_SEEDS[N] "near" its ground truth (rng of that seed); per query an 8 x 8 grid built in NumPy
    (scan_helpers.numpy_grid) and the oracle's occupations, signal and relative gap there.  CPU only, computed once."""
    if N not in _ORACLE:
        R, L, G = 8, layout(N), N + 1
        seed = ORACLE_SEEDS[N]
        eb = H.sample_blocks(N, [seed])
        rng = np.random.default_rng(seed)
        par, st = eb.params[0], H.place(N, eb.state[0], "near", rng, vgm_noise=0.0)
        dev = H.dev_view(N, par)
        gv = st[L.s_gate_v:L.s_gate_v + N]; bv = st[L.s_barrier_v:L.s_barrier_v + N - 1]; sv = st[L.s_sensor_gt]
        vgm = st[L.s_vgm:L.s_vgm + G * G].reshape(G, G)
        phys = vgm @ np.concatenate([gv, [sv]]) + par[L.origin:L.origin + G]
        cases = []
        for ax, ay, frame in _oracle_queries(N):
            base = np.concatenate([phys if frame == "physical" else np.concatenate([gv, [sv]]), bv])
            rg = np.array([base[ax] - 1.0, base[ax] + 2.0, base[ay] + 1.5, base[ay] - 1.5])
            qst = SH.query_state(N, st, base[:N], bv, base[N])
            grid = SH.numpy_grid(N, qst, par[L.origin:L.origin + G], ax, ay, rg, R,
                                 SH.PHYSICAL if frame == "physical" else SH.VIRTUAL).reshape(R * R, 2 * N)
            vg, vb = grid[:, :G], grid[:, G:]
            n, states, F, tc = O.ground_state_open(dev, vg, vb, return_states=True)
            sig, _ = O.charge_sensor_open(dev, vg, vb, n_open=n)
            Hm = F[:, :, None] * np.eye(states.shape[1]) + O.tunnel_hamiltonian(tc, states)
            w = np.linalg.eigvalsh(Hm)
            hn = np.abs(Hm).sum(axis=2).max(axis=1)
            cases.append(dict(ax=ax, ay=ay, frame=frame, rg=rg, gv=base[:N], sv=base[N], bv=bv, occ=n, sig=sig[:, 0],
                              rel_gap=(w[:, 1] - w[:, 0]) / hn))
        _ORACLE[N] = (eb.params[:1], st[None], cases)
    return _ORACLE[N]


@pytest.mark.parametrize("N", [2, 4, 6])
def test_scans_against_the_oracle(tmp_path, N):
    """O.ground_state_open / O.charge_sensor_open at NumPy-built 8 x 8 grids: plunger vs barrier, a reversed non-adjacent
    plunger pair, sensor gate vs plunger, and a physical-frame plunger vs barrier scan.  The per-pixel rule of helpers: where
    the oracle's relative gap is above GAP_MIN, occupations and signal agree within 1e-6; at most 1 % of an image (0 of 64
    pixels) may be excused.  Seeds and ranges were chosen on the CPU beforehand: the oracle alone leaves 0 of 64 pixels
    unresolved in each of the 12 images (smallest relative gap: N = 2 6.2e-05, N = 4 3.2e-04, N = 6 1.1e-04)."""
    params, state, cases = _oracle_case(N)
    for c in cases:
        unres = int((c["rel_gap"] <= H.GAP_MIN).sum())
        assert unres <= 0.01 * 64, f"the oracle alone leaves {unres} of 64 pixels unresolved"
    env = _vec(tmp_path, 1, N, 8, ORACLE_SEEDS[N])
    _load(env, params, state)
    for c in cases:
        out = env.scan2d([0], c["ax"], c["ay"], c["rg"][:2], c["rg"][2:], c["gv"][None], c["bv"][None], sensor_voltage=c["sv"],
                         frame=c["frame"], occupations=True)
        occ = out["occupations"].cpu().numpy().reshape(64, N); sig = out["raw"].cpu().numpy().reshape(64)
        ok = c["rel_gap"] > H.GAP_MIN
        d_occ = np.abs(occ - c["occ"]).max(axis=1)
        d_sig = np.abs(sig - c["sig"]) / np.maximum(np.abs(c["sig"]), 1e-3)
        print(f"[scan vs oracle] N={N} ({c['ax']}, {c['ay']}) {c['frame']}: worst occupation {d_occ[ok].max():.3e}, "
              f"worst signal {d_sig[ok].max():.3e}, unresolved {int((~ok).sum())}")
        assert np.all(c["rel_gap"][d_occ > 1e-6] <= H.GAP_MIN), d_occ[ok].max()
        assert np.all(c["rel_gap"][d_sig > 1e-6] <= H.GAP_MIN), d_sig[ok].max()
        assert int((~ok).sum()) <= 0.01 * 64
    env.close()


# ------------------------------------------------------------------ 5. nothing else moves
def _raw_call(env, ids, axes, rg, gv, bv, nq, raw, image=None, plohi=None, occ=None, flags=0):
    import torch
    from qadapt_hip import _lib
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dt)).cuda()      # noqa: E731
    keep = [t(ids, np.int32), t(axes, np.int32), t(rg, np.float64), t(gv, np.float64), t(bv, np.float64)]
    o = _lib.QdScanOpts(struct_size=ctypes.sizeof(_lib.QdScanOpts), noise_flags=flags, serial=(1 << 63) | 5,
                        occ_dst=None if occ is None else occ.data_ptr())
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())          # noqa: E731
    rc = env._lib.qd_scan2d(env._h, p(keep[0]), nq, p(keep[1]), p(keep[2]), p(keep[3]), p(keep[4]), None, p(raw), p(image), p(plohi),
                            ctypes.byref(o), env._stream())
    torch.cuda.synchronize()
    return rc


def test_guards_inert_queries_and_chunks(tmp_path):
    """nq = 5 with env_chunk = 2 (three launch chunks) against every query alone, through the C entry point with guard rows
    on both sides of every destination; then a bad axis, ax == ay and env ids out of range leave their slots untouched."""
    import torch
    N, R, B, seed = 4, 8, 3, 6500
    L, C, P = layout(N), N - 1, 64
    env = _vec(tmp_path, B, N, R, seed, env_chunk=2)
    assert env.chunk_envs() == 2
    st = _placed(env, N, seed, ("near", "mid", "near"))
    gv, bv, _ = _volts(N, st)
    ids = np.array([0, 1, 2, 1, 0], np.int32)
    axes = np.array([[0, 1], [0, N + 1], [3, 0], [N, 2], [N + 1, N + 3]], np.int32)
    ctr = np.concatenate([gv, np.zeros((B, 1)), bv], axis=1)
    rg = np.stack([[ctr[e, a] - 1, ctr[e, a] + 2, ctr[e, b] + 2, ctr[e, b] - 1] for e, (a, b) in zip(ids, axes)])
    nq, g0, g1, guard = 5, 2, 3, -12345.678
    full = lambda *s: torch.full(s, guard, dtype=torch.float64, device="cuda")     # noqa: E731
    raw, plohi, occ = full(g0 + nq + g1, P), full(g0 + nq + g1, 2), full(g0 + nq + g1, P, N)
    img = torch.full((g0 + nq + g1, P), -7.0, dtype=torch.float32, device="cuda")
    flags = 1 | 4
    assert _raw_call(env, ids, axes, rg, gv[ids], bv[ids], nq, raw[g0:], img[g0:], plohi[g0:], occ[g0:], flags) == 0
    for a, gval in ((raw, guard), (plohi, guard), (occ, guard), (img, -7.0)):
        a = a.cpu().numpy()
        assert np.all(a[:g0] == gval) and np.all(a[g0 + nq:] == gval)
        assert np.isfinite(a[g0:g0 + nq]).all() and not np.any(a[g0:g0 + nq] == gval)
    # every query alone: same stream (stream_base + q) needs the same query index, so alone = the same call with the other
    # queries made inert
    for q in range(nq):
        ids1 = np.where(np.arange(nq) == q, ids, -1).astype(np.int32)
        r1, p1, o1 = full(nq, P), full(nq, 2), full(nq, P, N)
        i1 = torch.full((nq, P), -7.0, dtype=torch.float32, device="cuda")
        assert _raw_call(env, ids1, axes, rg, gv[ids], bv[ids], nq, r1, i1, p1, o1, flags) == 0
        assert PH.same(r1[q], raw[g0 + q]) and PH.same(p1[q], plohi[g0 + q]) and PH.same(o1[q], occ[g0 + q]) and PH.same(i1[q], img[g0 + q])
        others = np.arange(nq) != q
        assert np.all(r1.cpu().numpy()[others] == guard) and np.all(o1.cpu().numpy()[others] == guard)
        assert np.all(p1.cpu().numpy()[others] == guard) and np.all(i1.cpu().numpy()[others] == -7.0)
    # deterministic queries do not depend on their position either
    det = env.scan2d(ids, axes[:, 0], axes[:, 1], rg[:, :2], rg[:, 2:], gv[ids], bv[ids])["raw"]
    for q in range(nq):
        one = env.scan2d([int(ids[q])], int(axes[q, 0]), int(axes[q, 1]), rg[q, :2], rg[q, 2:], gv[ids[q]][None], bv[ids[q]][None])["raw"]
        assert PH.same(one[0], det[q]), q
    # inert queries
    bad_axes = np.array([[0, 2 * N], [2, 2], [-1, 1], [0, 1], [0, 1]], np.int32)
    bad_ids = np.array([0, 1, 2, B, -1], np.int32)
    r2, p2, o2 = full(nq, P), full(nq, 2), full(nq, P, N)
    assert _raw_call(env, bad_ids, bad_axes, rg, gv[ids], bv[ids], nq, r2, None, p2, o2, 0) == 0
    assert np.all(r2.cpu().numpy() == guard) and np.all(p2.cpu().numpy() == guard) and np.all(o2.cpu().numpy() == guard)
    env.close()


def test_scans_leave_no_footprint_on_a_noisy_run(tmp_path):
    """All stochastic stages on, env_chunk = 2, a rollout of 3 steps through a truncation with automatic resets, scans
    between all calls: byte-equal to the run without.  A probe and an eval_points call before and after are byte-equal."""
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
        x, y = ((0, N + 1), (N, 2), (3, 1))[k]
        ctr = np.concatenate([gv, np.zeros((n, 1)), bv], axis=1)
        out = poked.scan2d(ids, x, y, np.stack([ctr[:, x] - 1, ctr[:, x] + 2], 1), np.stack([ctr[:, y] + 1, ctr[:, y] - 2], 1),
                           gv, bv, noise=("sensor", "latch") if k != 1 else None, occupations=k == 2, normalised=True,
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
        out = dict(env.probe(np.arange(B), st[:, L.s_gate_gt:L.s_gate_gt + N] + 1.5, par[:, L.vbopt:L.vbopt + C], normalised=True))
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


# ------------------------------------------------------------------ 6. a degenerate axis
@pytest.mark.parametrize("N,R,pixel_search", [(4, 32, False), (4, 12, True), (8, 36, False), (2, 8, False)])
def test_degenerate_axis_repeats_a_sweep(tmp_path, N, R, pixel_search):
    """x_lo == x_hi: all columns of a row are bit-equal (default and pixel_search handles; a default handle from 4 dots and
    R >= 32 on runs the tile search, whose x plane then has slope 0).  The same for y_lo == y_hi and rows."""
    env = _vec(tmp_path, 1, N, R, 6600 + N, pixel_search=pixel_search)
    st = _placed(env, N, 6600 + N, ("near",))
    gv, bv, sv = _volts(N, st)
    for ax, ay in ((0, 1), (N + 1, 0), (1, N)):
        ctr = np.concatenate([gv[0], sv, bv[0]])
        out = env.scan2d([0, 0], ax, ay, [[ctr[ax] + 0.7] * 2, [ctr[ax] - 1, ctr[ax] + 2]],
                         [[ctr[ay] - 1, ctr[ay] + 2], [ctr[ay] - 0.3] * 2], gv[[0, 0]], bv[[0, 0]], sensor_voltage=sv[[0, 0]],
                         occupations=True)
        raw, occ = out["raw"].cpu().numpy(), out["occupations"].cpu().numpy()
        assert np.ptp(raw[0]) > 0 and np.ptp(raw[1]) > 0, (ax, ay)
        assert PH.same(raw[0], np.broadcast_to(raw[0][:, :1], (R, R))) and PH.same(occ[0], np.broadcast_to(occ[0][:, :1], (R, R, N)))
        assert PH.same(raw[1], np.broadcast_to(raw[1][:1, :], (R, R))) and PH.same(occ[1], np.broadcast_to(occ[1][:1], (R, R, N)))
    env.close()


# ------------------------------------------------------------------ 7. refusals on the device
def test_refusals(tmp_path):
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
            env.scan2d([0], 0, 1, (-1, 1), (-1, 1), gv, bv)
        assert f"code {_lib.QD_ERR_STATE}" in str(ei.value)
        assert PH.same(env.raw()[0], raw0)
        env.close()
    env = _vec(tmp_path, 1, N, R, 78)
    env.reset(seed=78)
    with pytest.raises(ValueError, match="radial"):
        env.scan2d([0], 0, 1, (-1, 1), (-1, 1), gv, bv, noise=("sensor", "radial"))
    import torch
    raw = torch.full((1, R * R), -5.0, dtype=torch.float64, device="cuda")
    rc = _raw_call(env, [0], [[0, 1]], [[-1, 1, -1, 1]], gv, bv, 1, raw, flags=_lib.QD_NOISE_RADIAL)
    assert rc == _lib.QD_ERR_ARG and b"radial" in env._lib.qd_last_error(env._h)
    assert np.all(raw.cpu().numpy() == -5.0)
    with pytest.raises(ValueError):
        env.scan2d([0], "vP1", "vP1", (-1, 1), (-1, 1), gv, bv)
    env.close()
