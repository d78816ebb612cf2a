"""Dense 1-D sweeps on the MI355X (run with -m gpu): qd_scan1d against qd_eval_points at the voltages of the host front end,
against row 0 of qd_scan_affine with and without noise, the latching walk along a line longer than the handle's image side
against the noise oracle, NumPy-built lines against the oracle, percentiles and image, the launch chunking with guard rows
and inert queries, the absent footprint on a noisy auto-resetting run, and the refusals."""
import ctypes

import numpy as np
import pytest
import yaml

import affine_helpers as AH
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


# ------------------------------------------------------------------ 1. lines = points
def _line_queries(N, st, par, seed):
    """(axis, s_range, frame, base W0, vgm or None, gamma or None) per query: a plunger, a barrier, e1_2 under a matrix
    override, a dict axis in the physical frame, dense directions in both frames, one with an explicit peak width.  The base
    point is the env's own voltages (its physical working point in the physical frame)."""
    L, G = layout(N), N + 1
    gv = st[L.s_gate_v:L.s_gate_v + N]; bvv = st[L.s_barrier_v:L.s_barrier_v + N - 1]; sv = st[L.s_sensor_gt]
    virt = np.concatenate([gv, [sv], bvv])
    phys = np.concatenate([_physical_point(N, st, par), bvv])
    rng = np.random.default_rng(seed)
    vgm = -np.eye(G) + rng.normal(0, 0.05, (G, G))
    return [(f"vP{N}", (-2.0, 2.5), "virtual", virt, None, None),
            ("B1", (3.0, -2.0), "virtual", virt, None, None),
            ("e1_2", (-1.5, 1.5), "virtual", virt, vgm, None),
            ({"P1": 0.5, "B1": -1.0}, (-1.0, 2.0), "physical", phys, None, None),
            (_dense(N, rng), (-1.2, 1.2), "virtual", virt, None, 0.7 * par[L.scal + 1]),
            (_dense(N, rng), (1.6, -0.8), "physical", phys, None, None)]


@pytest.mark.parametrize("N,K,R,n", [(2, 32, 8, 64), (4, 32, 12, 100), (8, 32, 8, 37), (8, 16, 8, 64), (8, 20, 8, 1)])
def test_lines_equal_points(tmp_path, N, K, R, n):
    """One handle, envs "near" and "mid": the raw signal of a line along a plunger, a barrier, e1_2 under a matrix override, a
    dict axis, and dense directions in both frames (one with an explicit gamma) has the bits of eval_points(signal) at the v_ext
    of the host front end (tests/hosttest_line).  The occupations have the bits of eval_points(occupations) for K = 20; for K in
    {8, 16, 32} the points solve the occupations from the reference order and the line from the search order: rtol 1e-9, atol
    1e-12, the rule of test_combination_axes_equal_points.  n = 64 fills the slot of an 8 x 8 handle, 100 one of 10 x 10 inside
    a 12 x 12 handle, 37 leaves a tail of 12 inert records, 1 is a slot of one record."""
    from qadapt_hip.vec_env import scan_axis_vector
    B, G = 2, N + 1
    seed = 8100 + 10 * N + K
    env = _vec(tmp_path, B, N, R, seed, num_charge_states=K)
    st = _placed(env, N, seed, ("near", "mid"))
    frames = set()
    for e in range(B):
        par = env._params_host[e]
        for axis, rg, frame, W0, vgm, gamma in _line_queries(N, st[e], par, seed + 1 + e):
            out = env.scan1d([e], axis, rg, n, W0[None, :N], W0[None, G:], W0[N], frame=frame, occupations=True,
                             vgm=None if vgm is None else vgm[None], gamma=gamma)
            qst = SH.query_state(N, st[e], W0[:N], W0[G:], float(W0[N]), vgm)
            v_ext, _, _ = LH.line_voltages(N, par, qst, scan_axis_vector(axis, N, frame), rg, n,
                                           LH.PHYSICAL if frame == "physical" else LH.VIRTUAL)
            pts = env.eval_points([e], v_ext[None, :, :G], v_ext[None, :, G:], gamma=gamma)
            raw, occ = _np(out["raw"])[0], _np(out["occupations"])[0]
            sig, occ_pts = _np(pts["signal"])[0], _np(pts["occupations"])[0]
            tag = (e, axis if isinstance(axis, str) else "dict/dense", frame, vgm is not None, gamma is not None)
            frames.add(frame)
            assert raw.shape == (n,) and occ.shape == (n, N) and np.isfinite(raw).all() and (n == 1 or np.ptp(raw) > 0), tag
            d = float(np.abs(raw - sig).max()); do = float(np.abs(occ - occ_pts).max())
            print(f"[line vs points] N={N} K={K} R={R} n={n} {tag}: raw diff {d:.3e}, occupation diff {do:.3e}")
            assert PH.same(raw, sig), (tag, d)
            if K in (8, 16, 32):
                assert np.allclose(occ, occ_pts, rtol=1e-9, atol=1e-12), (tag, do)
            else:
                assert PH.same(occ, occ_pts), (tag, do)
    assert frames == {"virtual", "physical"}
    env.close()


# ------------------------------------------------------------------ scenes with latching, fixed on the CPU
LATCH_SEED, LATCH_SERIAL, LATCH_BASE = 8200, (1 << 63) | 77, 1234


def _latch_scene(N, n, seed, axis, rg, p_lead=0.15, p_inter=0.15):
    """One device of `seed` "near" its ground truth (vgm_noise 0) whose parameter block latches often (every p_leads and p_inter
    entry set to the given probabilities); a virtual-frame line of n points along `axis` from the env's own voltages; the
    oracle's clean occupations there.  CPU only."""
    L, G = layout(N), N + 1
    eb = H.sample_blocks(N, [seed])
    rng = np.random.default_rng(seed)
    par, st = eb.params[0].copy(), H.place(N, eb.state[0], "near", rng, vgm_noise=0.0)
    par[L.pleads:L.pleads + N] = p_lead
    par[L.pinter:L.pinter + N * N] = p_inter
    from qadapt_hip.vec_env import scan_axis_vector
    d = scan_axis_vector(axis, N)
    grid = LH.numpy_line(N, st, par[L.origin:L.origin + G], d, rg, n)
    occ = O.ground_state_open(H.dev_view(N, par), grid[:, :G], grid[:, G:])
    return par, st, d, occ


def _walk(par, N, occ, R, q, seed):
    """the oracle's latching walk of query q on occupations occ (n, N) with rows of R"""
    L = layout(N)
    s = NO.Stream(seed, LATCH_BASE + q, LATCH_SERIAL)
    return NO.latch_walk(s, 0, occ, R, par[L.pleads:L.pleads + N], par[L.pinter:L.pinter + N * N].reshape(N, N))


# ------------------------------------------------------------------ 2. a line = row 0 of an affine scan
@pytest.mark.parametrize("N,K,R", [(4, 32, 16), (2, 32, 8), (8, 16, 12)])
def test_line_equals_row_0_of_an_affine_scan(tmp_path, N, K, R):
    """pixel_search handle, n = R: raw and occupations of the line have the bits of row 0 of scan_affine(dx = d, dy = 0),
    deterministically and with sensor noise and latching under the same serial and stream base -- row 0 of an image and a line
    share the point indices, the start of the telegraph chain and the latching walk.  Fixed on the CPU beforehand with the oracle:
    at least one point of each noisy line is latched."""
    L, G = layout(N), N + 1
    seed = LATCH_SEED + N
    axes = ["e1_2", f"vP{N}"]
    rgs = [(-6.0, 6.0), (7.0, -6.0)]
    scenes = [_latch_scene(N, R, seed, a, rg) for a, rg in zip(axes, rgs)]
    for q, (par, st, d, occ) in enumerate(scenes):
        latched = int((_walk(par, N, occ, R, q, seed) != occ).any(axis=1).sum())
        assert latched > 0, f"the oracle latches no point of line {q}"
    par, st = scenes[0][0], scenes[0][1]
    env = _vec(tmp_path, 1, N, R, seed, pixel_search=True, num_charge_states=K)
    _load(env, par[None], st[None])
    gv, bv, sv = _volts(N, st[None])
    dirs = np.stack([s[2] for s in scenes])
    zero = np.zeros_like(dirs)
    ids = [0, 0]
    for kw in (dict(), dict(noise=("sensor", "latch"), serial=LATCH_SERIAL, stream_base=LATCH_BASE)):
        line = env.scan1d(ids, dirs, rgs, R, gv[ids], bv[ids], sv[ids], occupations=True, **kw)
        img = env.scan_affine(ids, dirs, zero, rgs, (0.5, -0.25), gv[ids], bv[ids], sensor_voltage=sv[ids], occupations=True, **kw)
        for key in ("raw", "occupations"):
            a, b = _np(line[key]), _np(img[key])[:, 0]
            assert np.isfinite(a).all() and PH.same(a, b), ("noise" in kw, key, int((PH.bits(a) != PH.bits(b)).sum()))
        if kw:
            clean = env.scan1d(ids, dirs, rgs, R, gv[ids], bv[ids], sv[ids], occupations=True)
            assert not PH.same(clean["raw"], line["raw"])                          # the noise really ran
            held = (_np(clean["occupations"]) != _np(line["occupations"])).any(axis=2)
            print(f"[line vs affine row 0] N={N} R={R}: latched points per line {held.sum(axis=1).tolist()}")
            assert held.any(axis=1).all()
    env.close()


# ------------------------------------------------------------------ 3. the walk runs through
@pytest.mark.parametrize("N,R,n", [(4, 12, 90), (2, 8, 50)])
def test_latching_walks_the_line_as_one_row(tmp_path, N, R, n):
    """n > R of the handle; the slot side Rl = ceil(sqrt(n)) differs from R in the first case (90 points: 10, in a 12 x 12
    handle) and equals it in the second (50 points: 8, in an 8 x 8 handle).  With LATCH alone the occupations are, bit for bit,
    qd_noise_oracle.latch_walk called as ONE row of n on the clean occupations of a deterministic run of the same query, and
    differ from the walks that reset at multiples of Rl or of R.
    The corrected signal: the kernel adds 2 sum_i A[N][i] (held_i - n_i) to the sensor constant of a held point and forms the
    Lorentzians from it; the oracle's sensor_signal forms the eleven free energies from the held occupations and differences
    them.  The two are float64 evaluations of one expression that differ by the rounding of the free energies, eps |F| with
    |F| ~ 1e2 at these occupations: ~1e-14 in a difference dF, times a Lorentzian slope of at most 1 / gamma < 10, ~1e-13 in a
    signal of O(0.1).  The bound is rtol 1e-9, atol 1e-12, the one the line-against-points comparison uses where two
    evaluation orders meet; on the CPU the two expressions differ by at most 3.1e-13 relative on these lines."""
    from qadapt_hip.vec_env import scan_axis_vector
    L, G = layout(N), N + 1
    seed = LATCH_SEED + 50 + N
    axis, rg = "e1_2", (-20.0, 20.0)
    par, st, d, occ_oracle = _latch_scene(N, n, seed, axis, rg, p_lead=0.08, p_inter=0.08)
    side = LH.slot(n)[0]
    one = _walk(par, N, occ_oracle, n, 0, seed)
    assert int((one != occ_oracle).any(axis=1).sum()) >= 5, "the oracle latches too few points of the line"
    for rows in {side, R}:
        assert not np.array_equal(one, _walk(par, N, occ_oracle, rows, 0, seed)), f"a walk that resets every {rows} points gives the same line"
    env = _vec(tmp_path, 1, N, R, seed)
    _load(env, par[None], st[None])
    gv, bv, sv = _volts(N, st[None])
    clean = env.scan1d([0], axis, rg, n, gv, bv, sv, occupations=True)
    got = env.scan1d([0], axis, rg, n, gv, bv, sv, occupations=True, noise=("latch",), serial=LATCH_SERIAL, stream_base=LATCH_BASE)
    occ0, occ1 = _np(clean["occupations"])[0], _np(got["occupations"])[0]
    want = _walk(par, N, occ0, n, 0, seed)
    held = (want != occ0).any(axis=1)
    print(f"[latching along a line] N={N} R={R} n={n} side={side}: held points {int(held.sum())}, at multiples of side "
          f"{int(held[::side].sum())}, of R {int(held[::R].sum())}")
    assert held.sum() >= 5
    assert PH.same(occ1, want)
    for rows in {side, R}:
        assert not np.array_equal(occ1, _walk(par, N, occ0, rows, 0, seed)), rows
    v_ext, _, _ = LH.line_voltages(N, par, st, d, rg, n)
    sig = NO.sensor_signal(H.dev_view(N, par), v_ext, want, float(par[L.scal + 1]), np.zeros(n))
    raw0, raw1 = _np(clean["raw"])[0], _np(got["raw"])[0]
    print(f"[latching along a line] worst corrected signal difference {np.abs(raw1 - sig).max():.3e}")
    assert np.allclose(raw1, sig, rtol=1e-9, atol=1e-12)
    assert PH.same(raw1[~held], raw0[~held]) and not np.any(raw1[held] == raw0[held])
    env.close()


# ------------------------------------------------------------------ 4. the oracle on NumPy-built lines
ORACLE_SEEDS = {2: 50, 4: 50, 6: 51}
ORACLE_N = 64


def _oracle_lines(N):
    from qadapt_hip.vec_env import scan_axis_vector as vec
    return [(vec("e1_2", N), (-2.0, 2.0), "virtual"), (vec(f"vP{N}", N), (3.0, -2.0), "virtual"),
            (vec({"vP1": 1.0, "B1": -0.5}, N), (-1.5, 2.5), "virtual"),
            (_dense(N, np.random.default_rng(2000 + N)), (-1.2, 1.2), "physical")]


_ORACLE = {}


def _oracle_case(N):
    """The devices of seed ORACLE_SEEDS[N] "near" and "far" from the ground truth (rng of that seed, vgm_noise = 0); per env and
    line 64 points built in NumPy (line_helpers.numpy_line) from the env's own voltages (its physical working point in the
    physical frame) and the oracle's occupations, signal and relative gap there.  CPU only, computed once."""
    if N not in _ORACLE:
        n, L, G = ORACLE_N, layout(N), N + 1
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
            for d, rg, frame in _oracle_lines(N):
                base = phys if frame == "physical" else virt
                qst = SH.query_state(N, st, base[:N], bv, base[N])
                pts = LH.numpy_line(N, qst, par[L.origin:L.origin + G], d, rg, n, LH.PHYSICAL if frame == "physical" else LH.VIRTUAL)
                vg, vb = pts[:, :G], pts[:, G:]
                occ, sts, F, tc = O.ground_state_open(dev, vg, vb, return_states=True)
                sig, _ = O.charge_sensor_open(dev, vg, vb, n_open=occ)
                Hm = F[:, :, None] * np.eye(sts.shape[1]) + O.tunnel_hamiltonian(tc, sts)
                w = np.linalg.eigvalsh(Hm)
                hn = np.abs(Hm).sum(axis=2).max(axis=1)
                cases.append(dict(e=e, mode=mode, d=d, rg=np.array(rg), frame=frame, gv=base[:N], sv=base[N], bv=bv, occ=occ,
                                  sig=sig[:, 0], rel_gap=(w[:, 1] - w[:, 0]) / hn))
        _ORACLE[N] = (eb.params[:2], np.stack(states), cases)
    return _ORACLE[N]


@pytest.mark.parametrize("N", [2, 4, 6])
def test_lines_against_the_oracle(tmp_path, N):
    """O.ground_state_open / O.charge_sensor_open at NumPy-built lines of 64 points, on a device near and one far from its ground
    truth: e1_2, vP_N downwards, a plunger with a compensating barrier, and a dense physical direction.  The per-point rule of
    helpers: where the oracle's relative gap is above GAP_MIN, occupations and signal agree within 1e-6; 0 of 64 points may be
    excused.  Checked on the CPU beforehand: the oracle alone leaves 0 of 64 points unresolved in each of the 8 lines."""
    params, state, cases = _oracle_case(N)
    assert len(cases) == 8 and {c["mode"] for c in cases} == {"near", "far"}
    for c in cases:
        unres = int((c["rel_gap"] <= H.GAP_MIN).sum())
        assert unres == 0, f"the oracle alone leaves {unres} of 64 points unresolved"
    env = _vec(tmp_path, 2, N, 8, ORACLE_SEEDS[N])
    _load(env, params, state)
    for k, c in enumerate(cases):
        out = env.scan1d([c["e"]], c["d"], c["rg"], ORACLE_N, c["gv"][None], c["bv"][None], c["sv"], frame=c["frame"], occupations=True)
        occ, sig = _np(out["occupations"])[0], _np(out["raw"])[0]
        ok = c["rel_gap"] > H.GAP_MIN
        d_occ = np.abs(occ - c["occ"]).max(axis=1)
        d_sig = np.abs(sig - c["sig"]) / np.maximum(np.abs(c["sig"]), 1e-3)
        print(f"[line vs oracle] N={N} line {k} {c['mode']} {c['frame']}: worst occupation {d_occ[ok].max():.3e}, worst signal "
              f"{d_sig[ok].max():.3e}, unresolved {int((~ok).sum())}, smallest gap {c['rel_gap'].min():.2e}, total charge "
              f"{c['occ'].sum(axis=1).min():.2f}..{c['occ'].sum(axis=1).max():.2f}")
        assert np.all(c["rel_gap"][d_occ > 1e-6] <= H.GAP_MIN), d_occ[ok].max()
        assert np.all(c["rel_gap"][d_sig > 1e-6] <= H.GAP_MIN), d_sig[ok].max()
        assert int((~ok).sum()) == 0
    env.close()


# ------------------------------------------------------------------ 5. percentiles and image
def test_percentiles_and_image(tmp_path):
    """plohi has the bits of np.percentile(raw, [0.5, 99.5]) and image those of O.normalise_image(raw), per line: lines of 1, 2, 37,
    64 and 256 points with and without sensor noise, a constant line (lo == hi: all zeros), and the zero direction."""
    N, R = 4, 16
    env = _vec(tmp_path, 2, N, R, 8500)
    st = _placed(env, N, 8500, ("near", "mid"))
    gv, bv, sv = _volts(N, st)
    ids = [0, 1, 1]
    for n in (1, 2, 37, 64, 256):
        for kw in (dict(), dict(noise=("sensor",), serial=(1 << 63) | 3)):
            out = env.scan1d(ids, ["e1_2", "vP1", np.zeros(2 * N)], [(-2.0, 2.0), (1.25, 1.25), (-1.0, 1.0)], n, gv[ids], bv[ids], sv[ids], **kw)
            raw, img, plohi = _np(out["raw"]), _np(out["image"]), _np(out["plohi"])
            assert raw.shape == (3, n) and img.shape == (3, n) and img.dtype == np.float32 and plohi.shape == (3, 2)
            for q in range(3):
                assert PH.same(plohi[q], np.percentile(raw[q], [0.5, 99.5])), (n, q, bool(kw))
                assert PH.same(img[q], O.normalise_image(raw[q])), (n, q, bool(kw))
            if not kw:
                # the constant line and the zero direction repeat one point: equal signals, equal percentiles, an all-zero image
                for q in (1, 2):
                    assert PH.same(raw[q], np.full(n, raw[q, 0])) and plohi[q, 0] == plohi[q, 1] and not img[q].any(), (n, q)
            if n > 2:
                assert np.ptp(raw[0]) > 0 and img[0].max() == 1.0 and img[0].min() == 0.0
            if n == 1:
                assert not img.any()
    env.close()


# ------------------------------------------------------------------ 6. chunking, guards, inert queries
def _raw_call(env, ids, dirs, rg, gv, bv, nq, n, raw, image=None, plohi=None, occ=None, flags=0):
    import torch
    from qadapt_hip import _lib
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dt)).cuda()      # noqa: E731
    keep = [t(ids, np.int32), t(dirs, np.float64), t(rg, np.float64), t(gv, np.float64), t(bv, np.float64)]
    o = _lib.QdScan1dOpts(struct_size=ctypes.sizeof(_lib.QdScan1dOpts), noise_flags=flags, serial=(1 << 63) | 5,
                          occ_dst=None if occ is None else occ.data_ptr())
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())          # noqa: E731
    rc = env._lib.qd_scan1d(env._h, p(keep[0]), nq, n, p(keep[1]), p(keep[2]), p(keep[3]), p(keep[4]), None, p(raw), p(image),
                            p(plohi), ctypes.byref(o), env._stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("R,n,chunks", [(8, 64, (2, 3)), (8, 37, (2, 3)), (20, 256, (1, 2))])
def test_guards_inert_queries_and_chunks(tmp_path, R, n, chunks):
    """7 queries on 3 envs through the C entry point with sensor noise and latching, guard rows on both sides of every
    destination: the same bits with two values of env_chunk that cut the call into launches differently.  A 4-dot 8 x 8 handle
    with env_chunk 2 and 3 has 6 and 9 slabs, one per slot of 64 or 49 records, which its 384 and 576 records also hold at
    64 but exceed at 49: the slabs set the slot count, two launches (6 + 1) then one.  A 20 x 20 handle with env_chunk 1 and 2
    holds 1200 and 2400 records, 4 and 9 slots of 256, but 6 and 12 slabs: there the records set it, two launches (4 + 3) then
    one.  Then env ids outside [0, B) leave their pre-filled slots untouched while the live queries beside them keep their
    bits, and a call whose queries are all inert writes nothing."""
    import torch
    from qadapt_hip.vec_env import scan_axis_vector as vec
    N, B, seed = 4, 3, 8600
    ids = np.array([0, 1, 2, 1, 0, 2, 2], np.int32)
    nq, g0, g1, guard = 7, 2, 3, -12345.678
    full = lambda *s: torch.full(s, guard, dtype=torch.float64, device="cuda")     # noqa: E731
    rng = np.random.default_rng(seed)
    dirs = np.stack([vec("e1_2", N), vec("U1_4", N), _dense(N, rng), vec("B2", N), vec("vP1", N), _dense(N, rng),
                     vec({"vP2": 1.0, "B2": -0.5}, N)])
    rg = np.tile([-2.5, 2.5], (nq, 1)) + rng.uniform(-0.3, 0.3, (nq, 2))
    rg[3] = rg[3, ::-1]
    flags = 1 | 4
    results = {}
    for chunk in chunks:
        env = _vec(tmp_path, B, N, R, seed, env_chunk=chunk)
        assert env.chunk_envs() == chunk
        st = _placed(env, N, seed, ("near", "mid", "near"))
        gv, bv, _ = _volts(N, st)
        raw, plohi, occ = full(g0 + nq + g1, n), full(g0 + nq + g1, 2), full(g0 + nq + g1, n, N)
        img = torch.full((g0 + nq + g1, n), -7.0, dtype=torch.float32, device="cuda")
        assert _raw_call(env, ids, dirs, rg, gv[ids], bv[ids], nq, n, raw[g0:], img[g0:], plohi[g0:], occ[g0:], flags) == 0
        out = [a.cpu().numpy() for a in (raw, plohi, occ, img)]
        for a, gval in zip(out, (guard, guard, guard, -7.0)):
            assert np.all(a[:g0] == gval) and np.all(a[g0 + nq:] == gval)
            assert np.isfinite(a[g0:g0 + nq]).all() and not np.any(a[g0:g0 + nq] == gval)
        results[chunk] = out
        if chunk == chunks[0]:
            # inert queries: their slots keep the pre-fill, the live ones keep their bits (same query index = same streams)
            bad_ids = np.array([0, B, -1, 1, B + 5, 2, -7], np.int32)
            live = (bad_ids >= 0) & (bad_ids < B)
            r2, p2, o2 = full(nq, n), full(nq, 2), full(nq, n, N)
            i2 = torch.full((nq, n), -7.0, dtype=torch.float32, device="cuda")
            assert _raw_call(env, bad_ids, dirs, rg, gv[ids], bv[ids], nq, n, r2, i2, p2, o2, flags) == 0
            for a, b, gval in zip((r2, p2, o2, i2), out, (guard, guard, guard, -7.0)):
                a = a.cpu().numpy()
                assert np.all(a[~live] == gval)
                assert PH.same(a[live], b[g0:g0 + nq][live])
            # an all-inert call writes nothing at all
            r3 = full(nq, n)
            assert _raw_call(env, np.full(nq, B, np.int32), dirs, rg, gv[ids], bv[ids], nq, n, r3, flags=flags) == 0
            assert np.all(r3.cpu().numpy() == guard)
        env.close()
    for a, b in zip(results[chunks[0]], results[chunks[1]]):
        assert PH.same(a, b)


# ------------------------------------------------------------------ 7. nothing else moves
def test_lines_leave_no_footprint_on_a_noisy_run(tmp_path):
    """Two handles with all stochastic stages on, env_chunk = 2, a rollout of 3 steps through a truncation with automatic
    reloads; one of them calls scan1d between all calls: observations, rewards, state blocks, raw signal, percentiles, parameter
    blocks and the observation serial stay byte-identical.  A probe, a scan2d, a scan_affine and an eval_points call before and
    after are byte-equal."""
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
        axis = ("e1_2", _dense(N, prng), {"vP3": 1.0, "B2": -0.4})[k]
        out = poked.scan1d(ids, axis, (-1.5, 1.5), (100, 256, 7)[k], gv, bv, noise=("sensor", "latch") if k != 1 else None,
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


# ------------------------------------------------------------------ 8. refusals
def test_refusals(tmp_path):
    import torch
    from qadapt_hip import _lib
    N, R = 3, 8
    q = DM.load_yaml(None, "qarray_config.yaml")
    q["simulator"]["model"]["max_charge_carriers"] = 2
    qp = tmp_path / "qarray_m2.yaml"
    qp.write_text(yaml.safe_dump(q))
    gv, bv = np.zeros((1, N)), np.zeros((1, N - 1))
    d = AH.unit(N, 0)[None]
    for kw, word in ((dict(validate=True), "QD_FLAG_VALIDATE"),
                     (dict(num_charge_states="all", qarray_config_path=str(qp)), "full charge-state space")):
        env = _vec(tmp_path, 1, N, R, 77, **kw)
        env.reset(seed=77)
        raw0 = env.raw()[0].copy()
        with pytest.raises(_lib.QdError, match=word) as ei:
            env.scan1d([0], "e1_2", (-1, 1), 16, gv, bv)
        assert f"code {_lib.QD_ERR_STATE}" in str(ei.value)
        dst = torch.full((1, 16), -5.0, dtype=torch.float64, device="cuda")
        assert _raw_call(env, [0], d, [[-1, 1]], gv, bv, 1, 16, dst) == _lib.QD_ERR_STATE
        assert np.all(dst.cpu().numpy() == -5.0)
        assert PH.same(env.raw()[0], raw0)
        env.close()
    env = _vec(tmp_path, 1, N, R, 78)
    env.reset(seed=78)
    with pytest.raises(ValueError, match="radial"):
        env.scan1d([0], "e1_2", (-1, 1), 16, gv, bv, noise=("sensor", "radial"))
    for bad in (0, R * R + 1):
        with pytest.raises(ValueError, match="n_points"):
            env.scan1d([0], "e1_2", (-1, 1), bad, gv, bv)
    raw = torch.full((1, 16), -5.0, dtype=torch.float64, device="cuda")
    rc = _raw_call(env, [0], d, [[-1, 1]], gv, bv, 1, 16, raw, flags=_lib.QD_NOISE_RADIAL)
    assert rc == _lib.QD_ERR_ARG and b"radial" in env._lib.qd_last_error(env._h)
    rc = _raw_call(env, [0], d, [[-1, 1]], gv, bv, 1, R * R + 1, raw)
    assert rc == _lib.QD_ERR_ARG and b"n_points" in env._lib.qd_last_error(env._h)
    assert np.all(raw.cpu().numpy() == -5.0)
    out = env.scan1d([0], "e1_2", (-1, 1), R * R, gv, bv)                       # n = P is the longest line
    assert np.isfinite(_np(out["raw"])).all() and out["raw"].shape == (1, R * R)
    with pytest.raises(ValueError):
        env.scan1d([0], "e1_1", (-1, 1), 16, gv, bv)
    env.close()
