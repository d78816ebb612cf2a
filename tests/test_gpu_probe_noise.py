"""Probe scans with the stochastic stages and the occupations on the MI355X (run with -m gpu): qd_probe_ex against the
qd_observe it must reproduce bit for bit, against the NumPy restatement of the noise rules on a stream of its own, across
launch chunks, its occupations against the oracle, NaN and guard slots, and `array._get_obs(noise=True)`.  The scenes and
what the oracle alone says about them come from tests/probe_noise_helpers.py and need no GPU."""
import ctypes

import numpy as np
import pytest
import yaml

import helpers as H
import probe_noise_helpers as PN
from qadapt_hip import device_model as DM
from qadapt_hip.layout import layout

pytestmark = pytest.mark.gpu

TOP = 1 << 63


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


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _serial(env):
    ser = ctypes.c_uint64(0)
    assert env._lib.qd_get_rng_state(env._h, ctypes.byref(ser)) == 0
    return int(ser.value)


def _own_queries(L, st):
    """every env's own gate and barrier voltages and sensor slot"""
    N = L.N
    return (st[:, L.s_gate_v:L.s_gate_v + N].copy(), st[:, L.s_barrier_v:L.s_barrier_v + N - 1].copy(),
            st[:, L.s_sensor_gt].copy())


def _replaced(L, par, st, gv, ch):
    full = par[L.noise + 6]
    gt = st[L.s_gate_gt:L.s_gate_gt + L.N]
    return bool(full > 0 and (abs(gv[ch] - gt[ch]) > full or abs(gv[ch + 1] - gt[ch + 1]) > full))


# ------------------------------------------------------------------ 1. equivalence with a step
@pytest.mark.parametrize("flags", [["sensor"], ["radial"], ["latch"], ["sensor", "radial", "latch"]])
def test_probe_has_the_bits_of_the_noisy_observe(tmp_path, flags):
    """Two handles of the same seed, env_id_offset = 40, B = 3, N = 4, R = 24, at the offsets [1.5, 27.0, 70.0] of
    test_noisy_observation_matches_numpy_restatement (latched pixels in envs 0 and 1, every channel of env 2 replaced:
    probe_noise_helpers.noise_reference says so on the CPU).  A observes; B probes with its own voltages, the handle's
    noise flags, stream_base = env_id_offset and the serial of A's observe."""
    B, N, R, C = PN.B, PN.N, PN.R, PN.N - 1
    if "latch" in flags:
        ref = PN.noise_reference(PN.OFF, 1, tuple(flags))
        assert sum(c.latched for q in ref for c in q) > 0, "the scene was meant to contain latched pixels"
    params, state = PN.noise_scene()
    a, b = [_vec(tmp_path, B, N, R, PN.SEED, env_id_offset=PN.OFF, noise=flags) for _ in range(2)]
    L = a.L
    st = PN.load_scene(a, params, state)
    assert _same(PN.load_scene(b, params, state), st)
    assert any(_replaced(L, params[2], st[2], st[2, L.s_gate_v:L.s_gate_v + N], ch) for ch in range(C))
    b_raw0, b_plohi0 = b.raw()
    b_ser0 = _serial(b)
    a.observe()
    S = _serial(a)
    assert S == b_ser0 + 1
    raw_a, plohi_a = a.raw()
    img_a = a.global_image.cpu().numpy().copy()
    gv, bv, sv = _own_queries(L, st)
    out = b.probe(np.arange(B), gv, bv, sensor_voltage=sv, normalised=True, noise=flags, serial=S, stream_base=PN.OFF,
                  occupations="latch" in flags)
    assert np.isfinite(raw_a).all() and np.ptp(raw_a) > 0
    assert _same(out["raw"].reshape(B, C, R * R), raw_a)
    assert _same(out["plohi"], plohi_a)
    assert _same(out["image"], img_a)
    if "latch" in flags:
        occ_a = a.occupations()
        occ_b = out["occupations"].cpu().numpy().reshape(B, C, R * R, N)
        for e in range(B):
            for ch in range(C):
                if "radial" in flags and _replaced(L, params[e], st[e], gv[e], ch):
                    assert np.isnan(occ_b[e, ch]).all(), (e, ch)          # never solved, in the step as in the probe
                else:
                    assert _same(occ_b[e, ch], occ_a[e, ch]), (e, ch)
    # noise=True is the handle's own stages
    again = b.probe(np.arange(B), gv, bv, sensor_voltage=sv, noise=True, serial=S, stream_base=PN.OFF)
    assert _same(again["raw"], out["raw"])
    # the probes moved nothing of B: state, raw signal, serial are as before, and its next observe is A's
    st_b, steps_b = b.get_state()
    assert _same(st_b, st) and not steps_b.any()
    b_raw1, b_plohi1 = b.raw()
    assert _same(b_raw1, b_raw0) and _same(b_plohi1, b_plohi0) and _serial(b) == b_ser0
    b.observe()
    raw_b, plohi_b = b.raw()
    assert _serial(b) == S and _same(raw_b, raw_a) and _same(plohi_b, plohi_a) and _same(b.global_image, img_a)
    if "latch" in flags:
        ok = np.array([[not ("radial" in flags and _replaced(L, params[e], st[e], gv[e], ch)) for ch in range(C)] for e in range(B)])
        assert _same(b.occupations()[ok], occ_a[ok])
    a.close(); b.close()


# ------------------------------------------------------------------ 2. against the NumPy restatement
def test_noisy_probe_matches_numpy_restatement(tmp_path):
    """The same scene probed with stream_base = 1000 and a top-bit serial, all three stages, on a handle created WITHOUT
    noise: query q against NO.Stream(seed, 1000 + q, serial) + OC.csd_channel + NO.observe_channel, with the tolerances of
    test_noisy_observation_matches_numpy_restatement."""
    B, N, R, C = PN.B, PN.N, PN.R, PN.N - 1
    base, serial = 1000, TOP | 11
    ref = PN.noise_reference(base, serial)
    assert sum(c.latched for q in ref for c in q) > 0, "the scene was meant to contain latched pixels"
    assert any(c.replaced for q in ref for c in q) and any(c.ok.any() for q in ref for c in q)
    params, state = PN.noise_scene()
    env = _vec(tmp_path, B, N, R, PN.SEED, env_id_offset=PN.OFF)
    st = PN.load_scene(env, params, state)
    gv, bv, sv = _own_queries(env.L, st)
    out = env.probe(np.arange(B), gv, bv, sensor_voltage=sv, noise=PN.ALL, serial=serial, stream_base=base, occupations=True)
    raw = out["raw"].cpu().numpy().reshape(B, C, R * R)
    occ = out["occupations"].cpu().numpy().reshape(B, C, R * R, N)
    latched = 0
    for q in range(B):
        for ch, c in enumerate(ref[q]):
            if c.replaced:
                print(f"[noisy probe vs numpy] query {q} ch {ch}: pure noise, worst {np.abs(raw[q, ch] - c.z).max():.3e}")
                assert np.allclose(raw[q, ch], c.z, rtol=1e-12, atol=1e-12), (q, ch)
                assert np.isnan(occ[q, ch]).all()
                continue
            ok = c.ok
            print(f"[noisy probe vs numpy] query {q} ch {ch}: {int(ok.sum())} pixels compared, latched {c.latched}, worst raw "
                  f"{np.abs(raw[q, ch][ok] - c.z[ok]).max() if ok.any() else 0.0:.3e}")
            assert np.allclose(occ[q, ch][ok], c.occ[ok], rtol=1e-6, atol=1e-6), (q, ch)
            assert np.allclose(raw[q, ch][ok], c.z[ok], rtol=1e-6, atol=1e-9), (q, ch)
            # the GPU held the pixels the oracle held: a held pixel carries its left neighbour's occupations
            det = PN.noise_reference(base, serial, ("sensor", "radial"))[q][ch].occ
            held = (c.occ != det).any(axis=1) & ok
            latched += int(np.all(occ[q, ch][held] == occ[q, ch][np.nonzero(held)[0] - 1], axis=1).sum())
    assert latched > 0
    # another serial, another stream base: other noise; the same again: the same bits
    for kw in (dict(serial=serial + 1, stream_base=base), dict(serial=serial, stream_base=base + 1)):
        other = env.probe(np.arange(B), gv, bv, sensor_voltage=sv, noise=PN.ALL, **kw)
        assert not _same(other["raw"], out["raw"])
    same = env.probe(np.arange(B), gv, bv, sensor_voltage=sv, noise=PN.ALL, serial=serial, stream_base=base)
    assert _same(same["raw"], out["raw"])
    # serial=None: a fresh top-bit serial per noisy call
    d1 = env.probe(np.arange(B), gv, bv, sensor_voltage=sv, noise=PN.ALL)
    d2 = env.probe(np.arange(B), gv, bv, sensor_voltage=sv, noise=PN.ALL)
    assert not _same(d1["raw"], d2["raw"]) and env._probe_serials == 2
    first = env.probe(np.arange(B), gv, bv, sensor_voltage=sv, noise=PN.ALL, serial=TOP | 0)
    assert _same(first["raw"], d1["raw"])
    env.close()


# ------------------------------------------------------------------ 3. chunks, many queries per env
def test_noisy_probe_does_not_depend_on_the_launch_chunk(tmp_path):
    """7 queries on the 3 envs (env 1 three times), all stages, occupations and images: a handle with env_chunk = 2 (four
    launch chunks, the stream base advancing with each) against one with the default chunk (the whole batch: chunks of
    3, 3 and 1 queries)."""
    B, N, R, C = PN.B, PN.N, PN.R, PN.N - 1
    params, state = PN.noise_scene()
    L = layout(N)
    ids = np.array([0, 1, 2, 0, 1, 2, 1], np.int32)
    rng = np.random.default_rng(31)
    gv = state[ids, L.s_gate_gt:L.s_gate_gt + N] + np.array([1.5, 27.0, 70.0, 3.0, 0.5, 33.0, 2.0])[:, None] + rng.uniform(-1, 1, (7, N))
    bv = state[ids, L.s_barrier_gt:L.s_barrier_gt + C] + rng.uniform(-2, 2, (7, C))
    sv = state[ids, L.s_sensor_gt] + rng.uniform(-0.2, 0.2, 7)
    win = rng.uniform(1.0, 2.0, 7)
    outs = []
    for chunk in (2, 0):
        env = _vec(tmp_path, B, N, R, PN.SEED, env_id_offset=PN.OFF, env_chunk=chunk)
        assert env.chunk_envs() == (chunk or B)
        PN.load_scene(env, params, state)
        det = env.probe(ids, gv, bv, sensor_voltage=sv, window=win)
        out = env.probe(ids, gv, bv, sensor_voltage=sv, window=win, normalised=True, noise=PN.ALL, serial=TOP | 77,
                        stream_base=5, occupations=True)
        assert not _same(out["raw"], det["raw"])
        outs.append({k: v.cpu().numpy() for k, v in out.items()})
        env.close()
    assert outs[0].keys() == outs[1].keys() == {"raw", "image", "plohi", "occupations"}
    for k in outs[0]:
        assert _same(outs[0][k], outs[1][k]), k
    occ = outs[0]["occupations"]
    nan_ch = np.isnan(occ).all(axis=(2, 3, 4))
    assert nan_ch.any() and not nan_ch.all() and np.array_equal(np.isnan(occ).any(axis=(2, 3, 4)), nan_ch)
    # queries 1, 4 and 6 name one env and sit at different voltages on different streams
    assert not _same(outs[0]["raw"][1], outs[0]["raw"][4]) and not _same(outs[0]["raw"][4], outs[0]["raw"][6])


# ------------------------------------------------------------------ 4. occupations without noise
@pytest.mark.parametrize("N", [4, 8])
def test_occupations_of_a_clean_probe_match_the_oracle(tmp_path, N):
    R, C = 16, N - 1
    params, st, ref = PN.occ_scene(N)
    for e in range(2):                                           # a condition on the case, fixed on the CPU
        for ch in range(C):
            unres = int((ref[e][ch].rel_gap <= H.GAP_MIN).sum())
            assert unres <= 0.01 * R * R, (N, e, ch, unres)
    env = _vec(tmp_path, 2, N, R, PN.OCC_CASES[N])
    L = env.L
    PN.load_scene(env, params, st)
    gv, bv, sv = _own_queries(L, st)
    plain = env.probe([0, 1], gv, bv, sensor_voltage=sv)
    assert "occupations" not in plain
    out = env.probe([0, 1], gv, bv, sensor_voltage=sv, occupations=True)
    assert _same(out["raw"], plain["raw"])                        # asking for them only adds stores
    assert env._probe_serials == 0                               # no noisy call was made
    occ = out["occupations"].cpu().numpy()
    assert occ.shape == (2, C, R, R, N)
    occ = occ.reshape(2, C, R * R, N)
    for e in range(2):
        for ch in range(C):
            d = np.abs(occ[e, ch] - ref[e][ch].occ).max(axis=1)
            ok = ref[e][ch].rel_gap > H.GAP_MIN
            print(f"[probe occupations vs oracle] N={N} env {e} ch {ch}: worst {d[ok].max():.3e}, unresolved {int((~ok).sum())}")
            assert np.all(ref[e][ch].rel_gap[d > 1e-6] <= H.GAP_MIN), (e, ch, d[ok].max())
    env.close()


def test_occupations_in_the_full_space_sum_to_whole_carriers(tmp_path):
    """(3 dots, 4 carriers) at 8x8: hopping conserves the total charge, so wherever the ground vector is resolved the
    occupations add up to an integer."""
    N, R, m, seed = 3, 8, 4, 6203
    params, st, gaps = PN.full_scene(R, m, seed)
    q = DM.load_yaml(None, "qarray_config.yaml")
    q["simulator"]["model"]["max_charge_carriers"] = m
    qp = tmp_path / "qarray_m4.yaml"
    qp.write_text(yaml.safe_dump(q))
    env = _vec(tmp_path, 2, N, R, seed, num_charge_states="all", qarray_config_path=str(qp))
    PN.load_scene(env, params, st)
    gv, bv, sv = _own_queries(env.L, st)
    plain = env.probe([0, 1], gv, bv, sensor_voltage=sv)
    out = env.probe([0, 1], gv, bv, sensor_voltage=sv, occupations=True)
    assert _same(out["raw"], plain["raw"])
    occ = out["occupations"].cpu().numpy().reshape(2, N - 1, R * R, N)
    assert np.isfinite(occ).all() and occ.min() >= -1e-9 and occ.max() <= m + 1e-9
    applies = 0
    for e in range(2):
        for ch in range(N - 1):
            ok = gaps[e][ch] > H.GAP_MIN
            tot = occ[e, ch].sum(axis=1)
            assert np.all(np.abs(tot - np.round(tot))[ok] < 1e-6), (e, ch)
            applies += int(ok.sum())
    assert applies >= 0.99 * 2 * (N - 1) * R * R
    env.close()


# ------------------------------------------------------------------ 5. NaN and guard slots
def test_replaced_channels_are_nan_and_foreign_ids_leave_their_slots(tmp_path):
    import torch
    N, R, B, seed = 4, 16, 2, 66
    C, guard = N - 1, -7.0
    env = _vec(tmp_path, B, N, R, seed)
    env.load_new_devices(seed=seed)
    st, _ = env.get_state()
    L = env.L
    ids = np.array([1, B, 0, -1], np.int32)                      # B and -1 are out of range
    gt = st[[1, 0, 0, 0], L.s_gate_gt:L.s_gate_gt + N]
    gv = gt + 1.0
    gv[0, 0] += 80.0                                             # query 0: gate 0 far beyond full_noise_distance -> channel 0 replaced
    bv = st[[1, 0, 0, 0], L.s_barrier_gt:L.s_barrier_gt + C]
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()      # noqa: E731
    ids_d, gv_d, bv_d = t(ids, torch.int32), t(gv, torch.float64), t(bv, torch.float64)
    raw = torch.full((4, C, R, R), guard, dtype=torch.float64).cuda()
    occ = torch.full((4, C, R, R, N), guard, dtype=torch.float64).cuda()
    from qadapt_hip import _lib
    opts = _lib.QdProbeOpts(struct_size=ctypes.sizeof(_lib.QdProbeOpts), noise_flags=_lib.QD_NOISE_RADIAL, serial=TOP | 1,
                            stream_base=0, occ_dst=occ.data_ptr())
    p = lambda x: ctypes.c_void_p(x.data_ptr())                                       # noqa: E731
    rc = env._lib.qd_probe_ex(env._h, p(ids_d), 4, p(gv_d), p(bv_d), None, None, p(raw), None, None, ctypes.byref(opts),
                              env._stream())
    assert rc == 0
    raw, occ = raw.cpu().numpy(), occ.cpu().numpy()
    for q in (1, 3):
        assert np.all(raw[q] == guard) and np.all(occ[q] == guard)
    assert np.isnan(occ[0, 0]).all() and np.isfinite(occ[0, 1:]).all() and np.isfinite(occ[2]).all()
    assert np.isfinite(raw[[0, 2]]).all() and abs(raw[0, 0].std() - 1.0) < 0.2           # pure N(0, 1) image, 256 pixels
    # the slots of the valid ids are what the Python entry point gives for them
    ref = env.probe([1, 0], gv[[0, 2]], bv[[0, 2]], noise=["radial"], serial=TOP | 1, stream_base=0, occupations=True)
    # (query 2 drew from stream 2 above and draws from stream 1 here: compare its noise-free part, the occupations)
    assert _same(ref["raw"][0], raw[0]) and _same(ref["occupations"][0], occ[0]) and _same(ref["occupations"][1], occ[2])
    # a validate handle still refuses, with options as without
    val = _vec(tmp_path, B, N, R, seed, validate=True)
    val.load_new_devices(seed=seed)
    with pytest.raises(_lib.QdError, match=r"code 3.*QD_FLAG_VALIDATE"):
        val.probe([0], gv[2:3], bv[2:3], noise=["sensor"])
    val.close(); env.close()


# ------------------------------------------------------------------ 6. the array facade
def test_get_obs_with_noise_on_a_single_env(tmp_path):
    from qadapt_hip.env import QuantumDeviceEnv
    N, R, seed = 4, 16, 515
    path = _cfg(tmp_path, num_dots=N, resolution=R)
    envs = [QuantumDeviceEnv(config_path=path, backend=_vec(tmp_path, 1, N, R, seed, config_path=path, noise=PN.ALL))
            for _ in range(2)]
    probed, twin = envs
    for env in envs:
        env.reset(seed=seed)
    gt = probed.device_state["gate_ground_truth"].astype(np.float64)
    bgt = probed.device_state["barrier_ground_truth"].astype(np.float64)
    clean = probed.array._get_obs(gt + 0.5, bgt)["image"]
    assert _same(clean, probed.array._get_obs(gt + 0.5, bgt, noise=False)["image"])
    n1 = probed.array._get_obs(gt + 0.5, bgt, noise=True)["image"]
    n2 = probed.array._get_obs(gt + 0.5, bgt, noise=True)["image"]
    assert n1.shape == clean.shape == (R, R, N - 1) and np.isfinite(n1).all()
    assert not _same(n1, clean) and not _same(n1, n2)
    assert np.mean(n1 != clean) > 0.5                            # white noise on the sensor potential reaches every pixel
    act = {"action_gate_voltages": np.linspace(-0.3, 0.3, N).astype(np.float32),
           "action_barrier_voltages": np.linspace(0.2, -0.2, N - 1).astype(np.float32)}
    outs = [env.step(act) for env in envs]
    for k in ("image", "obs_gate_voltages", "obs_barrier_voltages"):
        assert _same(outs[0][0][k], outs[1][0][k]), k
    assert _same(outs[0][1]["gates"], outs[1][1]["gates"])
    assert _same(probed._b.raw()[0], twin._b.raw()[0]) and _serial(probed._b) == _serial(twin._b)
    for env in envs:
        env.close()


# ------------------------------------------------------------------ 7. maps
def test_centred_map_with_noise_shows_the_white_noise_region(tmp_path):
    """3 x 3 tiles 50 V apart: the outer tiles lie beyond full_noise_distance (30..40 V) and are white noise with
    noise=["radial"], as in the reference's maps; without the keyword the map is the clean one of before."""
    from qadapt_hip import device_map as M
    N, R, seed = 4, 16, 808
    vec = _vec(tmp_path, 1, N, R, seed)
    vec.load_new_devices(seed=seed)
    full = float(vec._params_host[0, vec.L.noise + 6])
    assert 0 < full < 50.0
    clean = M.map_device_range(vec, 0, 0, half_range=75.0, window_size=50.0)
    noisy = M.map_device_range(vec, 0, 0, half_range=75.0, window_size=50.0, noise=["radial"])
    assert (noisy["n_scans_x"], noisy["n_scans_y"]) == (3, 3) and noisy["positions"] == clean["positions"]
    a, b = clean["scans"].cpu().numpy(), noisy["scans"].cpu().numpy()
    for k in range(9):
        if k == 4:                                               # the centre tile: the ramp's noise, not a replacement
            assert np.abs(b[k] - a[k]).max() < 1.0
        else:
            assert abs(b[k].mean()) < 0.3 and abs(b[k].std() - 1.0) < 0.2, k      # 256 samples of N(0, 1): s.e. 0.06 and 0.04
            assert not _same(a[k], b[k])
    vec.close()
