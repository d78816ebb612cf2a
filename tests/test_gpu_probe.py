"""Probe scans on the MI355X (run with -m gpu): qd_probe against the set_state + observe route bit for bit, its absent
footprint on a noisy auto-resetting run, the oracle at the probe's voltages, qd_probe_compose against NumPy, the
device-range maps, and the refusals."""
import ctypes
import types

import numpy as np
import pytest
import yaml

import helpers as H
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


def _qpath(tmp_path, m):
    q = DM.load_yaml(None, "qarray_config.yaml")
    q["simulator"]["model"]["max_charge_carriers"] = m
    p = tmp_path / f"qarray_m{m}.yaml"
    p.write_text(yaml.safe_dump(q))
    return str(p)


def _vec(tmp_path, B, N, R, seed, **kw):
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    if "config_path" not in kw:                     # (not setdefault: _cfg writes the file, and would overwrite a given one)
        kw["config_path"] = _cfg(tmp_path)
    return VecQuantumDeviceEnv(B, num_dots=N, resolution=R, seed=seed, **kw)


def _bits(a):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _queries(L, params, state, rng, gate_off=35.0):
    """Per env one query as the dataset generator draws them: gates up to +-gate_off off the ground truth, barriers
    inside their range, a sensor voltage, the env's own window."""
    n, N, nb = params.shape[0], L.N, L.N - 1
    gv = state[:, L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-gate_off, gate_off, (n, N))
    bv = state[:, L.s_barrier_gt:L.s_barrier_gt + nb] + rng.uniform(-3.0, 3.0, (n, nb))
    sv = state[:, L.s_sensor_gt] + rng.uniform(-0.3, 0.3, n)
    return gv, bv, sv, params[:, L.scal + 2].copy()


# ------------------------------------------------------------------ 1. same bits as the existing path
def _old_route(env, params, st, steps):
    """The parent's only route: upload parameter blocks (a changed window lives there) and state blocks, observe, and
    read the signal back."""
    ids = np.arange(env.B, dtype=np.int32)
    from qadapt_hip import _lib
    rc = env._lib.qd_load_episodes(env._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), env.B,
                                   np.ascontiguousarray(params).ctypes.data, np.ascontiguousarray(st).ctypes.data, 0,
                                   env._stream())
    _lib.check(env._h, rc, "qd_load_episodes")
    env.set_state(st, steps)
    obs = env.observe()
    raw, plohi = env.raw()
    return raw.copy(), plohi.copy(), obs["image"].cpu().numpy().copy()


@pytest.mark.parametrize("N,R,K,m", [(4, 64, 32, None), (8, 64, 32, None), (3, 64, "all", 4)])
def test_probe_has_the_bits_of_set_state_and_observe(tmp_path, N, R, K, m):
    B, seed = 4, 9100 + N
    kw = dict(num_charge_states=K)
    if m is not None:
        kw["qarray_config_path"] = _qpath(tmp_path, m)
    old, new = _vec(tmp_path, B, N, R, seed, **kw), _vec(tmp_path, B, N, R, seed, **kw)
    L = layout(N); G = N + 1
    rng = np.random.default_rng(77 + N)
    for env in (old, new):
        env.load_new_devices(seed=seed)
    st0, steps0 = new.get_state()
    st0[:, L.s_vgm:L.s_vgm + G * G] += np.random.default_rng(5).normal(0, 0.05, (B, G * G))   # a VGM that is not the identity
    new.set_state(st0, steps0)
    params = new._params_host.copy()
    assert np.array_equal(params, old._params_host)
    gv, bv, sv, win = _queries(L, params, st0, rng)
    win[1] = win[1] * 0.6 + 0.4                                  # one query with a window that is not its env's own
    assert win[1] != params[1, L.scal + 2]
    sv[2] = 0.0
    # old route: the query's voltages in the state block, its window in the parameter block
    st = st0.copy()
    st[:, L.s_gate_v:L.s_gate_v + N] = gv
    st[:, L.s_barrier_v:L.s_barrier_v + N - 1] = bv
    st[:, L.s_sensor_gt] = sv
    par = params.copy(); par[:, L.scal + 2] = win
    raw_a, plohi_a, img_a = _old_route(old, par, st, steps0)
    raw_b, plohi_b, img_b = _old_route(old, par, st, steps0)
    assert _same(raw_a, raw_b) and _same(plohi_a, plohi_b) and _same(img_a, img_b), "the old route differs from itself"
    assert np.isfinite(raw_a).all() and np.ptp(raw_a) > 0
    # probe on the untouched handle
    out = new.probe(np.arange(B), gv, bv, sensor_voltage=sv, window=win, normalised=True)
    assert out["raw"].shape == (B, N - 1, R, R) and out["image"].shape == (B, R, R, N - 1)
    assert _same(out["raw"].reshape(B, N - 1, R * R), raw_a)
    assert _same(out["plohi"], plohi_a)
    assert _same(out["image"], img_a)
    # window=None takes each env's own window; sensor_voltage=None is 0.0: queries 0 and 2 with their own window
    par2 = params.copy(); st2 = st.copy(); st2[:, L.s_sensor_gt] = 0.0
    raw_c, _, _ = _old_route(old, par2, st2, steps0)
    out2 = new.probe([0, 2], gv[[0, 2]], bv[[0, 2]])
    assert _same(out2["raw"].reshape(2, N - 1, R * R), raw_c[[0, 2]])
    # and the probed handle's own state is as it was
    st1, steps1 = new.get_state()
    assert _same(st1, st0) and np.array_equal(steps1, steps0)
    old.close(); new.close()


# ------------------------------------------------------------------ 2. no footprint
@pytest.mark.parametrize("R,env_chunk", [(16, 0), (16, 2), (32, 2)])
def test_probes_leave_no_footprint_on_a_noisy_run(tmp_path, R, env_chunk):
    """env_chunk = 2: an observe of the B = 5 envs runs three chunks over the two launch lanes, and the probes (13, 1 or 5
    queries) run between them in chunks of 2 on lane 0's scratch.  R = 32 has the tile search and its redo pass (N = 4)."""
    import torch
    N, B, seed, max_steps = 4, 5, 31337, 3
    path = _cfg(tmp_path, max_steps=max_steps)
    mk = lambda chunk: _vec(tmp_path, B, N, R, seed, config_path=path, noise=("sensor", "radial", "latch"), env_chunk=chunk)
    envs = [mk(env_chunk) for _ in range(2)]
    if env_chunk:
        assert all(env.chunk_envs() == env_chunk for env in envs)
    plain, probed = envs
    L = layout(N)
    prng = np.random.default_rng(3)
    calls = [0]

    def poke():
        nq = (2 * B + 3, 1, B)[calls[0] % 3]                      # nq > B, a single query, nq == B
        calls[0] += 1
        ids = prng.integers(0, B, nq)                             # repeated env ids
        par = probed._params_host[ids]                            # anywhere in each device's action ranges
        gv = par[:, L.pmin:L.pmin + N] + (par[:, L.pmax:L.pmax + N] - par[:, L.pmin:L.pmin + N]) * prng.random((nq, N))
        bv = par[:, L.bmin:L.bmin + N - 1] + (par[:, L.bmax:L.bmax + N - 1] - par[:, L.bmin:L.bmin + N - 1]) * prng.random((nq, N - 1))
        win = None if calls[0] % 2 else prng.uniform(0.8, 2.0, nq)
        out = probed.probe(ids, gv, bv, sensor_voltage=prng.uniform(-0.2, 0.2, nq), window=win, normalised=True)
        assert np.isfinite(out["raw"].cpu().numpy()).all()

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

    trace = [[], []]
    for k, env in enumerate(envs):
        trace[k].append(snapshot(env, env.reset(seed=seed)))
    if env_chunk:
        # the lanes do not change the result: one launch of all B envs renders the same bits, noise included
        one = mk(B)
        assert one.chunk_envs() == B
        first = snapshot(one, one.reset(seed=seed))
        assert first.keys() == trace[0][0].keys()
        for key in first:
            assert _same(first[key], trace[0][0][key]), key
        one.close()
    poke()
    acts = np.random.default_rng(11).uniform(-1, 1, (6, B, 2 * N - 1)).astype(np.float32)
    truncations = 0
    for t in range(6):
        for k, env in enumerate(envs):
            obs, rew, term, trunc = env.step(torch.as_tensor(acts[t]).cuda(), auto_reset=True)
            trace[k].append(snapshot(env, obs, rew, trunc))
        truncations += int(trace[0][-1]["trunc"].sum())
        poke(); poke()
    assert truncations >= B, "no truncation and reload fell inside the run"
    for a, b in zip(*trace):
        assert a.keys() == b.keys()
        for key in a:
            assert _same(a[key], b[key]), key
    for env in envs:
        env.close()


# ------------------------------------------------------------------ 3. against the oracle
ORACLE_CASES = [(2, 9311), (4, 9302), (6, 9303)]       # (dots, seed): on these the oracle alone excuses <= 1 % of each image
                                                       # (rel_gap <= GAP_MIN).  The count needs no GPU and is
                                                       # `_oracle_case(N, seed)[2][k].unres` for query k: 0 in all six images;
                                                       # the test asserts the condition before it renders anything.  Many 2-dot seeds fail the condition: +-10 V off the
                                                       # ground truth often empties both dots, and the ground state is then one
                                                       # of several identical |0 0> padding states (gap exactly 0)


def _oracle_case(N, seed, B=2, R=16):
    """Devices of a VecQuantumDeviceEnv(B, seed=seed) as its constructor samples them, and one query per env (+-10 V off
    the ground truth, own sensor voltage and window): parameter / state rows, query arrays and per query the oracle's
    raw image and its count of pixels the float64 ground vector does not resolve."""
    q, e = H.configs()
    s = DM.DeviceSampler(N, q, e)
    eb = s.build(np.stack([np.random.Generator(np.random.PCG64(seed + k)).random(s.n_draws) for k in range(B)]))
    L = layout(N)
    rng = np.random.default_rng(seed)
    gv, bv, sv, _ = _queries(L, eb.params, eb.state, rng, gate_off=10.0)
    win = rng.uniform(1.0, 2.5, B)
    views = []
    for k in range(B):
        dev, st = H.dev_view(N, eb.params[k]), H.state_view(N, eb.state[k])
        img = O.get_obs_images(dev, st.vgm, dev.origin, gv[k], bv[k], sv[k], win[k], R)
        unres = sum(int((H.pixel_spectrum(dev, st.vgm, dev.origin, gv[k], sv[k], bv[k], win[k], ch, R)["rel_gap"]
                         <= H.GAP_MIN).sum()) for ch in range(N - 1))
        views.append(types.SimpleNamespace(N=N, R=R, raw_image=img, dev=dev, vgm_at_obs=st.vgm, origin=dev.origin,
                                           gate_v=gv[k], sensor_gt=sv[k], barrier_v=bv[k], window=win[k], unres=unres))
    return eb, (gv, bv, sv, win), views


@pytest.mark.parametrize("N,seed", ORACLE_CASES)
def test_probe_matches_the_oracle(tmp_path, N, seed):
    B, R = 2, 16
    eb, (gv, bv, sv, win), views = _oracle_case(N, seed, B, R)
    for v in views:                                            # the cap is a condition on the case, not a measurement
        assert v.unres <= 0.01 * R * R * (N - 1), (N, seed, v.unres)
    env = _vec(tmp_path, B, N, R, seed)
    env.reset(seed=seed)
    assert np.array_equal(env._params_host, eb.params)
    out = env.probe(np.arange(B), gv, bv, sensor_voltage=sv, window=win, normalised=True)
    raw = out["raw"].cpu().numpy().reshape(B, N - 1, R * R); img = out["image"].cpu().numpy()
    for k, v in enumerate(views):
        # raw within 1e-6 wherever rel_gap > GAP_MIN, the normalised image within the observation tolerance everywhere
        worst, unres = H.image_parity(v, img[k], raw[k])
        print(f"N={N} query {k}: worst image difference {worst:.3e}, unresolved pixels {unres}")
        assert unres == v.unres
    env.close()


# ------------------------------------------------------------------ 4. compose
def _np_compose(scans, nx, ny, R, mode):
    """The scripts' stitching on (nx*ny, R, R) float64 scans: (composite float64, percentiles)."""
    if mode == "global":                                       # map_full_device_range.py:168-194
        comp = np.zeros((R * ny, R * nx))
        for idx, scan in enumerate(scans):
            i, j = idx // ny, idx % ny
            comp[j * R:(j + 1) * R, i * R:(i + 1) * R] = scan
        p_low, p_high = np.percentile(comp, 0.5), np.percentile(comp, 99.5)
        norm = (comp - p_low) / (p_high - p_low) if p_high > p_low else np.zeros_like(comp)
        return np.clip(norm, 0, 1), np.array([p_low, p_high])
    rows = [[None] * nx for _ in range(ny)]                    # map_device_range.py:134-170
    pl = []
    for idx, scan in enumerate(scans):
        p_low, p_high = np.percentile(scan, 0.5), np.percentile(scan, 99.5)
        pl.append((p_low, p_high))
        norm = (scan - p_low) / (p_high - p_low) if p_high > p_low else np.zeros_like(scan)
        rows[ny - 1 - idx % ny][idx // ny] = np.clip(norm, 0, 1)
    return np.vstack([np.hstack(r) for r in rows]), np.array(pl)


def _check_compose(env, raw, nx, ny, channel):
    R = env.R
    scans = raw.cpu().numpy()[:, channel]
    for mode in ("global", "per_scan"):
        comp, plohi = env.compose(raw, nx, ny, channel=channel, mode=mode)
        ref, ref_pl = _np_compose(scans, nx, ny, R, mode)
        assert _same(plohi, ref_pl), (mode, plohi.cpu().numpy(), ref_pl)          # bit-equal to np.percentile
        comp = comp.cpu().numpy()
        assert comp.shape == (ny * R, nx * R) and comp.dtype == np.float32
        ref32 = ref.astype(np.float32)
        assert np.all(np.abs(comp - ref32) <= np.spacing(ref32)), mode              # within 1 ulp of float32


@pytest.mark.parametrize("nx,ny,R", [(3, 2, 16), (5, 5, 16), (3, 3, 64)])
def test_compose_equals_numpy(tmp_path, nx, ny, R):
    """(3, 3, 64): nx*ny*P = 36 864 > 32 * 1024, more than one block's cached keys."""
    N, seed = 4, 5150
    if R == 64:
        assert nx * ny * R * R > 32 * 1024
    env = _vec(tmp_path, 2, N, R, seed)
    env.reset(seed=seed)
    st, _ = env.get_state(); L = env.L
    gt = st[1, L.s_gate_gt:L.s_gate_gt + N]; bgt = st[1, L.s_barrier_gt:L.s_barrier_gt + N - 1]
    w = float(env._params_host[1, L.scal + 2])
    gates = np.tile(gt, (nx * ny, 1))
    for i in range(nx):
        for j in range(ny):
            gates[i * ny + j, 1] = gt[1] + (i - nx / 2) * 2 * w
            gates[i * ny + j, 2] = gt[2] + (j - ny / 2) * 2 * w
    raw = env.probe([1], gates, np.tile(bgt, (nx * ny, 1)))["raw"]
    _check_compose(env, raw, nx, ny, channel=1)
    if (nx, ny) == (3, 2):
        # p_hi <= p_lo: the zero image, in both modes
        flat = raw.clone(); flat[:] = 0.25
        for mode in ("global", "per_scan"):
            comp, plohi = env.compose(flat, nx, ny, channel=0, mode=mode)
            assert not comp.cpu().numpy().any() and np.all(plohi.cpu().numpy() == 0.25)
        # values that tie around the ranks, negative keys included
        rng = np.random.default_rng(1)
        tied = raw.clone()
        tied[:] = env._to_dev(rng.integers(-3, 4, tuple(raw.shape)).astype(np.float64) * 0.5, raw.dtype, tuple(raw.shape))
        _check_compose(env, tied, nx, ny, channel=2)
    env.close()


# ------------------------------------------------------------------ 5. maps
def test_full_device_range_map(tmp_path):
    from qadapt_hip import device_map as M
    from qadapt_hip.env import QuantumDeviceEnv
    N, R, seed = 4, 16, 808
    vec = _vec(tmp_path, 1, N, R, seed)
    env = QuantumDeviceEnv(config_path=_cfg(tmp_path, num_dots=N, resolution=R), backend=vec)
    L = vec.L
    gt = env.device_state["gate_ground_truth"].astype(np.float64)
    w = float(vec._params_host[0, L.scal + 2])
    assert env.array.obs_voltage_max == w and env.array.obs_voltage_min == -w
    v0 = (gt[0] - 3.3 * w * 2, gt[0] + 0.6 * w * 2); v1 = (gt[1] - 1.2 * w * 2, gt[1] + 2.7 * w * 2)     # 4 x 4 tiles
    st_before, steps_before = vec.get_state()
    m = M.map_full_device_range(vec, 0, 0, v0_min=v0[0], v0_max=v0[1], v1_min=v1[0], v1_max=v1[1])
    nx, ny = m["n_scans_x"], m["n_scans_y"]
    assert (nx, ny) == (4, 4)
    plan = M.tile_plan_full_range(np.array([v0[0], v1[0]]), np.array([v0[1], v1[1]]), 2 * w)
    assert m["positions"] == plan["positions"] and _same(m["centres"], plan["centres"])
    assert m["extent"][0] <= gt[0] <= m["extent"][1] and m["extent"][2] <= gt[1] <= m["extent"][3]
    assert min(p[0] for p in m["positions"]) <= gt[0] <= max(p[1] for p in m["positions"])
    assert min(p[2] for p in m["positions"]) <= gt[1] <= max(p[3] for p in m["positions"])
    scans = m["scans"].cpu().numpy()
    assert scans.shape == (nx * ny, R, R) and m["composite"].shape == (ny * R, nx * R)
    bgt = env.device_state["barrier_ground_truth"].astype(np.float64)
    for i in range(nx):
        for j in range(ny):
            g = gt.copy(); g[0], g[1] = plan["centres"][i * ny + j]
            one = env.array._get_obs(g, bgt)["image"]
            assert _same(one[:, :, 0], scans[i * ny + j]), (i, j)
    ref, ref_pl = _np_compose(scans, nx, ny, R, "global")
    assert _same(m["plohi"], ref_pl)
    comp = m["composite"].cpu().numpy()
    assert np.all(np.abs(comp - ref.astype(np.float32)) <= np.spacing(ref.astype(np.float32)))
    # the centred map: per-scan normalisation, flipped row blocks, ground truth in the middle of the extent
    c = M.map_device_range(vec, 0, 1, half_range=4.0, window_size=3.0)
    assert (c["n_scans_x"], c["n_scans_y"]) == (3, 3)
    assert c["positions"] == M.tile_plan_centred(gt[1], gt[2], 4.0, 3.0)["positions"]
    ref, ref_pl = _np_compose(c["scans"].cpu().numpy(), 3, 3, R, "per_scan")
    assert _same(c["plohi"], ref_pl)
    assert np.all(np.abs(c["composite"].cpu().numpy() - ref.astype(np.float32)) <= np.spacing(ref.astype(np.float32)))
    assert c["extent"][0] < gt[1] < c["extent"][1] and c["extent"][2] < gt[2] < c["extent"][3]
    p = M.save_npz(str(tmp_path / "map.npz"), m)
    with np.load(p) as z:
        assert z["composite"].shape == comp.shape and int(z["n_scans_x"]) == nx
    st_after, steps_after = vec.get_state()
    assert _same(st_before, st_after) and np.array_equal(steps_before, steps_after)
    env.close()


# ------------------------------------------------------------------ 6. refusals
def test_probe_refusals(tmp_path):
    import torch
    from qadapt_hip import _lib
    N, R, B, seed = 4, 16, 2, 66
    val = _vec(tmp_path, B, N, R, seed, validate=True)
    val.reset(seed=seed)
    with pytest.raises(_lib.QdError, match=r"code 3.*QD_FLAG_VALIDATE"):
        val.probe([0], np.zeros((1, N)), np.zeros((1, N - 1)))
    val.close()
    env = _vec(tmp_path, B, N, R, seed)
    env.reset(seed=seed)
    ids = torch.tensor([1, B, 0, -1], dtype=torch.int32).cuda()            # B and -1 are out of range
    gv = torch.zeros((4, N), dtype=torch.float64).cuda(); bv = torch.full((4, N - 1), 4.0, dtype=torch.float64).cuda()
    raw = torch.full((4, N - 1, R, R), -7.0, dtype=torch.float64).cuda()
    img = torch.full((4, R, R, N - 1), -7.0, dtype=torch.float32).cuda()
    pl = torch.full((4, 2), -7.0, dtype=torch.float64).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())                               # noqa: E731
    rc = env._lib.qd_probe(env._h, p(ids), 4, p(gv), p(bv), None, None, p(raw), p(img), p(pl), env._stream())
    assert rc == 0
    raw, img, pl = raw.cpu().numpy(), img.cpu().numpy(), pl.cpu().numpy()
    for q in (1, 3):
        assert np.all(raw[q] == -7.0) and np.all(img[q] == -7.0) and np.all(pl[q] == -7.0)
    ref = env.probe([1, 0], np.zeros((2, N)), np.full((2, N - 1), 4.0), normalised=True)
    assert _same(raw[[0, 2]], ref["raw"]) and _same(img[[0, 2]], ref["image"]) and _same(pl[[0, 2]], ref["plohi"])
    env.close()
