"""The closed regime on the MI355X (run with -m gpu): qd_eval_points_closed and qd_scan_grid_closed against the host build of
the same source (kept states, bit for bit) and the reference of tests/closed_helpers.py (occupations, signal), the
conservation of the total charge, the classical limit, isolation from everything else the handle does, closed grids against
closed points, the facade's shapes and the refusals.

R = 16, B = 2: env 0 is queried, env 1 is a sampled neighbour.  A case is six groups of the same 300 points on env 0 at the
total charges {0, 1, Qs - 1, Qs, Qs + 1, 2N + 1}, Qs the rounded median over the points of the open oracle's total; at N = 2 a
slot holds 256 points, so every group crosses a slot boundary."""
import ctypes

import numpy as np
import pytest
import yaml

import closed_helpers as CH
import grid_helpers as GH
import helpers as H
import points_helpers as PH
import scan_helpers as SH
from qadapt_hip import device_model as DM
from qadapt_hip.layout import layout

pytestmark = pytest.mark.gpu

R, B, NPTS = 16, 2, 300
CASES = [(2, 32), (3, 32), (5, 32), (8, 32), (5, 16), (5, 8), (5, 5)]
_CASES = {}


def _cfg(tmp_path, **sim):
    cfg = DM.load_yaml(None, "env_config.yaml")
    cfg["capacitance_model"]["update_method"] = None          # deterministic physics, no CNN in the loop
    cfg["simulator"].update(sim)
    p = tmp_path / "env.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def _vec(tmp_path, N, seed, nb=B, **kw):
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    if "config_path" not in kw:
        kw["config_path"] = _cfg(tmp_path)
    return VecQuantumDeviceEnv(nb, num_dots=N, resolution=R, seed=seed, **kw)


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def _snapshot(env):
    st, steps = env.get_state()
    raw, plohi = env.raw()
    return dict(state=st.copy(), steps=steps.copy(), raw=raw.copy(), plohi=plohi.copy())


def _kc(K):
    return 8 if K <= 8 else (16 if K <= 16 else 32)


def _case(tmp_path, N, K):
    """One case, run once for its tests: the device results of the six groups together, of group 3 alone, the handle's raw
    signal and state before and after, the host build's lists and the reference."""
    if (N, K) not in _CASES:
        seed = 6100 + 10 * N + K
        env = _vec(tmp_path, N, seed, num_charge_states=K)
        env.reset(seed=seed)
        par = env._params_host[0].copy()
        dev = H.dev_view(N, par)
        vg, vb = CH.points(N, np.random.default_rng(seed + 1), NPTS)
        totals, _ = CH.open_totals(dev, vg, vb)
        Qv = CH.q_values(N, int(np.rint(np.median(totals))))
        before = _snapshot(env)
        out = env.eval_points([0] * 6, np.tile(vg, (6, 1, 1)), np.tile(vb, (6, 1, 1)), n_charge=Qv, states=True)
        alone = env.eval_points([0], vg[None], vb[None], n_charge=Qv[3], states=True)
        after = _snapshot(env)
        env.close()
        vg6, vb6 = np.tile(vg, (6, 1)), np.tile(vb, (6, 1))
        Q6 = np.repeat(np.array(Qv), NPTS)
        host = CH.host_closed(N, par, np.concatenate([vg6, vb6], axis=1), Q6, _kc(K))
        occ_ref, gap = CH.occupations_ref(dev, vg6, vb6, host["states"], host["nvalid"], K)
        sig_ref = CH.signal_ref(dev, vg6, vb6, occ_ref)
        _CASES[(N, K)] = dict(Qv=Qv, Q6=Q6, host=host, occ_ref=occ_ref, gap=gap, sig_ref=sig_ref, before=before, after=after,
                              out={k: _np(v) for k, v in out.items()}, alone={k: _np(v) for k, v in alone.items()})
    return _CASES[(N, K)]


@pytest.mark.parametrize("N,K", CASES)
def test_kept_states_are_the_host_lists(tmp_path, N, K):
    c = _case(tmp_path, N, K)
    st = c["out"]["states"]
    assert st.shape == (6, NPTS, K, N) and st.dtype == np.int32
    want = c["host"]["states"][:, :K].reshape(6, NPTS, K, N)
    nd = int((st != want).any(axis=(2, 3)).sum())
    print(f"[closed states] N={N} K={K} Q={c['Qv']}: points whose list differs {nd} of {6 * NPTS}; candidates found "
          f"{int(c['host']['nvalid'].min())}..{int(c['host']['nvalid'].max())}")
    assert np.array_equal(st, want), nd
    # zeros behind the candidates found, every kept state in the sector
    nv = np.minimum(c["host"]["nvalid"], K).reshape(6, NPTS)
    slot = np.arange(K)[None, None, :]
    assert np.all(st[slot >= nv[:, :, None]] == 0)
    sums = st.sum(axis=3)
    assert np.all(sums[slot < nv[:, :, None]] == np.broadcast_to(c["Q6"].reshape(6, NPTS, 1), sums.shape)[slot < nv[:, :, None]])


@pytest.mark.parametrize("N,K", CASES)
def test_occupations_signal_and_total_charge(tmp_path, N, K):
    """Occupations within 1e-6 of the reference wherever its relative gap is above GAP_MIN (at most 5 % of a case exempt), the
    signal within 1e-6 relative there, and |sum(occ) - Q| <= 1e-9 at EVERY point: the open path cannot pass that."""
    c = _case(tmp_path, N, K)
    occ, sig = c["out"]["occupations"].reshape(-1, N), c["out"]["signal"].reshape(-1)
    assert np.isfinite(occ).all() and np.isfinite(sig).all()
    ok = c["gap"] > H.GAP_MIN
    d_occ = np.abs(occ - c["occ_ref"]).max(axis=1)
    d_sig = np.abs(sig - c["sig_ref"]) / np.maximum(np.abs(c["sig_ref"]), 1e-3)
    d_tot = np.abs(occ.sum(axis=1) - c["Q6"])
    print(f"[closed vs reference] N={N} K={K}: worst occupation {d_occ[ok].max():.3e}, worst signal {d_sig[ok].max():.3e}, "
          f"worst |sum(occ) - Q| {d_tot.max():.3e}, exempt {int((~ok).sum())} of {len(ok)}")
    assert (~ok).sum() <= 0.05 * len(ok)
    assert np.all(d_occ[ok] <= 1e-6) and np.all(d_sig[ok] <= 1e-6)
    assert np.all(d_tot <= 1e-9), float(d_tot.max())


@pytest.mark.parametrize("N,K", CASES)
def test_a_group_alone_and_the_handle_untouched(tmp_path, N, K):
    c = _case(tmp_path, N, K)
    for key in ("signal", "occupations", "states"):
        assert PH.same(c["alone"][key][0], c["out"][key][3]), key
    for key in c["before"]:
        assert PH.same(c["before"][key], c["after"][key]), key


def test_classical_limit(tmp_path):
    """tc_base = 0 on env 0: the Hamiltonian is diagonal, the occupations are the integers of the first kept state, and at
    Q = the open oracle's total that state is the open ground state."""
    N, K, seed = 5, 32, 6400
    L = layout(N)
    env = _vec(tmp_path, N, seed, num_charge_states=K)
    env.reset(seed=seed)
    params = env._params_host.copy()
    params[0, L.scal] = 0.0
    st, _ = env.get_state()
    ids = np.arange(B, dtype=np.int32)
    from qadapt_hip import _lib
    rc = env._lib.qd_load_episodes(env._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), B, np.ascontiguousarray(params).ctypes.data,
                                   np.ascontiguousarray(st).ctypes.data, 0, env._stream())
    _lib.check(env._h, rc, "qd_load_episodes")
    dev = H.dev_view(N, params[0])
    vg, vb = CH.points(N, np.random.default_rng(seed + 1), 90)
    totals, n_open = CH.open_totals(dev, vg, vb)
    qs = sorted(set(totals.tolist()))
    sel = [np.nonzero(totals == q)[0] for q in qs]
    out = env.eval_points([0] * len(qs), [vg[s] for s in sel], [vb[s] for s in sel], n_charge=qs, states=True)
    for s, occ, kept in zip(sel, out["occupations"], out["states"]):
        occ, kept = _np(occ), _np(kept)
        assert np.array_equal(occ, kept[:, 0].astype(np.float64))
        assert np.array_equal(occ, n_open[s])
    env.close()


def test_closed_calls_leave_no_footprint_on_steps(tmp_path):
    """Two handles of one seed, one of them interleaved with closed points and closed grids: raw(), state and the
    observations of both envs stay the same bits through a reset and two steps."""
    import torch
    N, seed = 4, 6500
    plain, poked = _vec(tmp_path, N, seed), _vec(tmp_path, N, seed)
    rng = np.random.default_rng(3)

    def poke():
        vg, vb = CH.points(N, rng, 70)
        o = poked.eval_points([1, 0], np.stack([vg, vg]), np.stack([vb, vb]), n_charge=[2, 3], states=True)
        g = poked.scan_grid_closed([0, 1], "P1", "P2", (-1.0, 3.0), (-1.0, 3.0), 9, 5, np.zeros((2, N)), np.zeros((2, N - 1)), [1, 4],
                                   frame="physical", occupations=True)
        assert np.isfinite(_np(o["signal"])).all() and np.isfinite(_np(g["raw"])).all()

    def snap(env, obs):
        d = _snapshot(env)
        d.update({k: _np(obs[k]).copy() for k in ("image", "obs_gate_voltages", "obs_barrier_voltages")})
        return d

    acts = np.random.default_rng(4).uniform(-1, 1, (2, B, 2 * N - 1)).astype(np.float32)
    trace = [[], []]
    for k, env in enumerate((plain, poked)):
        trace[k].append(snap(env, env.reset(seed=seed)))
    poke()
    for t in range(2):
        for k, env in enumerate((plain, poked)):
            obs = env.step(torch.as_tensor(acts[t]).cuda())[0]
            trace[k].append(snap(env, obs))
        poke()
    for a, b in zip(*trace):
        for key in a:
            assert PH.same(a[key], b[key]), key
    plain.close(); poked.close()


@pytest.mark.parametrize("N,K", [(4, 32), (2, 32), (5, 5)])
def test_closed_grids_equal_closed_points(tmp_path, N, K):
    """Physical frame, 24 x 8, 64 x 1 and 16 x 16 on R = 16 (a tail of 4 inert records, a line, the whole slot): occupations and
    raw signal of a closed grid are the bits of closed points at the voltages of the host front end (grid_helpers.grid_voltages),
    two queries with different total charges per call."""
    from qadapt_hip.vec_env import scan_axis_vector as vec
    G, seed = N + 1, 6600 + 10 * N + K
    env = _vec(tmp_path, N, seed, num_charge_states=K)
    env.reset(seed=seed)
    st, _ = env.get_state()
    rng = np.random.default_rng(seed)
    x, y = "P1", {"P2": 1.0, "B1": -0.5}
    for nx, ny in ((24, 8), (64, 1), (16, 16)):
        W0 = np.concatenate([rng.uniform(0.0, 2.5, G), rng.uniform(-1.0, 1.0, N - 1)])
        rgx, rgy = (-1.5, 2.0), (1.0, -1.0)
        Qv = [int(rng.integers(1, N + 2)), 2 * N]
        out = env.scan_grid_closed([0, 0], x, y, rgx, rgy, nx, ny, np.tile(W0[:N], (2, 1)), np.tile(W0[G:], (2, 1)), Qv,
                                   sensor_voltage=W0[N], frame="physical", occupations=True)
        qst = SH.query_state(N, st[0], W0[:N], W0[G:], float(W0[N]))
        v_ext, _, _ = GH.grid_voltages(N, env._params_host[0], qst, vec(x, N, "physical"), vec(y, N, "physical"), [*rgx, *rgy], nx, ny,
                                       GH.PHYSICAL)
        pts = env.eval_points([0, 0], np.stack([v_ext[:, :G]] * 2), np.stack([v_ext[:, G:]] * 2), n_charge=Qv)
        raw, occ = _np(out["raw"]), _np(out["occupations"])
        sig, occ_p = _np(pts["signal"]).reshape(2, ny, nx), _np(pts["occupations"]).reshape(2, ny, nx, N)
        assert raw.shape == (2, ny, nx) and occ.shape == (2, ny, nx, N) and np.isfinite(raw).all()
        assert PH.same(raw, sig), (nx, ny, float(np.abs(raw - sig).max()))
        assert PH.same(occ, occ_p), (nx, ny, float(np.abs(occ - occ_p).max()))
        assert np.all(np.abs(occ.sum(axis=3) - np.array(Qv)[:, None, None]) <= 1e-9)
        assert not PH.same(raw[0], raw[1])
    env.close()


def test_facade_do1d_and_do2d_closed(tmp_path):
    from qadapt_hip.env import QuantumDeviceEnv
    N = 3
    path = _cfg(tmp_path, num_dots=N, resolution=R)
    env = QuantumDeviceEnv(config_path=path, num_dots=N, backend=_vec(tmp_path, N, 6700, nb=1, config_path=path))
    model = env.array.model
    sig, n = model.do1d_closed("P1", -1.0, 3.0, 33, 2)
    assert sig.shape == (33, 1) and n.shape == (33, N) and sig.dtype == n.dtype == np.float64
    assert np.all(np.abs(n.sum(axis=1) - 2) <= 1e-9)
    sig, n = model.do2d_closed("vP1", -2.0, 2.0, 12, "e1_2", -1.0, 1.0, 7, 3)
    assert sig.shape == (7, 12, 1) and n.shape == (7, 12, N) and np.all(np.abs(n.sum(axis=2) - 3) <= 1e-9)
    vg, vb = CH.points(N, np.random.default_rng(5), 6)
    sig, n = model.charge_sensor_closed(vg, 1, vb)
    assert sig.shape == (6, 1) and np.array_equal(model.ground_state_closed(vg, 1, vb), n) and np.all(np.abs(n.sum(axis=1) - 1) <= 1e-9)
    env.close()


def test_refusals_on_the_device(tmp_path):
    import torch
    from qadapt_hip import _lib
    N = 3
    q = DM.load_yaml(None, "qarray_config.yaml")
    q["simulator"]["model"]["max_charge_carriers"] = 2
    qp = tmp_path / "qarray_m2.yaml"
    qp.write_text(yaml.safe_dump(q))
    zg, zb = np.zeros((1, 4, N + 1)), np.zeros((1, 4, N - 1))
    for kw, word in ((dict(validate=True), "QD_FLAG_VALIDATE"),
                     (dict(num_charge_states="all", qarray_config_path=str(qp)), "full charge-state space")):
        env = _vec(tmp_path, N, 77, nb=1, **kw)
        env.reset(seed=77)
        raw0 = env.raw()[0].copy()
        with pytest.raises(_lib.QdError, match=word) as ei:
            env.eval_points([0], zg, zb, n_charge=2)
        assert f"code {_lib.QD_ERR_STATE}" in str(ei.value)
        with pytest.raises(_lib.QdError, match=word) as ei:
            env.scan_grid_closed([0], "P1", "P2", (0.0, 1.0), (0.0, 1.0), 4, 4, np.zeros((1, N)), np.zeros((1, N - 1)), 2, frame="physical")
        assert f"code {_lib.QD_ERR_STATE}" in str(ei.value)
        assert PH.same(env.raw()[0], raw0)
        env.close()
    env = _vec(tmp_path, N, 78, nb=1)
    env.reset(seed=78)
    for bad in (-1, 32768, 2.5, [1, 2]):
        with pytest.raises(ValueError):
            env.eval_points([0], zg, zb, n_charge=bad)
        with pytest.raises(ValueError):
            env.scan_grid_closed([0], "P1", "P2", (0.0, 1.0), (0.0, 1.0), 4, 4, np.zeros((1, N)), np.zeros((1, N - 1)), bad, frame="physical")
    with pytest.raises(ValueError, match="states"):
        env.eval_points([0], zg, zb, states=True)
    with pytest.raises(ValueError):
        env.scan_grid_closed([0], "P1", "P2", (0.0, 1.0), (0.0, 1.0), 4, 4, np.zeros((1, N)), np.zeros((1, N - 1)), None)
    # the C calls themselves: a total charge out of range in device memory, and a noise stage
    dev = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt).cuda()          # noqa: E731
    ids, dr, rg = dev([0, 0], torch.int32), dev(np.eye(2 * N)[:2][None].repeat(2, 0), torch.float64), dev([[0, 1, 0, 1]] * 2, torch.float64)
    gv, bv = dev(np.zeros((2, N)), torch.float64), dev(np.zeros((2, N - 1)), torch.float64)
    raw = torch.full((2, 4, 4), -7.0, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                  # noqa: E731
    opts = _lib.QdScanGridOpts(struct_size=ctypes.sizeof(_lib.QdScanGridOpts), frame=_lib.QD_SCAN_PHYSICAL)
    for qbad in ([2, 40000], [-1, 2]):
        qd = dev(qbad, torch.int32)
        rc = env._lib.qd_scan_grid_closed(env._h, p(ids), 2, 4, 4, p(dr), p(rg), p(gv), p(bv), None, p(qd), p(raw), None, None,
                                          ctypes.byref(opts), env._stream())
        assert rc == _lib.QD_ERR_ARG and b"0..32767" in env._lib.qd_last_error(env._h)
    qd = dev([2, 3], torch.int32)
    opts.noise_flags = _lib.QD_NOISE_LATCH
    rc = env._lib.qd_scan_grid_closed(env._h, p(ids), 2, 4, 4, p(dr), p(rg), p(gv), p(bv), None, p(qd), p(raw), None, None,
                                      ctypes.byref(opts), env._stream())
    assert rc == _lib.QD_ERR_ARG and b"no noise stages" in env._lib.qd_last_error(env._h)
    assert bool((raw == -7.0).all())
    opts.noise_flags = 0
    rc = env._lib.qd_scan_grid_closed(env._h, p(ids), 2, 4, 4, p(dr), p(rg), p(gv), p(bv), None, p(qd), p(raw), None, None,
                                      ctypes.byref(opts), env._stream())
    assert rc == 0 and bool(torch.isfinite(raw).all()) and not bool((raw == -7.0).any())
    env.close()
