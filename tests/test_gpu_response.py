"""The charge response per point on the MI355X (run with -m gpu): qd_eval_points_response / eval_points(kT=, response=True) against
the reference of tests/response_helpers.py -- the divided-difference formula on numpy.linalg.eigh of the oracle's Hamiltonian over
the kept list, Lam and Gam from the oracle device -- open and closed, at the kT of 100 K and of 1 K, on handles of 2 dots (a single
pair, 2N - 1 = 3), 4 dots at K = 8 and 8 dots at K = 32; the bits of the thermal outputs with and without the response; dS/dv
against the analytic derivative of the sensor expression at the reference occupations; couplings that are exactly zero (all of
them, and one among coupled pairs); the refusals; the facade.

Bounds (response_helpers): chi within 8 n_max^2 (1e-12 hs + 1e-13 hn) min(1/kT, 1/g)^2 + 1e-12 n_max^2 / kT (ln tc columns:
||T_d||_inf for one n_max), the jacobian through |Lam| and |Gam|, dS/dv through |S'| and the bound of S'' on the error of c0.  EVERY
point is compared.  Worst err / tol measured on an MI355X (also in DESIGN 7, "Charge response"): open chi 4.7e-4, jacobian 4.6e-4,
dsignal 2.2e-4 (8 dots, 100 K); closed chi 5.2e-4, jacobian 4.7e-4, dsignal 1.8e-4; symmetry 2.9e-4, largest eigenvalue 2.9e-4,
column sums of the closed lists 1.1e-4."""
import ctypes

import numpy as np
import pytest
import yaml

import closed_helpers as CH
import helpers as H
import points_helpers as PH
import qd_oracle as O
import response_helpers as RH
import thermal_helpers as TH
from qadapt_hip import device_model as DM
from qadapt_hip.layout import layout
from test_gpu_levels import SPANS, _cfg, _load, _np, _open_lists, _physical, _vec

pytestmark = pytest.mark.gpu

THERMAL = ("signal", "occupations", "variance", "ztail")
KTS = (("100 K", TH.KB_REF * 100), ("1 K", TH.KB_REF * 1))
HANDLES = [(2, 32), (4, 8), (8, 32)]


def _classical_ground(dev, vg, vb):
    """the charge state of lowest free energy among floor(n_cont) + {0, 1}^N per point (no tunnelling): which side of the
    transition lines the point is on"""
    N = dev.n_dot
    v_ext = np.concatenate([vg, vb], axis=1)
    base = np.floor(O.continuous_ground_state(v_ext, dev.cdd_inv_full, dev.cgd_full, N)).astype(np.int64)
    bits = (np.arange(2 ** N)[:, None] >> np.arange(N)[None, :]) & 1
    cand = np.maximum(base[:, None, :] + bits[None], 0)
    F = O.free_energy_states(v_ext, dev.cdd_inv_full, dev.cgd_full, cand, N)
    return cand[np.arange(len(F)), np.argmin(F, axis=1)]


def _onto_lines(dev, vg, vb, n=24):
    """points 0 .. n-1 are moved onto a charge-transition line: where the segment to point i + n changes its classical ground
    state, the crossing is bisected to 2^-40 of the segment"""
    vg, vb = vg.copy(), vb.copy()
    a_g, a_b, b_g, b_b = vg[:n], vb[:n], vg[n:2 * n], vb[n:2 * n]
    lo, hi = np.zeros(n), np.ones(n)
    g0 = _classical_ground(dev, a_g, a_b)
    cross = (g0 != _classical_ground(dev, b_g, b_b)).any(axis=1)
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        gm = _classical_ground(dev, a_g + mid[:, None] * (b_g - a_g), a_b + mid[:, None] * (b_b - a_b))
        same = (gm == g0).all(axis=1)
        lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
    t = np.where(cross, 0.5 * (lo + hi), 0.0)
    vg[:n] = a_g + t[:, None] * (b_g - a_g)
    vb[:n] = a_b + t[:, None] * (b_b - a_b)
    return vg, vb, int(cross.sum())


def _points(N, L, par, st, seed):
    """64 points around the device's own working point, wide enough to cross the transition lines of every dot; the first 24 are
    moved onto the line their segment to a partner crosses, where the response is the finite thermal peak"""
    rng = np.random.default_rng(seed)
    s, t = SPANS["mid"]
    vg = _physical(L, par, st, st[L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-s, s, (64, N)))
    vb = st[L.s_barrier_gt:L.s_barrier_gt + N - 1] + rng.uniform(-t, t, (64, N - 1))
    vg, vb, crossed = _onto_lines(H.dev_view(N, par), vg, vb)
    assert crossed >= 12
    return vg, vb


def _check(tag, dev, Hs, states, nv, tcs, kT, vg, vb, out, e, closed=False):
    chi, jac, ds = (_np(out[k][e]) for k in ("chi", "jacobian", "dsignal"))
    N = dev.n_dot
    assert chi.shape == (len(Hs), N, 2 * N - 1) and jac.shape == (len(Hs), N, 2 * N) and ds.shape == (len(Hs), 2 * N)
    assert np.isfinite(chi).all() and np.isfinite(jac).all() and np.isfinite(ds).all()
    return RH.compare_points(tag, dev, Hs, states, nv, tcs, kT, vg, vb, dev.gamma, chi, jac, ds, closed=closed)


# ------------------------------------------------------------------ 1. parity, open; the thermal outputs keep their bits
@pytest.mark.parametrize("N,K", HANDLES)
def test_open_parity_and_the_thermal_bits(tmp_path, N, K):
    L = layout(N)
    eb = H.sample_blocks(N, [41])
    par, st = eb.params[0], eb.state[0]
    assert par[L.scal + 4] == 0.0
    vg, vb = _points(N, L, par, st, 9800 + N)
    dev = H.dev_view(N, par)
    states, nv = _open_lists(dev, vg, vb, K)
    assert nv.min() >= 1
    Hs, tc = TH.hamiltonians(dev, vg, vb, states, nv)
    env = _vec(tmp_path, 1, N, 8, 41, num_charge_states=K)
    _load(env, eb.params, eb.state)
    worst, moved = 0.0, 0
    for name, kT in KTS:
        plain = env.eval_points([0], vg[None], vb[None], kT=kT, outputs=THERMAL)
        out = env.eval_points([0], vg[None], vb[None], kT=kT, outputs=THERMAL, response=True)
        assert set(out) == set(THERMAL) | {"chi", "jacobian", "dsignal"}
        for key in THERMAL:
            assert PH.same(plain[key], out[key]), (name, key)
        TH.compare_points(f"open N={N} K={K} {name}", Hs, states, nv, kT, _np(out["occupations"][0]), _np(out["variance"][0]),
                          _np(out["ztail"][0]))
        worst = max(worst, _check(f"open N={N} K={K} kT={kT:.2e} ({name})", dev, Hs, states, nv, tc, kT, vg, vb, out, 0))
        moved += int((np.abs(_np(out["chi"][0])).max(axis=(1, 2)) * kT > 1e-3).sum())
    assert moved >= 8, "too few points near a transition line among the 128"
    print(f"[response] open N={N} K={K}: worst err / tol {worst:.2e}; {moved} of 128 points with |chi| kT > 1e-3")
    env.close()


# ------------------------------------------------------------------ 2. parity, closed
@pytest.mark.parametrize("N,K", HANDLES)
def test_closed_parity(tmp_path, N, K):
    """a total charge in reach per env; the kept lists of the host build of the sector search; every column of chi sums to zero"""
    seed = 9850 + N
    env = _vec(tmp_path, 2, N, 8, seed, num_charge_states=K)
    env.reset(seed=seed)
    vg, vb = CH.points(N, np.random.default_rng(seed + 1), 64)
    Qv = [N, N + 1]
    worst = 0.0
    for name, kT in KTS:
        plain = env.eval_points([0, 1], np.stack([vg] * 2), np.stack([vb] * 2), n_charge=Qv, kT=kT, outputs=THERMAL)
        out = env.eval_points([0, 1], np.stack([vg] * 2), np.stack([vb] * 2), n_charge=Qv, kT=kT, outputs=THERMAL, response=True)
        for key in THERMAL:
            assert PH.same(plain[key], out[key]), (name, key)
        for e, Q in enumerate(Qv):
            par = env._params_host[e]
            assert par[layout(N).scal + 4] == 0.0
            host = CH.host_closed(N, par, np.concatenate([vg, vb], axis=1), Q, 8 if K <= 8 else (16 if K <= 16 else 32))
            nv = np.minimum(host["nvalid"], K)
            dev = H.dev_view(N, par)
            Hs, tc = TH.hamiltonians(dev, vg, vb, host["states"], nv)
            assert all(Hm is not None for Hm in Hs)                      # (a point without a valid state would be compared too)
            worst = max(worst, _check(f"closed N={N} K={K} Q={Q} ({name})", dev, Hs, host["states"], nv, tc, kT, vg, vb, out, e,
                                      closed=True))
    print(f"[response] closed N={N} K={K}: worst err / tol {worst:.2e}")
    env.close()


# ------------------------------------------------------------------ 2b. couplings that are exactly zero, on the device
def test_zero_couplings_give_zero_columns_and_the_covariance(tmp_path):
    """4 dots.  Handle A: tc_base = 0, every coupling exactly zero: the ln tc columns are exactly 0.0, chi[:, :N] = -cov / kT from
    the reference populations and its diagonal -var / kT from the device's own variance, to the tolerance.  Handle B: the same
    device with barrier 1 raised until exp(-alpha vb) underflows on half of the points: tc_1 == 0.0 among coupled pairs, and that
    column is exactly 0.0 (asserted in compare_points) while the others are compared as everywhere."""
    N, K = 4, 32
    L = layout(N)
    eb = H.sample_blocks(N, [41])
    st = eb.state[0]
    for cut in ("all", "one"):
        par = eb.params[0].copy()
        if cut == "all":
            par[L.scal] = 0.0
        vg, vb = _points(N, L, par, st, 9820)
        if cut == "one":
            vb[::2, 1] = 900.0 / par[L.alpha + 1]
        dev = H.dev_view(N, par)
        states, nv = _open_lists(dev, vg, vb, K)
        Hs, tc = TH.hamiltonians(dev, vg, vb, states, nv)
        assert (not tc.any()) if cut == "all" else (not tc[::2, 1].any() and tc[1::2, 1].all() and tc[:, 0].all() and tc[:, 2].all())
        env = _vec(tmp_path, 1, N, 8, 41, num_charge_states=K)
        _load(env, par[None], st[None])
        for name, kT in KTS:
            out = env.eval_points([0], vg[None], vb[None], kT=kT, outputs=THERMAL, response=True)
            _check(f"tc == 0 ({cut}) {name}", dev, Hs, states, nv, tc, kT, vg, vb, out, 0)
            chi, var = _np(out["chi"][0]), _np(out["variance"][0])
            if cut == "one":
                assert not chi[::2, :, N + 1].any() and chi[1::2, :, N + 1].any()
                continue
            assert not chi[:, :, N:].any()
            for p, Hm in enumerate(Hs):
                k = int(nv[p])
                nf = states[p, :k].astype(np.float64)
                P, _, _ = TH.reference(Hm, kT)
                mean = P @ nf
                cov = (nf - mean).T @ ((nf - mean) * P[:, None])
                t = RH.tol_chi(Hm, kT, nf.max(), [max(nf.max(), 1.0)] * N).max()
                assert np.all(np.abs(chi[p][:, :N] + cov / kT) <= t), (name, p)
                assert np.all(np.abs(np.diag(chi[p][:, :N]) + var[p] / kT) <= t), (name, p)
        env.close()


# ------------------------------------------------------------------ 3. the C entry point: NULL destinations, guard rows
def test_null_destinations_and_guard_rows(tmp_path):
    """with all three destinations NULL the call gives the bits of qd_eval_points_thermal; each destination alone gives the bits it
    has in the full call; nothing is written outside the caller's rows"""
    import torch
    from qadapt_hip import _lib
    N, R = 3, 8
    env = _vec(tmp_path, 1, N, R, 9870)
    env.reset(seed=9870)
    vg, vb = CH.points(N, np.random.default_rng(3), 150)                 # two slots of C P = 128
    kT = np.array([0.02])
    full = env.eval_points([0], vg[None], vb[None], kT=kT, outputs=THERMAL, response=True)
    g0, g1, n = 3, 5, 150
    rows = g0 + n + g1
    vg_all = torch.full((rows, N + 1), float("nan"), dtype=torch.float64, device="cuda")
    vb_all = torch.full((rows, N - 1), float("nan"), dtype=torch.float64, device="cuda")
    vg_all[g0:g0 + n] = torch.as_tensor(vg); vb_all[g0:g0 + n] = torch.as_tensor(vb)
    ids, start = np.array([0], np.int32), np.array([g0, g0 + n], np.int64)
    guard = -777.25
    shapes = {"signal": (), "occupations": (N,), "variance": (N,), "ztail": (), "chi": (N, 2 * N - 1), "jacobian": (N, 2 * N),
              "dsignal": (2 * N,)}

    def call(keys):
        dst = {k: torch.full((rows,) + shapes[k], guard, dtype=torch.float64, device="cuda") for k in keys}
        ptr = lambda k: dst[k].data_ptr() if k in dst else None      # noqa: E731
        opts = _lib.QdResponseOpts(struct_size=ctypes.sizeof(_lib.QdResponseOpts), var_dst=ptr("variance"), ztail_dst=ptr("ztail"),
                                   chi_dst=ptr("chi"), jac_dst=ptr("jacobian"), dsignal_dst=ptr("dsignal"))
        rc = env._lib.qd_eval_points_response(env._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                              start.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1,
                                              ctypes.c_void_p(vg_all.data_ptr()), ctypes.c_void_p(vb_all.data_ptr()),
                                              kT.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                              ctypes.c_void_p(ptr("signal")) if "signal" in dst else None,
                                              ctypes.c_void_p(ptr("occupations")) if "occupations" in dst else None,
                                              ctypes.byref(opts), env._stream())
        assert rc == 0, env._lib.qd_last_error(env._h)
        for k, t in dst.items():
            a = t.cpu().numpy()
            assert np.all(a[:g0] == guard) and np.all(a[g0 + n:] == guard), k
            assert PH.same(a[g0:g0 + n], full[k][0]), (keys, k)

    call(tuple(shapes))
    call(THERMAL)                                                        # the thermal kernel itself
    for k in ("chi", "jacobian", "dsignal"):
        call((k,))
    call(("signal", "dsignal"))
    env.close()


# ------------------------------------------------------------------ 4. refusals
def test_refusals(tmp_path):
    from qadapt_hip import _lib
    N, R = 3, 8
    zg, zb = np.zeros((1, 4, N + 1)), np.zeros((1, 4, N - 1))
    env = _vec(tmp_path, 1, N, R, 78)
    env.reset(seed=78)
    with pytest.raises(ValueError, match="response=True needs kT"):
        env.eval_points([0], zg, zb, response=True)
    with pytest.raises(ValueError, match="kT"):
        env.eval_points([0], zg, zb, kT=0.0, response=True)
    assert env.eval_points([0], zg, zb, kT=0.01, response=True)["chi"].shape == (1, 4, N, 2 * N - 1)
    env.close()
    env = _vec(tmp_path, 1, N, R, 77, validate=True)
    env.reset(seed=77)
    with pytest.raises(_lib.QdError, match="QD_FLAG_VALIDATE") as ei:
        env.eval_points([0], zg, zb, kT=0.01, response=True)
    assert f"code {_lib.QD_ERR_STATE}" in str(ei.value) and "qd_eval_points_response" in str(ei.value)
    env.close()
    # the voltage-dependent capacitance model: Lam would depend on v
    q = DM.load_yaml(None, "qarray_config.yaml")
    q["simulator"]["voltage_capacitance_model"]["type"] = "linear"
    qp = tmp_path / "qarray_vc.yaml"
    qp.write_text(yaml.safe_dump(q))
    env = _vec(tmp_path, 2, N, R, 79, qarray_config_path=str(qp))
    env.reset(seed=79)
    assert env._params_host[0][layout(N).scal + 4] != 0.0
    before = env.eval_points([0], zg, zb, kT=0.01, outputs=THERMAL)
    for more in ({}, {"n_charge": 2}):
        with pytest.raises(_lib.QdError, match="voltage-dependent capacitance") as ei:
            env.eval_points([1], zg, zb, kT=0.01, response=True, **more)
        assert f"code {_lib.QD_ERR_STATE}" in str(ei.value)
    # no response destination: the call is qd_eval_points_thermal, which takes such envs, and gives its bits
    import torch
    sig = torch.zeros(4, dtype=torch.float64, device="cuda")
    ids, start, kt = np.array([0], np.int32), np.array([0, 4], np.int64), np.array([0.01])
    g_d, b_d = torch.zeros((4, N + 1), dtype=torch.float64, device="cuda"), torch.zeros((4, N - 1), dtype=torch.float64, device="cuda")
    opts = _lib.QdResponseOpts(struct_size=ctypes.sizeof(_lib.QdResponseOpts))
    rc = env._lib.qd_eval_points_response(env._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                          start.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1, ctypes.c_void_p(g_d.data_ptr()),
                                          ctypes.c_void_p(b_d.data_ptr()), kt.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                          ctypes.c_void_p(sig.data_ptr()), None, ctypes.byref(opts), env._stream())
    assert rc == 0 and PH.same(sig, before["signal"][0])
    after = env.eval_points([0], zg, zb, kT=0.01, outputs=THERMAL)      # the thermal call itself is not refused, the handle is usable
    for key in THERMAL:
        assert PH.same(before[key], after[key]), key
    env.close()


# ------------------------------------------------------------------ 5. the facade
def test_facade_equals_the_vectorised_call(tmp_path):
    from qadapt_hip.env import QuantumDeviceEnv
    N, R = 3, 8
    path = _cfg(tmp_path, num_dots=N, resolution=R)
    backend = _vec(tmp_path, 1, N, R, 9900, config_path=path)
    env = QuantumDeviceEnv(config_path=path, num_dots=N, backend=backend)
    model = env.array.model
    T = float(backend.last_episode.extras["T"][0])
    gamma = float(model.coulomb_peak_width)
    vg, vb = CH.points(N, np.random.default_rng(6), 12)
    for lead in ((12,), (3, 4), ()):
        g = vg.reshape(lead + (N + 1,)) if lead else vg[0]
        b = vb.reshape(lead + (N - 1,)) if lead else vb[0]
        n = 12 if lead else 1
        chi, jac, ds = model.charge_response_open(g, b)
        assert chi.shape == lead + (N, 2 * N - 1) and jac.shape == lead + (N, 2 * N) and ds.shape == lead + (2 * N,)
        want = backend.eval_points([0], vg[None, :n], vb[None, :n], gamma=gamma, kT=TH.KB_REF * T, response=True)
        for got, key in ((chi, "chi"), (jac, "jacobian"), (ds, "dsignal")):
            assert PH.same(got.reshape(_np(want[key][0]).shape), want[key][0]), key
        assert all(PH.same(x, y) for x, y in zip((chi, jac, ds), model.charge_response_open(g, b, T=T)))
        chi, jac, ds = model.charge_response_closed(g, 2, vb=b)
        want = backend.eval_points([0], vg[None, :n], vb[None, :n], gamma=gamma, kT=TH.KB_REF * T, n_charge=2, response=True)
        assert PH.same(chi.reshape(n, N, 2 * N - 1), want["chi"][0]) and PH.same(jac.reshape(n, N, 2 * N), want["jacobian"][0])
    with pytest.raises(NotImplementedError):
        model.charge_response_open(vg)
    env.close()
