"""qd_k_update alone on the MI355X (run with -m gpu), every dot count 2..8: qd_load_episodes / qd_set_state put the inputs
in place and qd_update_capacitance launches only that kernel -- no observation.  Both parities of the round-robin schedule of
qd_pinv_wave (G = N + 1 even for N = 3, 5, 7), the [-6, 2] log-variance clamp, the acceptance gate, the +-1 mean clamp,
rank-deficient and ill-conditioned VGM products, the 1e-15 * s_max cut-off, row pivoting in qd_solve, and the launch
shape.  References: traces of the reference's own updater classes on the float32 numbers the device is fed
(tests/golden/updater_traces_f32.npz), the oracle, and extended-precision linear algebra (tests/update_helpers.py)."""
import numpy as np
import pytest

import helpers as H
import qd_oracle as O
import update_helpers as U
from qadapt_hip.layout import layout

pytestmark = pytest.mark.gpu

KALMAN_BAR = dict(rtol=1e-12, atol=1e-15)          # the project's bar for Kalman means and variances


def _changed(prev_m, prev_v, m, v):
    return (m != prev_m) | (v != prev_v)


# ------------------------------------------------------------------ a. the reference's traces on the device
@pytest.mark.parametrize("n_out", [3, 2])
@pytest.mark.parametrize("method", ["kalman", "direct"])
@pytest.mark.parametrize("N", range(2, 9))
def test_fixture_traces_on_the_device(N, method, n_out):
    """env 0 is fed the fixture case of this (N, updater, outputs) step by step and must reproduce the reference-run
    means and variances; an entry changes exactly when the fixture's did.  env 1 of the same launch is fed the inputs of
    the OTHER updater's case (different gate decisions, different clamps) and is compared with this updater's oracle,
    which test_oracle_golden.py pins to the same fixture."""
    fx = U.fixture()
    own = fx[(N, method, n_out)]
    other = fx[(N, "direct" if method == "kalman" else "kalman", n_out)]
    L = layout(N)
    par, st = U.blocks(N, 2)
    ok = (O.DirectOracle if method == "direct" else O.KalmanOracle)(N, include_nnn=n_out == 3)
    with U.Handle(N, 2, method, n_out) as h:
        h.load(par, st, reset_kalman=1)
        pm, pv = (a.copy() for a in U.views(L, h.get_state())[:2])
        assert np.array_equal(pm[1], ok.means) and np.array_equal(pv[1], ok.vars)              # the priors
        f_pm, f_pv = pm[0].copy(), pv[0].copy()
        o_pm, o_pv = ok.means.copy(), ok.vars.copy()
        seen_change = False
        for t in range(own["values"].shape[0]):
            values = np.stack([own["values"][t], other["values"][t]]); log_vars = np.stack([own["log_vars"][t], other["log_vars"][t]])
            h.update(values, log_vars, recompute=1)
            m, v = (a.copy() for a in U.views(L, h.get_state())[:2])
            # env 0 against the reference run
            assert np.allclose(m[0], own["means"][t], **KALMAN_BAR), (t, np.abs(m[0] - own["means"][t]).max())
            assert np.allclose(v[0], own["variances"][t], **KALMAN_BAR), (t, np.abs(v[0] - own["variances"][t]).max())
            dev_ch = _changed(pm[0], pv[0], m[0], v[0]); fix_ch = _changed(f_pm, f_pv, own["means"][t], own["variances"][t])
            assert np.array_equal(dev_ch, fix_ch), (t, np.argwhere(dev_ch != fix_ch))
            n_acc = int(own["accepted"][t] - (own["accepted"][t - 1] if t else 0))
            assert (n_acc == 0) == (not fix_ch.any())                                          # the fixture's own counters agree
            seen_change |= bool(fix_ch.any())
            # a clamped mean is exactly +-1 on the device too
            assert np.array_equal(np.abs(m[0]) == 1.0, np.abs(own["means"][t]) == 1.0), t
            # env 1 against the oracle of this updater
            ok.update_from_cnn(other["values"][t], other["log_vars"][t])
            assert np.allclose(m[1], ok.means, **KALMAN_BAR) and np.allclose(v[1], ok.vars, **KALMAN_BAR), t
            assert np.array_equal(_changed(pm[1], pv[1], m[1], v[1]), _changed(o_pm, o_pv, ok.means, ok.vars)), t
            o_pm, o_pv = ok.means.copy(), ok.vars.copy()
            pm, pv, f_pm, f_pv = m, v, own["means"][t].copy(), own["variances"][t].copy()
        assert seen_change and own["rejected"][-1] > 0 and (np.abs(own["means"]) == 1.0).any()


@pytest.mark.parametrize("method", ["kalman", "direct"])
@pytest.mark.parametrize("N", [2, 5])
def test_upper_clamp_with_a_wide_gate(N, method):
    """At the default gate (0.05) a variance at the upper clamp is rejected whatever the clamp is.  With
    variance_threshold = 10 the gate lies between exp(2) and exp(3): a log-variance in (2, 3] is accepted BECAUSE it is
    clamped to 2, and the direct updater stores exp(2) itself.  process_noise = 0.01 is the other knob no test sets."""
    B, thr, q = 3, 10.0, 0.01
    L = layout(N)
    par, st = U.blocks(N, B)
    rng = np.random.default_rng([41, N])
    cls = O.DirectOracle if method == "direct" else O.KalmanOracle
    ks = [cls(N, variance_threshold=thr, process_noise=q) for _ in range(B)]
    with U.Handle(N, B, method, variance_threshold=thr, process_noise=q) as h:
        h.load(par, st, reset_kalman=1)
        hit = 0
        for t in range(4):
            values, log_vars = U.fixture_like_inputs(rng, (B, N - 1, 3))
            if t % 2 == 0:                                    # past ln 10 = 2.303: accepted only because clamped
                log_vars[:, :, 0] = rng.uniform(2.35, 2.95, (B, N - 1)).astype(np.float32)
            hit += int((log_vars[:, :, 0] > np.log(thr)).sum())
            h.update(values, log_vars, recompute=1)
            m, v = U.views(L, h.get_state())[:2]
            for e in range(B):
                before = ks[e].vars.copy()
                ks[e].update_from_cnn(values[e], log_vars[e])
                assert np.allclose(m[e], ks[e].means, **KALMAN_BAR) and np.allclose(v[e], ks[e].vars, **KALMAN_BAR), (t, e)
                if t == 0:                                    # every nearest-neighbour pair took the clamped variance
                    assert (np.diag(ks[e].vars, 1) != np.diag(before, 1)).all()
                    if method == "direct" and N == 2:
                        assert np.isclose(v[e][0, 1], np.exp(2.0), rtol=4e-16, atol=0)      # exp(2) itself, to an ulp of exp
        assert hit >= B * (N - 1) * 2


# ------------------------------------------------------------------ b. oracle parity where nobody compared
@pytest.mark.parametrize("N", [3, 5, 6, 7])
def test_oracle_parity_at_the_uncompared_dot_counts(N):
    """reset (no ground truth, env.py:233) plus three updates, inputs drawn as the fixture's: Kalman state, VGM and ground
    truth against the oracle at the bars of test_episode_matches_oracle_env.  N = 3, 5, 7 run the even-G schedule."""
    B = 3
    L = layout(N)
    par, st = U.blocks(N, B)
    rng = np.random.default_rng([77, N])
    devs = [H.dev_view(N, par[e]) for e in range(B)]
    ks = [O.KalmanOracle(N) for _ in range(B)]
    with U.Handle(N, B) as h:
        h.load(par, st, reset_kalman=1)
        for t in range(4):
            values, log_vars = U.fixture_like_inputs(rng, (B, N - 1, 3))
            h.update(values, log_vars, recompute=int(t > 0))
            m, v, vgm, ggt, bgt, sgt = U.views(L, h.get_state())
            for e in range(B):
                ks[e].update_from_cnn(values[e], log_vars[e])
                s = np.linalg.svd(U.product(devs[e].cdd_inv_full, ks[e].means), compute_uv=False)
                assert s[0] / s[-1] < 1e3                          # input condition: the bars below are for such products
                ovgm = O.vgm_from_estimate(devs[e], ks[e].full_matrix())
                assert np.allclose(m[e], ks[e].means, **KALMAN_BAR) and np.allclose(v[e], ks[e].vars, **KALMAN_BAR), (t, e)
                if t == 0:
                    assert np.allclose(vgm[e], ovgm, rtol=1e-9, atol=1e-11), (t, e, np.abs(vgm[e] - ovgm).max())
                    assert np.array_equal(U.bits(ggt[e]), U.bits(st[e, L.s_gate_gt:L.s_gate_gt + N]))     # not recomputed
                    continue
                assert np.allclose(vgm[e], ovgm, rtol=1e-8, atol=1e-10), (t, e, np.abs(vgm[e] - ovgm).max())
                ogt, obgt, osgt = O.ground_truth(devs[e], ovgm, devs[e].origin)
                assert np.allclose(ggt[e], ogt, rtol=2e-6, atol=1e-6), (t, e)
                assert np.isclose(sgt[e], osgt, rtol=1e-8), (t, e)
                assert np.array_equal(bgt[e].astype(np.float32), obgt), (t, e)


# ------------------------------------------------------------------ c. the pseudo-inverse on matrix families
@pytest.mark.parametrize("G", range(3, 10))
def test_pinv_wave_on_matrix_families(G):
    """Every update rejected (log-variances at 2), so the product handed to qd_pinv_wave<G> is fixed by the loaded cdd_inv
    and the Kalman means set beforehand: E = I gives exactly -cdd_inv.  Bar: || P_dev - P_ref ||_2 <= C_PINV kappa_2 eps
    || P_ref ||_2 against the extended-precision pseudo-inverse, C_PINV = 8 x what np.linalg.pinv itself reaches
    (update_helpers.NUMPY_PINV_WORST).  Measured on an MI355X: worst device ratio 2.175
    ("dup_column" x 1e+60, G = 3), numpy's own worst 5.123, bar 41.0."""
    N = G - 1
    L = layout(N)
    cases = U.pinv_cases(G)
    B = len(cases)
    par, st = (a.copy() for a in U.blocks(N, B))
    for e, c in enumerate(cases):
        U.check_pinv_case_conditions(c)
        assert np.array_equal(U.product(c["cdd_inv"], c["means"]), c["target"]), c["name"]
        par[e, L.cdd_inv:L.cdd_inv + G * G] = c["cdd_inv"].ravel()
    assert {c["name"] for c in cases if c["deficient"] and c["rank"]} >= {"dup_column", "dep_row", "zero_column", "clamped_one_pair"}
    with U.Handle(N, B) as h:
        h.load(par, st, reset_kalman=1)
        s0 = h.get_state()
        for e, c in enumerate(cases):
            s0[e, L.s_kmean:L.s_kmean + N * N] = c["means"].ravel()
        h.set_state(s0)
        h.update(np.zeros((B, N - 1, 3), np.float32), np.full((B, N - 1, 3), 2.0, np.float32), recompute=0)
        s1 = h.get_state()
    m0, v0 = U.views(L, s0)[:2]; m1, v1, vgm = U.views(L, s1)[:3]
    assert np.array_equal(U.bits(m0), U.bits(m1)) and np.array_equal(U.bits(v0), U.bits(v1))       # all rejected
    ratios = {c["name"]: U.pinv_ratio(vgm[e], c) for e, c in enumerate(cases)}
    worst = max(ratios, key=ratios.get)
    print(f"G={G}: worst device ratio {ratios[worst]:.3f} at {worst}; bar {U.C_PINV:.1f}; "
          + " ".join(f"{k}={r:.2f}" for k, r in ratios.items()))
    for e, c in enumerate(cases):
        assert ratios[c["name"]] <= U.C_PINV, (c["name"], ratios[c["name"]], c["kappa"])
        if c["rank"] == 0:
            assert not vgm[e].any()


# ------------------------------------------------------------------ d. the ground-truth solve alone
def _solve_run(h, L, par, st, vgms):
    s0 = st.copy()
    for e, A in enumerate(vgms):
        s0[e, L.s_vgm:L.s_vgm + L.G * L.G] = A.ravel()
    h.load(par, s0, reset_kalman=1)
    s0 = h.get_state()
    h.update(None, None, recompute=1)
    return s0, h.get_state()


@pytest.mark.parametrize("N", range(2, 9))
def test_ground_truth_solve_alone(N):
    """values = log_vars = NULL, recompute_ground_truth = 1: qd_solve on the stored VGM.  sensor_gt (unrounded float64)
    within delta = C_SOLVE kappa_2 eps || x_ref ||_2 of the extended-precision solution, C_SOLVE = 8 x what
    np.linalg.solve itself reaches (0.1262, so 1.01; the device's worst measured: 0.0653); gate_gt the float32 of a value within delta; barrier_gt = float32(vbopt) exactly.  One
    env holds an exactly singular VGM: its ground truth is unspecified, the others must not notice it."""
    G = N + 1
    L = layout(N)
    cases = U.solve_cases(G)
    B = len(cases)
    par, st = U.blocks(N, B)
    sing = [e for e, c in enumerate(cases) if c["singular"]]
    assert len(sing) == 1
    with U.Handle(N, B) as h:
        s0, s1 = _solve_run(h, L, par, st, [c["vgm"] for c in cases])
        _, s2 = _solve_run(h, L, par, st, [(-np.eye(G) if c["singular"] else c["vgm"]) for c in cases])
    m0, v0, g0 = U.views(L, s0)[:3]; m1, v1, g1, ggt, bgt, sgt = U.views(L, s1)
    for a, b in ((m0, m1), (v0, v1), (g0, g1)):                              # NULL outputs: Kalman state and VGM stay
        assert np.array_equal(U.bits(a), U.bits(b))
    others = [e for e in range(B) if e not in sing]
    assert np.array_equal(U.bits(s1[others]), U.bits(s2[others]))            # the singular env's neighbours are untouched by it
    for e in others:
        c = cases[e]
        b = U.solve_rhs(L, par[e])
        x = U.ref_solve(c["vgm"], b)
        delta = U.C_SOLVE * c["kappa"] * U.EPS * np.linalg.norm(x)
        err = abs(sgt[e] - x[N])
        print(f"N={N} {c['name']}: sensor error / (kappa eps |x|) = {err / (c['kappa'] * U.EPS * np.linalg.norm(x)):.4f}, bar {U.C_SOLVE:.2f}")
        assert err <= delta, (c["name"], err, delta)
        lo, hi = (x[:N] - delta).astype(np.float32), (x[:N] + delta).astype(np.float32)
        assert np.array_equal(ggt[e], ggt[e].astype(np.float32).astype(np.float64))           # float32 numbers
        assert np.all((ggt[e] >= lo) & (ggt[e] <= hi)), (c["name"], ggt[e], x[:N])
        assert np.array_equal(U.bits(bgt[e]), U.bits(par[e, L.vbopt:L.vbopt + N - 1].astype(np.float32).astype(np.float64)))


# ------------------------------------------------------------------ e. launch shape
def test_env_id_lists_touch_only_their_envs():
    N, B = 5, 6                                          # G = 6: the even schedule
    L = layout(N)
    par, st = U.blocks(N, B)
    values, log_vars = U.fixture_like_inputs(np.random.default_rng(12), (B, N - 1, 3))
    with U.Handle(N, B) as h:
        h.load(par, st, reset_kalman=1)
        fresh = h.get_state()
        h.update(values, log_vars, recompute=1)
        full = h.get_state()
        assert all((U.bits(full[e]) != U.bits(fresh[e])).any() for e in range(B))
        for ids in ([1, 3, 4], list(range(B))[::-1], [B - 1], [4, 0]):
            h.load(par, st, reset_kalman=1)
            h.update(values, log_vars, ids=ids, recompute=1)
            got = h.get_state()
            for e in range(B):
                want = full[e] if e in ids else fresh[e]
                assert np.array_equal(U.bits(got[e]), U.bits(want)), (ids, e)
        # n = 0 is a no-op, with a list or without one to read
        h.load(par, st, reset_kalman=1)
        h.update(values, log_vars, ids=[2, 3], n=0, recompute=1)
        assert np.array_equal(U.bits(h.get_state()), U.bits(fresh))
        # a list longer than the count: only the first n entries run
        h.update(values, log_vars, ids=[2, 3, 5], n=2, recompute=1)
        got = h.get_state()
        for e in range(B):
            assert np.array_equal(U.bits(got[e]), U.bits(full[e] if e in (2, 3) else fresh[e])), e


def test_result_does_not_depend_on_the_slot():
    """the same env data at slot 0 and slot B - 1, B = 1, 3, 257: equal bits after two updates"""
    N = 3
    L = layout(N)
    p4, s4 = U.blocks(N, 4)
    rng = np.random.default_rng(21)
    v4, l4 = zip(*(U.fixture_like_inputs(rng, (2, N - 1, 3)) for _ in range(4)))     # per device: two steps of inputs
    rows = {}
    for B in (1, 3, 257):
        src = np.arange(B) % 3 + 1
        src[0] = src[B - 1] = 0
        with U.Handle(N, B) as h:
            h.load(p4[src], s4[src], reset_kalman=1)
            for t in range(2):
                h.update(np.stack([v4[k][t] for k in src]), np.stack([l4[k][t] for k in src]), recompute=1)
            st = h.get_state()
        rows[B] = st[0]
        assert np.array_equal(U.bits(st[0]), U.bits(st[B - 1])), B
        assert B == 1 or not np.array_equal(U.bits(st[0]), U.bits(st[1]))
    assert np.array_equal(U.bits(rows[1]), U.bits(rows[3])) and np.array_equal(U.bits(rows[1]), U.bits(rows[257]))
    assert (rows[1][L.s_vgm:L.s_vgm + (N + 1) ** 2] != s4[0, L.s_vgm:L.s_vgm + (N + 1) ** 2]).any()


@pytest.mark.parametrize("method", ["perfect", None])
def test_perfect_and_null_leave_means_and_vgm(method):
    """update_method perfect / null: the step calls qd_update_capacitance with NULL outputs; Kalman state and VGM stay as
    they are and the ground truth is that of the stored VGM"""
    N, B = 4, 3
    L = layout(N); G = N + 1
    par, st = U.blocks(N, B)
    st = st.copy()
    st[:, L.s_vgm:L.s_vgm + G * G] += np.random.default_rng(4).normal(0, 0.05, (B, G * G))
    with U.Handle(N, B, method) as h:
        h.load(par, st, reset_kalman=1)
        s0 = h.get_state()
        h.update(None, None, recompute=1)
        s1 = h.get_state()
        h.update(None, None, recompute=0)                                   # and without the solve: nothing at all
        s2 = h.get_state()
    assert np.array_equal(U.bits(s1), U.bits(s2))
    for a, b in zip(U.views(L, s0)[:3], U.views(L, s1)[:3]):
        assert np.array_equal(U.bits(a), U.bits(b))
    _, _, vgm, ggt, bgt, sgt = U.views(L, s1)
    for e in range(B):
        x = np.linalg.solve(vgm[e], U.solve_rhs(L, par[e]))
        assert np.allclose(ggt[e], x[:N].astype(np.float32), rtol=1e-6) and np.isclose(sgt[e], x[N], rtol=1e-10)
