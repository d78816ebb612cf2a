"""Energy levels per point without a GPU: the core of csrc/qd_levels.h (shift, power-of-two scaling, Householder, Sturm-count
multisection) compiled for the CPU with the 64 lanes as a loop (tests/hosttest_levels) against numpy.linalg.eigvalsh on the
families of eig_cases.py, exact multiplicities, the block it builds from a record against the oracle's Hamiltonian, the
argument checks of qd_eval_points_ex on a handle that never reached a device, and the sanitizer program.
Bar: every level within 1e-12 ||A||_inf of eigvalsh, the project's eigenvalue bar."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import eig_cases as EC
import helpers as H
import qd_oracle as O

HDIR = os.path.join(H.ROOT, "tests", "hosttest_levels")
BAR = 1e-12
_LIB = None
_WORST = [0.0]


def levels_lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-s", "-C", HDIR, "libqdsim_hosttest_levels.so"])
        _LIB = ctypes.CDLL(os.path.join(HDIR, "libqdsim_hosttest_levels.so"))
    return _LIB


def solve(A, L):
    s = A.shape[0]
    lev = np.full(L, np.nan)
    assert levels_lib().qdhl_levels(s, L, H._p(EC.packed(A), ctypes.c_double), H._p(lev, ctypes.c_double)) == 0
    return lev


def check(A, tag, L=None):
    """every level within BAR ||A||_inf of eigvalsh, in order, +inf from s on; returns the worst ratio"""
    s = A.shape[0]
    L = min(8, s) if L is None else L
    w = np.linalg.eigvalsh(A)
    hn = EC.hnorm(A)
    lev = solve(A, L)
    n = min(L, s)
    assert np.isfinite(lev[:n]).all() and np.all(np.isposinf(lev[n:])), (tag, lev)
    assert np.all(np.diff(lev[:n]) >= 0), (tag, lev)
    err = np.abs(lev[:n] - w[:n]).max()
    assert err <= BAR * hn, (tag, s, err / hn if hn else err)
    r = err / hn if hn else 0.0
    _WORST[0] = max(_WORST[0], r)
    return r


@pytest.mark.parametrize("s", EC.LANE_SIZES)
def test_families_of_every_size(s):
    """hop blocks over the nine coupling scales, near-degenerate pairs, couplings spread over decades inside one block
    (1e-9..1e2 and 1e-30..1e45), and the classical block, at L = min(8, s)"""
    worst = 0.0
    for tscale, A in EC.scale_family(s):
        worst = max(worst, check(A, ("hop", tscale)))
    for sep in (1e-5, 1e-7, 3e-9):
        for tc, A, hn in EC.near_degenerate_family(s, sep):
            worst = max(worst, check(A, ("near", sep, tc)))
    for k, A in enumerate(EC.mixed_scale_family(s)):
        worst = max(worst, check(A, ("mixed", k)))
    for k, A in enumerate(EC.extreme_scale_family(s, reps=60)):
        worst = max(worst, check(A, ("extreme", k)))
    worst = max(worst, check(EC.classical_block(s), "classical"))
    print(f"[levels cpu] s={s}: worst |level - eigvalsh| / ||A||_inf = {worst:.2e}")


def test_single_state_column_tail_and_every_level_count():
    for a in (0.0, -3.5, 1e5, 1e-300):
        lev = solve(np.array([[a]]), 8)
        assert lev[0] == a and np.all(np.isposinf(lev[1:])), (a, lev)
    A = EC.column_tail_block()
    for L in range(1, 9):
        check(A, ("tail", L), L)
    check(EC.small_entry_block(), "small entry")
    rng = np.random.default_rng(3)
    B = EC.hop_block(rng, 17, 1.0)
    full = solve(B, 8)
    for L in range(1, 9):                                   # fewer levels: other sections, the same eigenvalues
        assert np.abs(solve(B, L) - full[:L]).max() <= 2 * BAR * EC.hnorm(B)
    z = np.zeros(40)
    assert levels_lib().qdhl_levels(33, 2, H._p(np.zeros(33 * 17), ctypes.c_double), H._p(z, ctypes.c_double)) == 1
    assert levels_lib().qdhl_levels(4, 9, H._p(np.zeros(10), ctypes.c_double), H._p(z, ctypes.c_double)) == 1
    assert levels_lib().qdhl_levels(4, 0, H._p(np.zeros(10), ctypes.c_double), H._p(z, ctypes.c_double)) == 1


def test_fixed_rounds():
    """(P + 1)-section down to 2^-58 of the bracket, P = 64 // L lanes per level: the smallest r with (P + 1)^r >= 2^58"""
    for L in range(1, 9):
        P = 64 // L
        r = levels_lib().qdhl_rounds(L)
        assert (P + 1) ** r >= 2 ** 58 > (P + 1) ** (r - 1), (L, r)
    assert levels_lib().qdhl_ws_bytes() <= 13 * 1024


def test_exact_multiplicities_come_back_bitwise_equal():
    # a diagonal with repeats: 2-fold, 3-fold and single values, shuffled
    d = np.array([0.75, 0.25, 0.75, 1.5, 0.25, 0.25, 3.0, 1.5, 7.0])
    lev = solve(np.diag(d), 8)
    w = np.sort(d)[:8]
    assert np.abs(lev - w).max() <= BAR * 7.0
    for k in range(7):
        assert (lev[k] == lev[k + 1]) == (w[k] == w[k + 1]), (k, lev)
    # the same with a large common offset (the shift takes it out exactly: the entries are exact in float64)
    lev2 = solve(np.diag(d + 4096.0), 8)
    for k in range(7):
        assert (lev2[k] == lev2[k + 1]) == (w[k] == w[k + 1]), (k, lev2)
    # two identical disconnected 2x2 blocks: every level twice; three copies: three times
    B = np.array([[0.3, -0.7], [-0.7, 1.1]])
    for copies in (2, 3):
        A = np.kron(np.eye(copies), B)
        lev = solve(A, 2 * copies)
        w = np.linalg.eigvalsh(B)
        for k in range(2 * copies):
            assert abs(lev[k] - w[k // copies]) <= BAR * EC.hnorm(A)
            assert lev[k] == lev[(k // copies) * copies], (copies, lev)
    # crossing levels of disconnected components come back in order
    A = np.zeros((5, 5)); A[:2, :2] = B; A[2:4, 2:4] = B + 0.2 * np.eye(2); A[4, 4] = 0.1
    check(A, "interleaved components")


# ------------------------------------------------------------------ the record path
def _record_fields(N, states, floors, F, nv):
    """the fields of a QdPixelRec from a kept list: codes (base-4 digits delta + 1, dot 0 most significant), E"""
    idx = np.zeros(32, np.uint16); E = np.zeros(32)
    K = states.shape[0]
    dig = states[:nv] - floors[None, :] + 1
    assert dig.min() >= 0 and dig.max() <= 3
    idx[:nv] = (dig * (4 ** np.arange(N - 1, -1, -1))[None, :]).sum(axis=1)
    E[:K] = F
    return idx, E


def n_valid(v_ext, dev, N, K):
    """valid candidates of the oracle's search (floor + delta >= 0), at most K"""
    n_cont = O.continuous_ground_state(v_ext, dev.cdd_inv_full, dev.cgd_full, N)
    cfg = O._delta_table(N)[None] + np.floor(n_cont)[:, None, :]
    return np.minimum(np.all(cfg >= 0, axis=-1).sum(axis=1), K), np.floor(n_cont).astype(np.int32)


@pytest.mark.parametrize("N,K", [(2, 32), (3, 32), (4, 32), (8, 32), (4, 20), (8, 20), (3, 8), (8, 8)])
def test_block_of_a_record_is_the_oracles_hamiltonian_without_the_padding(N, K):
    rng = np.random.default_rng(100 * N + K)
    eb = H.sample_blocks(N, [61, 62])
    lay = H.layout(N)
    short = 0
    for e in range(2):
        par, st = eb.params[e], eb.state[e]
        dev = H.dev_view(N, par)
        n = 24
        vg = par[lay.vopt:lay.vopt + N + 1] + rng.uniform(-4, 4, (n, N + 1))
        if N <= 3:
            vg[: n // 2] -= 8.0                                 # towards the empty array: short lists with |0..0> padding
        vb = par[lay.vbopt:lay.vbopt + N - 1] + rng.uniform(-3, 3, (n, N - 1))
        v_ext = np.concatenate([vg, vb], axis=1)
        states, _ = O.candidate_states(v_ext, dev.cdd_inv_full, dev.cgd_full, N, k=K)
        F = O.free_energy_states(v_ext, dev.cdd_inv_full, dev.cgd_full, states, N)
        tc = O.tunnel_couplings(O.effective_barrier_potential(vg, vb, dev.Cbg, dev.Cbb), dev.tc_base, dev.alpha)
        Ht = O.tunnel_hamiltonian(tc, states)
        nvs, floors = n_valid(v_ext, dev, N, K)
        for p in range(n):
            nv = int(nvs[p])
            short += nv < K
            idx, E = _record_fields(N, states[p], floors[p], F[p], nv)
            Hm = np.zeros((32, 32)); hn = ctypes.c_double(); lev = np.zeros(8)
            got = levels_lib().qdhl_record(N, H._p(idx, ctypes.c_uint16), H._p(np.ascontiguousarray(floors[p]), ctypes.c_int32),
                                           H._p(np.ascontiguousarray(tc[p]), ctypes.c_double), H._p(E, ctypes.c_double), nv, K, 8,
                                           H._p(Hm, ctypes.c_double), ctypes.byref(hn), H._p(lev, ctypes.c_double))
            assert got == nv
            ref = np.diag(F[p, :nv]) + Ht[p, :nv, :nv]
            np.testing.assert_allclose(Hm[:nv, :nv], ref, rtol=4e-16, atol=0.0)
            assert not Hm[nv:].any() and not Hm[:, nv:].any()                     # the padding is left out
            assert ((Hm[:nv, :nv] != 0) == (ref != 0)).all()
            hn_ref = np.abs(ref).sum(axis=1).max()
            assert abs(hn.value - hn_ref) <= 1e-14 * hn_ref
            w = np.linalg.eigvalsh(ref)
            m = min(8, nv)
            assert np.abs(lev[:m] - w[:m]).max() <= BAR * hn_ref and np.all(np.isposinf(lev[m:]))
    if N <= 3 and K == 32:
        assert short > 0, "no short list among the points"


# ------------------------------------------------------------------ the C entry point without a device
def _built_lib():
    from qadapt_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is missing: run __graft_entry__.build() before the tests (no test compiles it)")
    return _lib, _lib.lib()


def _handle(L, N, R, B, flags=0, qconfig=None):
    from qadapt_hip import device_model as DM
    from qadapt_hip.vec_env import make_qd_config
    cfg = make_qd_config(DM.load_yaml(None, "env_config.yaml"), qconfig or DM.load_yaml(None, "qarray_config.yaml"), N, R, B,
                         flags=flags)
    h = ctypes.c_void_p()
    L.qd_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    if not h:
        pytest.fail("qd_create handed out no handle")
    return h


def test_prototype_and_struct_match_the_header():
    import re
    _lib, L = _built_lib()
    hdr = open(os.path.join(H.ROOT, "include", "qdsim.h")).read()
    assert "qd_eval_points_ex" in _lib.EXPORTS and hasattr(L, "qd_eval_points_ex")
    m = re.search(r"\bint qd_eval_points_ex\((.*?)\);", hdr, re.S)
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    fn = L.qd_eval_points_ex
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(decl) == 10
    assert fn.argtypes[8]._type_ is _lib.QdPointsOpts and decl[8].startswith("const qd_points_opts*")
    body = re.search(r"typedef struct qd_points_opts \{(.*?)\} qd_points_opts;", hdr, re.S).group(1)
    names = [ln.split(";")[0].split()[-1].lstrip("*") for ln in body.strip().splitlines()]
    assert names == [f[0] for f in _lib.QdPointsOpts._fields_]
    assert ctypes.sizeof(_lib.QdPointsOpts) == 48
    assert int(re.search(r"#define QD_LEVELS_MAX (\d+)", hdr).group(1)) == _lib.QD_LEVELS_MAX == 8


def test_argument_checks_need_no_device():
    _lib, L = _built_lib()
    B = 3
    one = ctypes.c_void_p(64)                          # a device pointer that is never dereferenced
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)     # noqa: E731
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)     # noqa: E731

    def opts(**kw):
        o = _lib.QdPointsOpts(struct_size=ctypes.sizeof(_lib.QdPointsOpts), n_levels=2, levels_dst=64, hnorm_dst=64)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(h, o, env=i32(0), start=i64(0, 1), ng=1, sig=one, occ=one):
        return L.qd_eval_points_ex(h, env, start, ng, one, one, sig, occ, None if o is None else ctypes.byref(o), None)

    assert call(None, opts()) == _lib.QD_ERR_ARG
    h = _handle(L, 4, 8, B)
    try:
        bad = [(opts(struct_size=40), b"struct_size"), (opts(n_levels=-1), b"n_levels"), (opts(n_levels=9), b"n_levels"),
               (opts(levels_dst=None), b"levels_dst"), (opts(states_dst=64), b"states_dst")]
        for o, word in bad:
            assert call(h, o) == _lib.QD_ERR_ARG, word
            msg = L.qd_last_error(h)
            assert msg.startswith(b"qd_eval_points_ex") and word in msg, msg
        # the checks of the shared loop, under the new name
        assert call(h, opts(), env=i32(B)) == _lib.QD_ERR_ARG and b"qd_eval_points_ex: env id" in L.qd_last_error(h)
        assert call(h, opts(), start=i64(2, 1)) == _lib.QD_ERR_ARG and b"qd_eval_points_ex" in L.qd_last_error(h)
        assert call(h, opts(n_charge_host=i32(-1))) == _lib.QD_ERR_ARG and b"0..32767" in L.qd_last_error(h)
        assert call(h, None, ng=-1) == _lib.QD_ERR_ARG
        # groups without a point: nothing to do, with or without options, levels only included
        assert call(h, opts(), start=i64(3, 3)) == 0 and call(h, None, start=i64(3, 3)) == 0
        assert call(h, opts(n_levels=0, levels_dst=None), start=i64(3, 3)) == 0
        assert call(h, opts(), start=i64(3, 3), sig=None, occ=None) == 0
        assert call(h, opts(n_charge_host=i32(2), states_dst=64), start=i64(3, 3)) == 0
    finally:
        L.qd_destroy(h)
    from qadapt_hip.vec_env import override_charge_states
    from qadapt_hip import device_model as DM
    q = override_charge_states(DM.load_yaml(None, "qarray_config.yaml"), "all")
    q["simulator"]["model"]["max_charge_carriers"] = 2
    for kw, word in ((dict(flags=_lib.QD_FLAG_VALIDATE), b"QD_FLAG_VALIDATE"), (dict(qconfig=q), b"full charge-state space")):
        hs = _handle(L, 3, 8, B, **kw)
        try:
            assert call(hs, opts()) == _lib.QD_ERR_STATE and word in L.qd_last_error(hs)
            assert L.qd_last_error(hs).startswith(b"qd_eval_points_ex")
            assert call(hs, opts(n_levels=9)) == _lib.QD_ERR_ARG                      # arguments first
        finally:
            L.qd_destroy(hs)


def test_python_layer_checks_levels_before_the_device():
    import inspect
    from qadapt_hip.env import ModelFacade
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    sig = inspect.signature(VecQuantumDeviceEnv.eval_points).parameters
    assert list(sig)[-1] == "levels" and sig["levels"].default == 0

    class Stub:
        def __init__(self):
            self.calls = []

        def eval_points(self, env_ids, vg, vb, gamma=None, outputs=("signal", "occupations"), n_charge=None, states=False, levels=0):
            self.calls.append(dict(outputs=tuple(outputs), n_charge=n_charge, levels=levels, gamma=gamma))
            m = np.asarray(vg).shape[1]
            return {"levels": np.arange(m * levels, dtype=np.float64).reshape(1, m, levels), "hnorm": np.ones((1, m))}

    N = 4
    model = ModelFacade(Stub(), N)
    model.coulomb_peak_width = 0.3                                                   # (levels do not depend on it)
    for lead in ((), (5,), (3, 7)):
        vg, vb = np.zeros(lead + (N + 1,)), np.zeros(lead + (N - 1,))
        lev, hn = model.energy_levels_open(vg, vb)
        assert lev.shape == lead + (2,) and hn.shape == lead and lev.dtype == hn.dtype == np.float64
        assert model._b.calls[-1] == dict(outputs=(), n_charge=None, levels=2, gamma=None)
        lev, hn = model.energy_levels_closed(vg, 3, n_levels=5, vb=vb)
        assert lev.shape == lead + (5,) and hn.shape == lead
        assert model._b.calls[-1] == dict(outputs=(), n_charge=3, levels=5, gamma=None)
    with pytest.raises(NotImplementedError):
        model.energy_levels_open(np.zeros(N + 1))
    with pytest.raises(ValueError):
        model.energy_levels_open(np.zeros(N + 1), np.zeros(N))


def test_sanitizer_program_runs_clean():
    """the core and the record path under AddressSanitizer and UBSan, as a stand-alone program in a child process"""
    subprocess.check_call(["make", "-s", "-C", HDIR, "qd_levels_asan"])
    r = subprocess.run([os.path.join(HDIR, "qd_levels_asan")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "levels asan ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


def test_worst_ratio_is_reported():
    print(f"[levels cpu] worst ratio over the families run in this session: {_WORST[0]:.2e} (bar {BAR:.0e})")
    assert _WORST[0] <= BAR
