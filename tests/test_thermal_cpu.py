"""The thermal state per point without a GPU: the core of csrc/qd_thermal.h (shift, power-of-two scaling, round-robin cyclic
Jacobi, Boltzmann weights, populations, moments) compiled for the CPU with the 64 lanes as a loop (tests/hosttest_thermal) against
numpy.linalg.eigh on the families of eig_cases.py, the exact cases (zero couplings, the 2 x 2 block, a doubly degenerate lowest
pair, one state), the eigenpairs themselves, the sweep cap, the record path, the header / ctypes agreement and the argument checks
of qd_eval_points_thermal on a handle that never reached a device, the Python layer, and the sanitizer program.
Bound: thermal_helpers -- populations within 4 (1e-12 hs + 1e-13 hn) min(1 / kT, 1 / g) + 1e-12 of the reference.
Measured over the families (31 sizes, 161 blocks each, three temperatures each): worst err / tol 5.2e-4 on the populations, 2.5e-4
on ztail; residual 2.0e-15 ||A||_inf, orthogonality 1.4e-14, at most 10 sweeps of the 24 allowed."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import eig_cases as EC
import helpers as H
import qd_oracle as O
import thermal_helpers as TH
from test_levels_cpu import _built_lib, _handle, _record_fields, n_valid

HDIR = os.path.join(H.ROOT, "tests", "hosttest_thermal")
EPS = np.finfo(np.float64).eps
WS_BYTES = 22792                                      # the figure of the header comment of csrc/qd_thermal.h
_LIB = None
_WORST = {"pop": 0.0, "ztail": 0.0, "resid": 0.0, "orth": 0.0, "sweeps": 0}
DP = ctypes.POINTER(ctypes.c_double)


def tol_ztail(A, kT):
    """the reference's bound on the last weight plus 4 eps: on blocks whose norm is far below kT (the 2 x 2 block at
    t = 1e-12) that bound falls below the rounding of exp, sum and quotient of a value of order one, half an ulp to an ulp each"""
    return TH.tol_ztail(A, kT) + 4 * EPS


def thermal_lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-s", "-C", HDIR, "libqdsim_hosttest_thermal.so"])
        _LIB = ctypes.CDLL(os.path.join(HDIR, "libqdsim_hosttest_thermal.so"))
        _LIB.qdht_thermal.argtypes = [ctypes.c_int, DP, ctypes.c_double, DP, DP, DP, DP]
        _LIB.qdht_record.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_int32), DP, DP,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_double, DP, DP, DP, DP]
    return _LIB


def solve(A, kT):
    """(sweeps, P, lam, V, ztail) of the host-compiled core"""
    s = A.shape[0]
    P, lam, V, z = np.full(s, np.nan), np.full(s, np.nan), np.full((s, s), np.nan), np.full(1, np.nan)
    sweeps = thermal_lib().qdht_thermal(s, H._p(EC.packed(A), ctypes.c_double), kT, H._p(P, ctypes.c_double),
                                        H._p(lam, ctypes.c_double), H._p(V, ctypes.c_double), H._p(z, ctypes.c_double))
    assert sweeps >= 0, (s, kT, sweeps)
    return sweeps, P, lam, V, z[0]


def check(A, kT, tag):
    """populations and ztail within the module's bound, eigenpairs, sweep count; returns the worst err / tol"""
    s = A.shape[0]
    sweeps, P, lam, V, z = solve(A, kT)
    cap = thermal_lib().qdht_sweep_cap()
    assert sweeps < cap, (tag, sweeps)
    Pr, wt, _ = TH.reference(A, kT)
    r = float(np.abs(P - Pr).max() / TH.tol_occ(A, kT, 1.0))
    rz = float(abs(z - wt[-1]) / tol_ztail(A, kT))
    hn = EC.hnorm(A)
    resid = float(np.abs(A @ V - V * lam[None, :]).max() / hn) if hn else 0.0
    orth = float(np.abs(V.T @ V - np.eye(s)).max())
    assert r <= 1.0 and rz <= 1.0, (tag, s, kT, r, rz)
    assert resid <= 1e-12 and orth <= 1e-13, (tag, s, resid, orth)
    assert abs(P.sum() - 1.0) <= 64 * EPS and P.min() >= 0.0, (tag, P.sum())
    for k, v in (("pop", r), ("ztail", rz), ("resid", resid), ("orth", orth), ("sweeps", sweeps)):
        _WORST[k] = max(_WORST[k], v)
    return max(r, rz)


def _temperatures(A):
    d = np.diag(A)
    spread = d.max() - d.min()
    return [f * spread if spread > 0 else f for f in (1e-3, 1e-1, 10.0)]


@pytest.mark.parametrize("s", EC.LANE_SIZES)
def test_families_of_every_size(s):
    """hop blocks over the nine coupling scales, near-degenerate pairs, couplings spread over decades inside one block
    (1e-9..1e2 and 1e-30..1e45), and the classical block, at kT = 1e-3, 1e-1 and 10 times the spread of the diagonal"""
    worst = 0.0
    fam = [(("hop", t), A) for t, A in EC.scale_family(s)]
    for sep in (1e-5, 1e-7, 3e-9):
        fam += [(("near", sep, tc), A) for tc, A, _ in EC.near_degenerate_family(s, sep)]
    fam += [(("mixed", k), A) for k, A in enumerate(EC.mixed_scale_family(s))]
    fam += [(("extreme", k), A) for k, A in enumerate(EC.extreme_scale_family(s, reps=60))]
    fam.append(("classical", EC.classical_block(s)))
    for tag, A in fam:
        for kT in _temperatures(A):
            worst = max(worst, check(A, kT, tag))
    print(f"[thermal cpu] s={s}: worst err / tol {worst:.2e}")


@pytest.mark.parametrize("s", EC.LANE_SIZES)
def test_zero_couplings_give_the_classical_distribution(s):
    """EC.classical_block and a block whose tunnel part is exactly zero, with a large common offset: P = softmax of the shifted
    diagonal within 64 eps, V = I, no sweep rotates anything"""
    rng = np.random.default_rng(500 + s)
    for A in (EC.classical_block(s), np.diag(4096.0 + rng.uniform(0, 2, s))):
        for kT in (1e-3, 0.05, 1.0, 30.0):
            sweeps, P, lam, V, z = solve(A, kT)
            d = np.diag(A) - np.diag(A).min()
            with np.errstate(under="ignore"):
                ref = TH.softmax(-d / kT)
            assert sweeps == 0 and np.array_equal(V, np.eye(s)) and np.array_equal(lam, np.diag(A))
            assert np.abs(P - ref).max() <= 64 * EPS, (s, kT, np.abs(P - ref).max())
            assert abs(z - ref.min()) <= 64 * EPS


def test_two_by_two_block_against_the_closed_form():
    """[[0, -t], [-t, eps]]: gap D = sqrt(eps^2 + 4 t^2), ground vector (cos, sin) with cos^2 = (1 + eps / D) / 2,
    P_0 = w_- cos^2 + w_+ sin^2, w_+ = 1 / (1 + exp(D / kT)).  The reference's bound on the populations."""
    for eps in (0.0, 1e-9, 0.3, -0.3, 5.0):
        for t in (1e-12, 1e-3, 0.2, 40.0):
            for kT in (1e-3, 0.1, 3.0):
                A = np.array([[0.0, -t], [-t, eps]])
                _, P, lam, V, z = solve(A, kT)
                D = np.hypot(eps, 2 * t)
                c2 = 0.5 * (1.0 + eps / D)
                with np.errstate(over="ignore"):
                    wp = 1.0 / (1.0 + np.exp(D / kT))
                P0 = (1.0 - wp) * c2 + wp * (1.0 - c2)
                tol = TH.tol_occ(A, kT, 1.0)
                assert abs(P[0] - P0) <= tol and abs(P[1] - (1.0 - P0)) <= tol and abs(z - wp) <= tol_ztail(A, kT), (eps, t, kT)
                assert abs(np.sort(lam)[1] - np.sort(lam)[0] - D) <= 1e-12 * EC.hnorm(A)


def test_degenerate_lowest_pair_one_state_and_bad_arguments():
    # an exactly doubly degenerate lowest pair, as a diagonal with a repeat: the two populations are bitwise equal
    for off in (0.0, 4096.0):
        d = np.array([0.75, 0.25, 1.5, 0.25, 3.0, 7.0]) + off
        for kT in (1e-3, 0.1, 10.0):
            _, P, _, _, _ = solve(np.diag(d), kT)
            assert P[1] == P[3] and P[1] > 0, (off, kT, P)
            if kT == 1e-3:
                assert P[1] == 0.5
    # two identical disconnected 2 x 2 blocks: the same populations twice, bit for bit (the same rotations on the same entries)
    B = np.array([[0.3, -0.7], [-0.7, 1.1]])
    _, P, _, _, _ = solve(np.kron(np.eye(2), B), 0.4)
    assert P[0] == P[2] and P[1] == P[3]
    # one state: P = 1 exactly
    for a in (0.0, -3.5, 1e5):
        sweeps, P, lam, V, z = solve(np.array([[a]]), 0.01)
        assert sweeps == 0 and P[0] == 1.0 and lam[0] == a and V[0, 0] == 1.0 and z == 1.0
    L = thermal_lib()
    z8 = np.zeros(40 * 40)
    args = [H._p(z8, ctypes.c_double)] * 4
    assert L.qdht_thermal(33, H._p(np.zeros(33 * 17), ctypes.c_double), 1.0, *args) == -1
    for kT in (0.0, -1.0, np.inf, np.nan):
        assert L.qdht_thermal(4, H._p(np.zeros(10), ctypes.c_double), kT, *args) == -1


def test_workspace_fits_the_stated_budget():
    """sizeof(QdThermalWs) is at most the figure of the header comment, which is the one the comment's seven blocks per CU rest on"""
    L = thermal_lib()
    hdr = open(os.path.join(H.ROOT, "rl-agent-for-qubit-array-tuning_amd", "csrc", "qd_thermal.h")).read()
    stated = int(re.search(r"sizeof\(QdThermalWs\) = ([\d ]+) B", hdr).group(1).replace(" ", ""))
    assert stated == WS_BYTES and L.qdht_ws_bytes() <= stated
    assert 7 * stated <= 160 * 1024 < 8 * stated
    assert L.qdht_sweep_cap() == int(re.search(r"#define QD_TH_SWEEPS (\d+)", hdr).group(1))


# ------------------------------------------------------------------ the record path
@pytest.mark.parametrize("N,K", [(2, 32), (3, 32), (4, 32), (8, 32), (8, 20), (3, 8), (8, 8)])
def test_moments_of_a_record_against_the_oracles_hamiltonian(N, K):
    """the record path of qd_k_thermal (block of the record, core, occupations and variances) on the oracle's kept lists, short
    lists with |0..0> padding among them, against the reference; and with all couplings zero against the classical sums"""
    rng = np.random.default_rng(200 * N + K)
    eb = H.sample_blocks(N, [61, 62])
    lay = H.layout(N)
    worst, short = 0.0, 0
    for e in range(2):
        par = eb.params[e]
        dev = H.dev_view(N, par)
        n = 16
        vg = par[lay.vopt:lay.vopt + N + 1] + rng.uniform(-4, 4, (n, N + 1))
        if N <= 3:
            vg[: n // 2] -= 8.0                                 # towards the empty array: short lists
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
            for cut in (False, True):
                t = np.zeros(N - 1) if cut else np.ascontiguousarray(tc[p])
                Hm = np.diag(F[p, :nv]) + (0.0 if cut else Ht[p, :nv, :nv])
                w = np.linalg.eigvalsh(Hm)
                for kT in ((w[1] - w[0]) if nv > 1 and w[1] > w[0] else 0.1, 8.617333262145e-5 * 100):
                    pop, occ, var, z = np.zeros(32), np.zeros(N), np.zeros(N), np.zeros(1)
                    got = thermal_lib().qdht_record(N, H._p(idx, ctypes.c_uint16), H._p(np.ascontiguousarray(floors[p]), ctypes.c_int32),
                                                    H._p(t, ctypes.c_double), H._p(E, ctypes.c_double), nv, K, kT,
                                                    H._p(pop, ctypes.c_double), H._p(occ, ctypes.c_double), H._p(var, ctypes.c_double),
                                                    H._p(z, ctypes.c_double))
                    assert got == nv and not pop[nv:].any()
                    o, v, zr, to, tv, tz, P, _ = TH.point_reference(Hm, states[p, :nv], kT)
                    r = max(np.abs(occ - o).max() / to, np.abs(var - v).max() / tv, abs(z[0] - zr) / tz, np.abs(pop[:nv] - P).max() / to)
                    assert r <= 1.0 and var.min() >= 0.0, (N, K, e, p, cut, kT, r)
                    worst = max(worst, float(r))
    print(f"[thermal cpu] record path N={N} K={K}: worst err / tol {worst:.2e}")
    if N <= 3 and K == 32:
        assert short > 0, "no short list among the points"


# ------------------------------------------------------------------ the C entry point without a device
def test_prototype_and_struct_match_the_header():
    _lib, L = _built_lib()
    hdr = open(os.path.join(H.ROOT, "include", "qdsim.h")).read()
    assert "qd_eval_points_thermal" in _lib.EXPORTS and hasattr(L, "qd_eval_points_thermal")
    m = re.search(r"\bint qd_eval_points_thermal\((.*?)\);", hdr, re.S)
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    fn = L.qd_eval_points_thermal
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(decl) == 11
    assert fn.argtypes[9]._type_ is _lib.QdThermalOpts and decl[9].startswith("const qd_thermal_opts*")
    assert decl[6].startswith("const double* kT_host")
    body = re.search(r"typedef struct qd_thermal_opts \{(.*?)\} qd_thermal_opts;", hdr, re.S).group(1)
    names = [ln.split(";")[0].split()[-1].lstrip("*") for ln in body.strip().splitlines()]
    assert names == [f[0] for f in _lib.QdThermalOpts._fields_]
    assert ctypes.sizeof(_lib.QdThermalOpts) == 40
    assert ctypes.sizeof(_lib.QdPointsOpts) == 48                      # (the sibling's struct is as it was)


def test_argument_checks_need_no_device():
    _lib, L = _built_lib()
    B = 3
    one = ctypes.c_void_p(64)                          # a device pointer that is never dereferenced
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)     # noqa: E731
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)     # noqa: E731
    f64 = lambda *v: (ctypes.c_double * len(v))(*v)    # noqa: E731

    def opts(**kw):
        o = _lib.QdThermalOpts(struct_size=ctypes.sizeof(_lib.QdThermalOpts), var_dst=64, ztail_dst=64)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(h, o, env=i32(0), start=i64(0, 1), ng=1, kT=f64(0.01), sig=one, occ=one):
        return L.qd_eval_points_thermal(h, env, start, ng, one, one, kT, sig, occ, None if o is None else ctypes.byref(o), None)

    assert call(None, opts()) == _lib.QD_ERR_ARG
    h = _handle(L, 4, 8, B)
    try:
        for bad in (0.0, -1.0, float("inf"), float("nan"), -0.0):
            assert call(h, opts(), kT=f64(bad)) == _lib.QD_ERR_ARG, bad
            msg = L.qd_last_error(h)
            assert msg.startswith(b"qd_eval_points_thermal") and b"kT" in msg, msg
            assert call(h, None, kT=f64(bad)) == _lib.QD_ERR_ARG
        assert call(h, opts(), env=i32(0, 1), start=i64(0, 1, 2), ng=2, kT=f64(0.01, 0.0)) == _lib.QD_ERR_ARG      # every group's
        assert call(h, opts(), kT=None) == _lib.QD_ERR_ARG and b"kT_host" in L.qd_last_error(h)
        assert call(h, opts(struct_size=48)) == _lib.QD_ERR_ARG and b"struct_size" in L.qd_last_error(h)
        # the checks of the shared loop, under the new name
        assert call(h, opts(), env=i32(B)) == _lib.QD_ERR_ARG and b"qd_eval_points_thermal: env id" in L.qd_last_error(h)
        assert call(h, opts(), start=i64(2, 1)) == _lib.QD_ERR_ARG and b"qd_eval_points_thermal" in L.qd_last_error(h)
        assert call(h, opts(n_charge_host=i32(-1))) == _lib.QD_ERR_ARG and b"0..32767" in L.qd_last_error(h)
        assert call(h, None, ng=-1) == _lib.QD_ERR_ARG
        # groups without a point: nothing to do, with or without options or outputs
        assert call(h, opts(), start=i64(3, 3)) == 0 and call(h, None, start=i64(3, 3)) == 0
        assert call(h, opts(), start=i64(3, 3), sig=None, occ=None) == 0
        assert call(h, opts(n_charge_host=i32(2)), start=i64(3, 3)) == 0
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
            assert L.qd_last_error(hs).startswith(b"qd_eval_points_thermal")
            assert call(hs, opts(), kT=f64(0.0)) == _lib.QD_ERR_ARG                          # arguments first
        finally:
            L.qd_destroy(hs)


# ------------------------------------------------------------------ the Python layer
def test_python_layer_checks_kt_before_the_device():
    from qadapt_hip.env import ModelFacade
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    sig = inspect.signature(VecQuantumDeviceEnv.eval_points).parameters
    assert sig["kT"].default is None and sig["kT"].kind is inspect.Parameter.KEYWORD_ONLY and sig["levels"].default == 0

    class Stub:
        def __init__(self, T):
            self.calls = []
            self._T_host = np.array([T])

        def eval_points(self, env_ids, vg, vb, gamma=None, outputs=("signal", "occupations"), n_charge=None, states=False, *,
                        kT=None, levels=0):
            self.calls.append(dict(outputs=tuple(outputs), n_charge=n_charge, kT=kT, gamma=gamma))
            m = np.asarray(vg).shape[1]
            return {"signal": np.zeros((1, m)), "occupations": np.ones((1, m, N)), "variance": np.full((1, m, N), 0.25)}

    N = 4
    model = ModelFacade(Stub(120.0), N)
    model.coulomb_peak_width = 0.3
    assert model.T == 120.0
    for lead in ((), (5,), (3, 7)):
        vg, vb = np.zeros(lead + (N + 1,)), np.zeros(lead + (N - 1,))
        s, n, v = model.thermal_state_open(vg, vb)
        assert s.shape == lead + (1,) and n.shape == v.shape == lead + (N,) and s.dtype == n.dtype == v.dtype == np.float64
        assert model._b.calls[-1] == dict(outputs=("signal", "occupations", "variance"), n_charge=None,
                                          kT=8.617333262145e-5 * 120.0, gamma=0.3)
        model.thermal_state_open(vg, vb, T=77.0)
        assert model._b.calls[-1]["kT"] == 8.617333262145e-5 * 77.0                          # the reference's line, literally
        s, n, v = model.thermal_state_closed(vg, 3, T=50.0, vb=vb)
        assert s.shape == lead + (1,) and model._b.calls[-1]["n_charge"] == 3 and model._b.calls[-1]["kT"] == 8.617333262145e-5 * 50.0
    with pytest.raises(NotImplementedError):
        model.thermal_state_open(np.zeros(N + 1))
    with pytest.raises(ValueError):
        model.thermal_state_open(np.zeros(N + 1), np.zeros(N))
    raw = ModelFacade(Stub(np.nan), N)                                                        # a device loaded from raw blocks
    with pytest.raises(ValueError, match="raw"):
        raw.thermal_state_open(np.zeros(N + 1), np.zeros(N - 1))
    assert raw.thermal_state_open(np.zeros(N + 1), np.zeros(N - 1), T=100.0)[1].shape == (N,)


def test_sampled_temperature_is_kept_and_no_draw_moves():
    """extras["T"] is the value the draw plan always drew (qarray_config T: 50..200); the plan itself, and with it every other
    draw of a seed, is where it was"""
    from qadapt_hip import device_model as DM
    N = 4
    sampler = DM.DeviceSampler(N, DM.load_yaml(None, "qarray_config.yaml"), DM.load_yaml(None, "env_config.yaml"))
    plan = sampler.plan
    names = list(plan.slices)
    assert names.index("T") == names.index("vpw_alpha") + 1 == names.index("coulomb_peak_width") - 1
    sl = plan.slices["T"]
    assert sl.stop - sl.start == 1 and (plan.lo[sl][0], plan.hi[sl][0]) == (50.0, 200.0)
    u = np.random.default_rng(5).random((3, sampler.n_draws))
    eb = sampler.build(u)
    assert np.array_equal(eb.extras["T"], 50.0 + 150.0 * u[:, sl.start]) and eb.extras["T"].shape == (3,)
    u2 = u.copy(); u2[:, sl.start] = 0.5                                                     # T moves nothing else
    eb2 = sampler.build(u2)
    assert np.array_equal(eb.params, eb2.params) and np.array_equal(eb.state, eb2.state)
    ref = H.sample_blocks(N, [41])                                                           # the suite's devices, by seed
    assert ref.params.shape[1] == eb.params.shape[1]


def test_sanitizer_program_runs_clean():
    """the core and the record path under AddressSanitizer and UBSan, as a stand-alone program in a child process"""
    subprocess.check_call(["make", "-s", "-C", HDIR, "qd_thermal_asan"])
    r = subprocess.run([os.path.join(HDIR, "qd_thermal_asan")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "thermal asan ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


def test_worst_figures_are_reported():
    print(f"[thermal cpu] worst over the families run in this session: err / tol populations {_WORST['pop']:.2e}, ztail "
          f"{_WORST['ztail']:.2e}; residual {_WORST['resid']:.2e} ||A||_inf, orthogonality {_WORST['orth']:.2e}, "
          f"sweeps {_WORST['sweeps']} of {thermal_lib().qdht_sweep_cap()}")
    assert _WORST["pop"] <= 1.0 and _WORST["ztail"] <= 1.0
