"""Shared by test_gpu_update_kernel.py: a bare handle that reaches qd_k_update alone (qd_load_episodes / qd_set_state, then
qd_update_capacitance: no observation), the float32 updater fixture grouped by dot count, the matrix families of the
pseudo-inverse and of the ground-truth solve, and their extended-precision references (mpmath when it imports, numpy
otherwise).  Everything here but `Handle` runs without a GPU."""
import ctypes
import functools
import os

import numpy as np

import helpers as H
from qadapt_hip import device_model as DM
from qadapt_hip.layout import layout

try:
    import mpmath as mp
except ImportError:                                       # the references fall back to numpy
    mp = None

EPS = 2.0 ** -52
R_UPDATE = 8
MP_DIGITS = 50

# ---------------------------------------------------------------------------------------------------------------------
# The bars.  `ratio` is err / (kappa_2 * EPS * ||ref||_2) against the extended-precision reference.
#   pseudo-inverse: np.linalg.pinv(rcond=1e-15) itself reaches at worst 5.123 on the families below (measure_numpy_pinv(),
#                   G = 3..9, 154 matrices; worst at "dup_column_tiny" of G = 6).  The device gets 8 times that: a Jacobi method
#                   with another rotation order is a different algorithm of the same stability class, a wrong schedule or
#                   cut-off is wrong by orders of magnitude.  The device's own worst ratio, measured on an MI355X: 2.175
#                   ("dup_column_huge", G = 3).
#   solve:          np.linalg.solve reaches at worst 0.1262 (measure_numpy_solve(), G = 3..9, 49 systems; worst at
#                   "zero_leading_pivot" of G = 9), the device again 8 times that; its own worst measured: 0.0653.
# ---------------------------------------------------------------------------------------------------------------------
NUMPY_PINV_WORST = 5.123
C_PINV = 8 * NUMPY_PINV_WORST
NUMPY_SOLVE_WORST = 0.1262
C_SOLVE = 8 * NUMPY_SOLVE_WORST


# ---------------------------------------------------------------------------------------------------------------- handle
class Handle:
    """qd_create with the package's default configs; update_method "kalman" / "direct" / "perfect" / None, 3 or 2 outputs;
    variance_threshold / process_noise: the capacitance_model knobs of env_config.yaml (defaults 0.05 / 0)"""

    def __init__(self, N, B, method="kalman", n_out=3, R=R_UPDATE, variance_threshold=None, process_noise=None):
        import torch
        from qadapt_hip import _lib
        from qadapt_hip.vec_env import make_qd_config
        self.torch, self._libmod = torch, _lib
        cfg = DM.load_yaml(None, "env_config.yaml"); q = DM.load_yaml(None, "qarray_config.yaml")
        cm = cfg["capacitance_model"]
        cm["update_method"] = method; cm["nearest_neighbour"] = n_out == 2
        assert (cm["variance_threshold"], cm["process_noise"]) == (0.05, 0.0)      # the fixture's constructor arguments
        if variance_threshold is not None:
            cm["variance_threshold"] = float(variance_threshold)
        if process_noise is not None:
            cm["process_noise"] = float(process_noise)
        self.N, self.B, self.C, self.K, self.G, self.L = N, B, N - 1, n_out, N + 1, layout(N)
        self.lib = _lib.lib()
        qc = make_qd_config(cfg, q, N, R, B)
        assert (qc.kalman_prior_mean, qc.kalman_prior_variance, qc.kalman_prior_mean_nnn) == (0.3, 0.5, 0.15)
        self.h = ctypes.c_void_p()
        rc = self.lib.qd_create(ctypes.byref(qc), torch.cuda.current_device(), ctypes.byref(self.h))
        if rc != 0:
            msg = self.lib.qd_last_error(self.h).decode() if self.h else "no handle"
            if self.h:
                self.lib.qd_destroy(self.h)
            self.h = None
            raise _lib.QdError(f"qd_create failed (code {rc}): {msg}")

    def stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def load(self, params, state, reset_kalman=1):
        """parameter and state rows of all B envs; reset_kalman: the Kalman block returns to its priors"""
        params = np.ascontiguousarray(params, np.float64); state = np.ascontiguousarray(state, np.float64)
        assert params.shape == (self.B, self.L.size) and state.shape == (self.B, self.L.s_size)
        ids = np.arange(self.B, dtype=np.int32)
        rc = self.lib.qd_load_episodes(self.h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), self.B,
                                       params.ctypes.data, state.ctypes.data, int(reset_kalman), self.stream())
        self._libmod.check(self.h, rc, "qd_load_episodes")

    def get_state(self):
        st = np.zeros((self.B, self.L.s_size))
        self._libmod.check(self.h, self.lib.qd_get_state(self.h, st.ctypes.data, None), "qd_get_state")
        return st

    def set_state(self, st):
        st = np.ascontiguousarray(st, np.float64)
        assert st.shape == (self.B, self.L.s_size)
        self._libmod.check(self.h, self.lib.qd_set_state(self.h, st.ctypes.data, None), "qd_set_state")

    def update(self, values=None, log_vars=None, ids=None, n=None, recompute=1):
        """qd_update_capacitance; values / log_vars (B, C, K) float32 indexed by env id, or None; ids: env ids or None"""
        torch = self.torch
        keep = []
        vp = lp = ip = None
        if values is not None:
            for a in (values, log_vars):
                a = np.ascontiguousarray(a, np.float32)
                assert a.shape == (self.B, self.C, self.K)
                keep.append(torch.from_numpy(a).cuda())
            vp, lp = (ctypes.c_void_p(t.data_ptr()) for t in keep)
        cnt = 0
        if ids is not None:
            ids = np.ascontiguousarray(ids, np.int32)
            assert ids.ndim == 1 and ids.size >= 1 and ids.min() >= 0 and ids.max() < self.B
            cnt = ids.size if n is None else int(n)
            assert 0 <= cnt <= ids.size
            keep.append(torch.from_numpy(ids).cuda())
            ip = ctypes.c_void_p(keep[-1].data_ptr())
        rc = self.lib.qd_update_capacitance(self.h, ip, cnt, vp, lp, int(recompute), self.stream())
        self._libmod.check(self.h, rc, "qd_update_capacitance")
        torch.cuda.synchronize()                               # `keep` outlives the launch

    def close(self):
        if self.h:
            self.lib.qd_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def views(L, st):
    """(means (n,N,N), variances (n,N,N), vgm (n,G,G), gate_gt (n,N), barrier_gt (n,N-1), sensor_gt (n,)) of state rows"""
    N, G = L.N, L.G
    return (st[:, L.s_kmean:L.s_kmean + N * N].reshape(-1, N, N), st[:, L.s_kvar:L.s_kvar + N * N].reshape(-1, N, N),
            st[:, L.s_vgm:L.s_vgm + G * G].reshape(-1, G, G), st[:, L.s_gate_gt:L.s_gate_gt + N],
            st[:, L.s_barrier_gt:L.s_barrier_gt + N - 1], st[:, L.s_sensor_gt])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def blocks(N, B, seed0=700):
    """B sampled devices of N dots: (params (B, L.size), state (B, L.s_size)), read-only"""
    eb = H.sample_blocks(N, [seed0 + 10 * N + k for k in range(B)])
    p, s = np.array(eb.params, np.float64), np.array(eb.state, np.float64)
    p.setflags(write=False); s.setflags(write=False)
    return p, s


# --------------------------------------------------------------------------------------------------------------- fixture
@functools.lru_cache(maxsize=None)
def fixture():
    g = np.load(os.path.join(H.ROOT, "tests", "golden", "updater_traces_f32.npz"))
    cases = {}
    for c in range(int(g["n_cases"])):
        d = {k: g[f"c{c}_{k}"] for k in ("values", "log_vars", "means", "variances", "full", "accepted", "rejected")}
        cases[(int(g[f"c{c}_n_dots"]), str(g[f"c{c}_kind"]), d["values"].shape[-1])] = d
    return cases


def fixture_like_inputs(rng, shape):
    """the fixture's input distribution (make_golden.updater_traces_f32), as float32"""
    v = rng.normal(0.0, 0.1, size=shape)
    v[rng.random(shape) < 0.05] *= 40.0
    return v.astype(np.float32), rng.uniform(-8.0, 3.0, size=shape).astype(np.float32)


# ------------------------------------------------------------------------------------------- extended-precision references
def product(cdd_inv, means):
    """cdd_inv_full @ (-E), E = [[estimate with unit diagonal, 0], [0, 1]], in the kernel's order of operations
    (one accumulator per entry, k ascending, no contraction): the float64 matrix qd_pinv_wave is given"""
    G = cdd_inv.shape[0]; N = G - 1
    E = np.zeros((G, G)); E[:N, :N] = means; E[np.arange(G), np.arange(G)] = 1.0
    out = np.zeros((G, G))
    for i in range(G):
        for j in range(G):
            acc = 0.0
            for k in range(G):
                acc = acc + cdd_inv[i, k] * (-E[k, j])
            out[i, j] = acc
    return out


def ref_pinv(M, digits=MP_DIGITS):
    """pseudo-inverse of the float64 matrix M with numpy.linalg.pinv's rule (singular values <= 1e-15 * s_max dropped) in
    extended precision: (P float64, singular values float64 descending, number kept).  numpy itself without mpmath."""
    M = np.asarray(M, np.float64); n = M.shape[0]
    if not M.any():
        return np.zeros_like(M), np.zeros(n), 0
    if mp is None:
        s = np.linalg.svd(M, compute_uv=False)
        return np.linalg.pinv(M, rcond=1e-15), s, int((s > 1e-15 * s[0]).sum())
    with mp.workdps(digits):
        # (scaled to s_max ~ 1 by a power of two, exactly: the SVD's own tolerances are absolute)
        e = int(np.floor(np.log2(np.abs(M).max())))
        A = mp.matrix(np.ldexp(M, -e).tolist())
        U, S, V = mp.svd_r(A)
        s = [S[i] for i in range(n)]
        keep = [i for i in range(n) if s[i] > mp.mpf("1e-15") * s[0]]
        P = mp.zeros(n, n)
        for i in keep:
            P += (V[i, :].T * U[:, i].T) / s[i]
        Pf = np.ldexp(np.array([[float(P[i, j]) for j in range(n)] for i in range(n)]), -e)
        sf = np.ldexp(np.array([float(x) for x in s]), e)
    return Pf, sf, len(keep)


def ref_solve(A, b, digits=MP_DIGITS):
    A = np.asarray(A, np.float64); b = np.asarray(b, np.float64)
    if mp is None:
        return np.linalg.solve(A, b)
    with mp.workdps(digits):
        x = mp.lu_solve(mp.matrix(A.tolist()), mp.matrix(b.tolist()))
        return np.array([float(v) for v in x])


def pinv_ratio(P, case):
    """|| P - P_ref ||_2 / (kappa_2 EPS || P_ref ||_2); for a zero reference: 0 if P is zero, else inf"""
    if case["rank"] == 0:
        return 0.0 if not np.asarray(P).any() else np.inf
    if not np.isfinite(P).all():
        return np.inf
    return float(np.linalg.norm(P - case["ref"], 2) / (case["kappa"] * EPS * np.linalg.norm(case["ref"], 2)))


# ------------------------------------------------------------------------------------------------------ pinv families
def _graded(rng, n, kappa):
    q1, _ = np.linalg.qr(rng.normal(size=(n, n))); q2, _ = np.linalg.qr(rng.normal(size=(n, n)))
    return q1 @ np.diag(np.logspace(0, -np.log10(kappa), n)) @ q2.T


def _grid(rng, n):
    """random entries on a 2^-12 grid: sums of two rows are exact, so a dependent row is dependent in float64 as well"""
    return np.round(rng.normal(size=(n, n)) * 4096) / 4096


GRADED = (1e2, 1e4, 1e8, 1e12, 1e13)       # 1e13: a kept singular value well inside (1e-15, 1e-12) * s_max, where a wrong
                                           # cut-off shows; at 1e12 the smallest one sits on 1e-12 * s_max


@functools.lru_cache(maxsize=None)
def pinv_cases(G):
    """The matrices qd_pinv_wave<G> is given, G = N + 1 = 3..9: dicts of name, `target` (the float64 product), how to get it
    (`cdd_inv` to load and Kalman `means` to set, all updates rejected), `deficient`, and the extended-precision
    reference (`ref`, singular values `sv`, `rank`, `kappa` over the kept ones)."""
    N = G - 1
    rng = np.random.default_rng([314, G])
    fam = []

    def direct(name, M, deficient=False):
        # E = I: the product is exactly -cdd_inv, so cdd_inv = -target
        fam.append(dict(name=name, target=np.array(M, np.float64), cdd_inv=-np.array(M, np.float64), means=np.zeros((N, N)),
                        deficient=deficient))

    direct("random", rng.normal(size=(G, G)))
    for kap in GRADED:
        direct(f"graded_{kap:.0e}", _graded(rng, G, kap))
    A = _grid(rng, G); A[:, -1] = A[:, 0]; direct("dup_column", A, True)
    A = _grid(rng, G); A[-1, :] = A[0, :] + A[1, :]; direct("dep_row", A, True)
    A = _grid(rng, G); A[:, 1] = 0.0; direct("zero_column", A, True)
    direct("zero", np.zeros((G, G)), True)
    for tag, s in (("tiny", 1e-60), ("huge", 1e+60)):
        # (entrywise scaling keeps equal columns equal and zeros zero; a dependent row would not survive the rounding)
        for name in ("random", "graded_1e+08", "dup_column", "zero_column", "zero"):
            base = next(c for c in fam if c["name"] == name)
            direct(f"{name}_{tag}", base["target"] * s, base["deficient"])
    for c in fam:
        _reference(c)
    # physically reachable: clamped means make the estimate singular, on a sampled device's real cdd_inv
    L = layout(N)
    one = np.zeros((N, N))                                  # one pair at 1, the other tracked pairs at their priors ...
    for i in range(N - 1):
        one[i, i + 1] = one[i + 1, i] = 0.3
    for i in range(N - 2):
        one[i, i + 2] = one[i + 2, i] = 0.15
    one[0, 1] = one[1, 0] = 1.0
    if N >= 3:                                              # ... but for the two that keep columns 0 and 1 of E from being
        one[0, 2] = one[2, 0] = one[1, 2]                   # equal: (0, 2) = (1, 2), and (1, 3) = 0 as the untracked (0, 3)
    if N >= 4:
        one[1, 3] = one[3, 1] = 0.0
    every = np.zeros((N, N))                                # all tracked pairs at 1
    for i in range(N):
        for j in range(N):
            if i != j and abs(i - j) <= 2:
                every[i, j] = 1.0
    for name, m in (("clamped_one_pair", one), ("clamped_all_pairs", every)):
        # E is singular exactly, its float64 product with cdd_inv only nearly: the device is drawn again until the
        # product meets the input condition of the rank-deficient families (check_pinv_case_conditions)
        for seed0 in range(700, 740):
            par, _ = blocks(N, 1, seed0)
            cdd = par[0, L.cdd_inv:L.cdd_inv + G * G].reshape(G, G).copy()
            c = dict(name=name, target=product(cdd, m), cdd_inv=cdd, means=m, deficient=None)
            _reference(c)
            c["deficient"] = c["rank"] < G                  # (all pairs at 1 is singular for some N only)
            try:
                check_pinv_case_conditions(c)
            except AssertionError:
                continue
            fam.append(c)
            break
        else:
            raise RuntimeError(f"no sampled device meets the input condition: G = {G}, {name}")
    return tuple(fam)


def _reference(c):
    c["ref"], c["sv"], c["rank"] = ref_pinv(c["target"])
    c["kappa"] = float(c["sv"][0] / c["sv"][c["rank"] - 1]) if c["rank"] else 0.0


def check_pinv_case_conditions(c):
    """rank-deficient families: discarded singular values below 2.5e-17 * s_max, kept ones above 1e-13 * s_max -- the
    cut-off is then not decided by rounding"""
    G = c["target"].shape[0]
    if not c["deficient"]:
        assert c["rank"] == G, c["name"]
        return
    assert c["rank"] < G, c["name"]
    if c["rank"] == 0:
        return
    sv, smax = c["sv"], c["sv"][0]
    assert np.all(sv[c["rank"]:] < 2.5e-17 * smax), (c["name"], sv / smax)
    assert np.all(sv[:c["rank"]] > 1e-13 * smax), (c["name"], sv / smax)


def measure_numpy_pinv():
    """worst pinv_ratio of np.linalg.pinv(rcond=1e-15) over every family and G: the figure NUMPY_PINV_WORST records"""
    worst = (0.0, None)
    for G in range(3, 10):
        for c in pinv_cases(G):
            check_pinv_case_conditions(c)
            r = pinv_ratio(np.linalg.pinv(c["target"], rcond=1e-15), c)
            worst = max(worst, (r, (G, c["name"])))
    return worst


# ------------------------------------------------------------------------------------------------------ solve families
@functools.lru_cache(maxsize=None)
def solve_cases(G):
    """VGMs for the ground-truth solve alone: dicts of name, `vgm`, `singular`"""
    rng = np.random.default_rng([2171, G])
    fam = []
    A = rng.normal(size=(G, G)); A[0, 0] = 0.0
    fam.append(dict(name="zero_leading_pivot", vgm=A))
    perm = rng.permutation(G)
    for _ in range(G):                                      # no row stays in place: every column needs its swap
        if not (perm == np.arange(G)).any():
            break
        perm = np.roll(perm, 1)
    else:
        perm = np.roll(np.arange(G), 1)
    fam.append(dict(name="permuted_diagonal", vgm=np.eye(G)[perm] @ np.diag(rng.uniform(0.5, 2.0, G) * rng.choice([-1, 1], G))))
    for kap in (1e2, 1e6, 1e10):
        fam.append(dict(name=f"graded_{kap:.0e}", vgm=_graded(rng, G, kap)))
    fam.append(dict(name="identity", vgm=-np.eye(G)))                       # O.identity_vgm: the electrons sign
    fam.append(dict(name="plain", vgm=rng.normal(size=(G, G)) - 2 * np.eye(G)))
    A = rng.normal(size=(G, G)); A[1, :] = 0.0
    fam.append(dict(name="singular", vgm=A, singular=True))
    for c in fam:
        c.setdefault("singular", False)
        c["vgm"] = np.ascontiguousarray(c["vgm"], np.float64)
        if not c["singular"]:
            s = np.linalg.svd(c["vgm"], compute_uv=False)
            c["kappa"] = float(s[0] / s[-1])
    return tuple(fam)


def solve_rhs(L, par):
    return par[L.vopt:L.vopt + L.G] - par[L.origin:L.origin + L.G]


def measure_numpy_solve():
    """worst || x_numpy - x_ref ||_2 / (kappa_2 EPS || x_ref ||_2) over the solve families, G = 3..9, on the right-hand
    sides the device test uses: the figure NUMPY_SOLVE_WORST records"""
    worst = (0.0, None)
    for G in range(3, 10):
        N = G - 1; L = layout(N)
        par, _ = blocks(N, len(solve_cases(G)))
        for k, c in enumerate(solve_cases(G)):
            if c["singular"]:
                continue
            b = solve_rhs(L, par[k])
            x = ref_solve(c["vgm"], b)
            r = float(np.linalg.norm(np.linalg.solve(c["vgm"], b) - x) / (c["kappa"] * EPS * np.linalg.norm(x)))
            worst = max(worst, (r, (G, c["name"])))
    return worst
