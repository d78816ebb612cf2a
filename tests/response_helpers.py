"""Reference, families and tolerance of the charge-response tests, one source for both tiers (tests/test_response_cpu.py through
the host build of csrc/qd_response.h, tests/test_gpu_response_device.py and tests/test_gpu_response.py through the device).

Reference, per point, in float64 and independent of the kernels: Hs = H - min(diag H) I, w, V = numpy.linalg.eigh(Hs),
p = softmax(-w / kT), and for a perturbation X and the occupation observables (diagonal in the charge basis)
    G = V^T X V,   D_aa = -p_a / kT,   D_ab = -p_lo phi(x) / kT,  x = |w_a - w_b| / kT,  phi(x) = -expm1(-x) / x,  phi(0) = 1
    dP = diag(V (D o G) V^T) + P <X> / kT,   <X> = sum_a p_a G_aa,   chi[i][X] = sum_m n_m[i] dP_m
Lam and Gam of the chain rule come from the oracle device's cdd_inv_full, cgd_full, Cbg and alpha (`chain`).

Tolerance, per point, with the notation of thermal_helpers (hs = ||Hs||_inf, hn = ||H||_inf, g = w[1] - w[0], n_max the largest
occupation):
    tol_chi = 8 n_max^2 (1e-12 hs + 1e-13 hn) min(1 / kT, 1 / g)^2 + 1e-12 n_max^2 / kT
the ln tc columns carry ||T_d||_inf in place of one n_max; tol_jac and tol_dsignal follow by the triangle inequality through
|Lam|, |Gam| and |S'|:  tol_jac = tol_chi_n |Lam| + tol_chi_t |Gam|,  tol_dsignal = |S'| 2 sum_i |A[N][i]| tol_jac
+ (20 / gamma^2) tol_c0 |dc0/dv| + 64 eps |S' dc0/dv|.  The middle term is there because the device evaluates the slope at its own
c0, whose error the occupations' tolerance bounds (tol_c0 = 2 sum_i |A[N][i]| tol_occ) and |S''| <= 2 / gamma^2 per peak, ten peaks;
the last one is the rounding of the ten-term sum itself.  The 8 is the thermal tests' 4 times 2 for the second spectral factor, the square is the order of the
divided difference.  The form is pinned against mpmath at 50 digits in tests/test_response_cpu.py before anything runs on a
device.  Every point is compared."""
import numpy as np

import eig_cases as EC
import qd_oracle as O
import thermal_helpers as TH

NONE = 255


# ------------------------------------------------------------------ the formula
def phi(x):
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        return np.where(x > 0, -np.expm1(-x) / np.where(x > 0, x, 1.0), 1.0)


def decompose(Hm, kT):
    """(w, V, p, D) of one dense symmetric block"""
    s = Hm.shape[0]
    Hs = Hm - np.min(np.diag(Hm)) * np.eye(s)
    w, V = np.linalg.eigh(Hs)
    with np.errstate(under="ignore"):
        p = TH.softmax(-w / kT)
        x = np.abs(w[:, None] - w[None, :]) / kT
        plo = np.where(w[:, None] <= w[None, :], p[:, None], p[None, :])
        D = -plo * phi(x) / kT
    D[np.diag_indices(s)] = -p / kT
    return w, V, p, D


def dpop(V, p, D, kT, X):
    """d P_m / d eps for H + eps X (dense symmetric X)"""
    with np.errstate(under="ignore"):
        G = V.T @ X @ V
        M = D * G
        P = (V * V) @ p
        return np.einsum("ma,ab,mb->m", V, M, V) + P * float(p @ np.diag(G)) / kT


def chi_reference(Hm, kT, nt, Xs):
    """chi (No, len(Xs)) for the occupation table nt (s, No) and the dense perturbations Xs"""
    _, V, p, D = decompose(Hm, kT)
    nt = np.asarray(nt, np.float64)
    return np.stack([nt.T @ dpop(V, p, D, kT, X) for X in Xs], axis=1)


def spectral_factor2(Hm, kT):
    """(1e-12 hs + 1e-13 hn) min(1 / kT, 1 / g)^2"""
    s = Hm.shape[0]
    Hs = Hm - np.min(np.diag(Hm)) * np.eye(s)
    cond = 1.0 / kT
    if s > 1:
        w = np.linalg.eigvalsh(Hs)
        g = w[1] - w[0]
        if g > 0:
            cond = min(cond, 1.0 / g)
    return (1e-12 * TH.hnorm(Hs) + 1e-13 * TH.hnorm(Hm)) * cond * cond


def tol_chi(Hm, kT, n_max, xnorms):
    """per column: xnorms[c] is n_max for an on-site column and ||T_d||_inf for a ln tc column"""
    n_max = max(float(n_max), 1.0)
    # (a column of a perturbation that is zero has the tolerance zero and must be zero: the floor keeps 0 / 0 out of the ratios)
    return np.maximum((8.0 * spectral_factor2(Hm, kT) + 1e-12 / kT) * n_max * np.asarray(xnorms, np.float64), 5e-324)


# ------------------------------------------------------------------ sparse perturbations, as the core takes them
def hop_tables(T):
    """(nb (s, 2) uint8, coef (s, 2)) of a symmetric T with at most two entries per row off the diagonal"""
    s = T.shape[0]
    nb, cf = np.full((s, 2), NONE, np.uint8), np.zeros((s, 2))
    for m in range(s):
        js = np.flatnonzero(T[m])
        assert len(js) <= 2 and m not in js
        for k, j in enumerate(js):
            nb[m, k], cf[m, k] = j, T[m, j]
    return nb, cf


def chain(s, rng, scale=1.0, cut=()):
    """a chain m <-> m + 1 with random negative coefficients (links in `cut` left out)"""
    T = np.zeros((s, s))
    for m in range(s - 1):
        c = -scale * rng.uniform(0.3, 2.0)
        if m not in cut:
            T[m, m + 1] = T[m + 1, m] = c
    return T


def probe(s, seed):
    """the observables and perturbations every family block is probed with: nt (s, 3) occupations 0..3, two sparse patterns"""
    rng = np.random.default_rng(7000 + 37 * s + seed)
    nt = rng.integers(0, 4, (s, 3)).astype(np.float64)
    T1 = chain(s, rng)
    T2 = np.zeros((s, s))
    for m in range(0, s - 2, 3):
        T2[m, m + 2] = T2[m + 2, m] = -rng.uniform(0.5, 1.5)
    return nt, [T1, T2]


def temperatures(A):
    """kT from 1e-6 hs to 1e3 hs (the low end makes the weights underflow)"""
    hs = TH.hnorm(A - np.min(np.diag(A)) * np.eye(A.shape[0]))
    hs = hs if hs > 0 else 1.0
    return [f * hs for f in (1e-6, 1e-3, 1e-1, 10.0, 1e3)]


def designed(s, kT=0.05):
    """(tag, A, kT) of the designed cases of size s >= 2 at a fixed kT"""
    rng = np.random.default_rng(8100 + s)
    out = []
    # exact degeneracy of the two lowest levels / of an excited pair, on the diagonal and inside coupled duplicate blocks
    d = np.sort(rng.integers(1, 40, s) / 16.0)
    d[1] = d[0]
    out.append(("deg lowest diag", np.diag(d.copy()), kT))
    if s >= 4:
        e = d.copy(); e[1] = e[0] + 0.25; e[3] = e[2] = e[1] + 0.5
        out.append(("deg excited diag", np.diag(e), kT))
        h = s // 2
        B = EC.hop_block(rng, h, 0.3)
        A = np.zeros((s, s)); A[:h, :h] = B; A[h:2 * h, h:2 * h] = B
        if s > 2 * h:
            A[s - 1, s - 1] = 9.0
        out.append(("deg every level, two equal blocks", A, kT))
    # level pairs at x = 1e-14, 1e-8, 1e-3: exact on the diagonal, and mixed by a rotation of the pair with its neighbour
    for x in (1e-14, 1e-8, 1e-3):
        e = np.arange(s, dtype=np.float64) * 0.07 + 1.0
        e[1] = e[0] + x * kT
        out.append((f"pair x={x:g} diag", np.diag(e), kT))
        A = np.diag(e)
        if s >= 3:
            A[0, 2] = A[2, 0] = -0.011
            A[1, 2] = A[2, 1] = -0.011
        out.append((f"pair x={x:g} coupled", A, kT))
    # denormal couplings
    A = np.diag(rng.uniform(0, 1, s))
    for m in range(s - 1):
        A[m, m + 1] = A[m + 1, m] = -5e-324 * (1 + m)
    out.append(("denormal tc", A, kT))
    return out


def family(s):
    """(tag, A, kT) over the blocks of size s: the eigen-solver families at five temperatures each, then the designed cases"""
    if s == 1:
        return [(("one state", a), np.array([[a]]), kT) for a in (0.0, -3.5, 1e5) for kT in (1e-3, 1.0)]
    fam = [(("hop", t), A) for t, A in list(EC.scale_family(s))[::3]]
    for sep in (1e-5, 3e-9):
        fam += [(("near", sep, tc), A) for tc, A, _ in EC.near_degenerate_family(s, sep)]
    fam += [(("mixed", k), A) for k, A in enumerate(EC.mixed_scale_family(s)) if k < 6]
    fam += [(("extreme", k), A) for k, A in enumerate(EC.extreme_scale_family(s, reps=6))]
    fam.append((("classical",), EC.classical_block(s)))
    out = [(tag, A, kT) for tag, A in fam for kT in temperatures(A)]
    return out + designed(s)


def kind(tag):
    """the family a block of `family` belongs to, for the per-family figures: hop, near, mixed, extreme, classical, designed"""
    return "designed" if isinstance(tag, str) else ("designed" if tag[0] == "one state" else tag[0])


def block_check(A, kT, nt, Ts, dP):
    """worst err / tol of chi = nt^T dP against the reference for the perturbations [diag(nt[:, k])] + Ts, and the properties:
    the on-site block symmetric and negative semidefinite to the tolerance.  dP: (No + len(Ts), s)."""
    No = nt.shape[1]
    Xs = [np.diag(nt[:, k]) for k in range(No)] + list(Ts)
    ref = chi_reference(A, kT, nt, Xs)
    got = nt.T @ np.asarray(dP).T
    n_max = max(float(nt.max()), 1.0)
    tol = tol_chi(A, kT, n_max, [n_max] * No + [max(TH.hnorm(T), 1e-300) for T in Ts])
    r = float((np.abs(got - ref) / tol[None, :]).max())
    cn = got[:, :No]
    r = max(r, float((np.abs(cn - cn.T) / tol[:No].max()).max()))
    r = max(r, float(np.linalg.eigvalsh(0.5 * (cn + cn.T)).max() / tol[:No].max()))
    return r


# ------------------------------------------------------------------ the chain rule and the signal, from the oracle's device
def chain_matrices(dev):
    """(Lam (N, 2N), Gam (N-1, 2N)) over v = (vg[0..N], vb[0..N-2])"""
    N = dev.n_dot
    A = np.asarray(dev.cdd_inv_full)[:N, :N]
    cgd = np.asarray(dev.cgd_full)[:N]
    Lam = -2.0 * A @ cgd
    dvb = np.concatenate([np.asarray(dev.Cbg)[:N - 1, :N + 1], np.eye(N - 1)], axis=1)
    Gam = -np.asarray(dev.alpha)[:N - 1, None] * dvb
    return Lam, Gam


def pair_matrices(tc, states):
    """T_d, d = 0 .. N-2, of one point: the pair-d part of the oracle's tunnel Hamiltonian at the point's own tc"""
    N = states.shape[1]
    out = []
    for d in range(N - 1):
        t = np.zeros_like(tc)
        t[d] = tc[d]
        with np.errstate(under="ignore"):
            out.append(O.tunnel_hamiltonian(t[None], states[None])[0])
    return out


def point_reference(dev, Hm, st, tc, kT, v_ext, gamma):
    """one point: dict(chi, jac, dsignal, occ, signal, tol_chi (2N-1,), tol_jac (2N,), tol_dsignal (2N,))"""
    N = dev.n_dot
    st = np.asarray(st, np.int64)
    nt = st.astype(np.float64)
    Ts = pair_matrices(np.asarray(tc, np.float64), st)
    Xs = [np.diag(nt[:, k]) for k in range(N)] + Ts
    chi = chi_reference(Hm, kT, nt, Xs)
    Lam, Gam = chain_matrices(dev)
    jac = chi[:, :N] @ Lam + chi[:, N:] @ Gam
    n_max = max(float(nt.max()), 1.0)
    tchi = tol_chi(Hm, kT, n_max, [n_max] * N + [TH.hnorm(T) for T in Ts])
    tjac = np.maximum(tchi[:N] @ np.abs(Lam) + tchi[N:] @ np.abs(Gam), 5e-324)          # (the floor: as in tol_chi)
    P, _, _ = TH.reference(Hm, kT)
    occ = P @ nt
    Af = np.asarray(dev.cdd_inv_full)
    cgd = np.asarray(dev.cgd_full)
    vpp = cgd @ v_ext
    a = Af[N, N]
    c0 = 2.0 * float(Af[N, :N] @ (occ - vpp[:N])) + a * (2.0 * (np.rint(vpp[N]) - vpp[N]) + 1.0)
    rr = (c0 + 2.0 * a * np.arange(-5, 5)) / gamma
    signal = float((1.0 / (rr * rr + 1.0)).sum())
    ds = float((-2.0 * rr / (gamma * (rr * rr + 1.0) ** 2)).sum())
    dc0 = 2.0 * Af[N, :N] @ (jac - cgd[:N]) - 2.0 * a * cgd[N]
    # |S''| <= 2 / gamma^2 per peak: the slope moves with the error of c0, which the occupations' own tolerance bounds
    to = TH.tol_occ(Hm, kT, n_max)
    tc0 = 2.0 * np.abs(Af[N, :N]).sum() * to
    tds_slope = abs(ds) * 2.0 * (np.abs(Af[N, :N]) @ np.broadcast_to(tjac, (N, 2 * N)))      # |S'| tol_dc0
    tds_c0 = 10 * 2.0 / gamma ** 2 * tc0 * np.abs(dc0)                                          # |dc0| tol_S'
    tds = tds_slope + tds_c0 + 64 * np.finfo(np.float64).eps * np.abs(ds * dc0)
    return dict(chi=chi, jac=jac, dsignal=ds * dc0, occ=occ, signal=signal, dc0=dc0, tol_chi=tchi, tol_jac=tjac, tol_dsignal=tds,
                tol_dsignal_c0_share=float((tds_c0 / tds).max()) if tds.min() > 0 else 0.0)


def empty_reference(dev, v_ext, gamma):
    """a point without a valid state counts as |0..0>: chi and the jacobian are zero exactly, dS/dv = S'(c0) dc0/dv at <n> = 0"""
    N = dev.n_dot
    Af, cgd = np.asarray(dev.cdd_inv_full), np.asarray(dev.cgd_full)
    vpp = cgd @ v_ext
    a = Af[N, N]
    c0 = 2.0 * float(Af[N, :N] @ (-vpp[:N])) + a * (2.0 * (np.rint(vpp[N]) - vpp[N]) + 1.0)
    rr = (c0 + 2.0 * a * np.arange(-5, 5)) / gamma
    ds = float((-2.0 * rr / (gamma * (rr * rr + 1.0) ** 2)).sum())
    return ds * (-2.0 * Af[N, :N] @ cgd[:N] - 2.0 * a * cgd[N])


def compare_points(tag, dev, Hs, states, nv, tcs, kT, vg, vb, gamma, chi, jac, dsignal, closed=False):
    """the module's bounds at every point, the symmetry and the sign of the on-site block, the column sums of a closed list;
    prints the worst err / tol first and returns it"""
    N = dev.n_dot
    kT = np.broadcast_to(np.asarray(kT, np.float64), (len(Hs),))
    worst = {"chi": 0.0, "jac": 0.0, "dsignal": 0.0, "sym": 0.0, "nsd": 0.0, "sum": 0.0}
    share = 0.0
    for p, Hm in enumerate(Hs):
        if Hm is None:                                  # no valid state: zeros exactly, the signal's slope to the rounding of its sums
            want = empty_reference(dev, np.concatenate([vg[p], vb[p]]), gamma)
            assert not chi[p].any() and not jac[p].any(), (tag, p)
            assert np.all(np.abs(dsignal[p] - want) <= 64 * np.finfo(np.float64).eps * np.abs(want)), (tag, p)
            continue
        k = int(nv[p])
        ref = point_reference(dev, Hm, states[p, :k], tcs[p], kT[p], np.concatenate([vg[p], vb[p]]), gamma)
        tchi = np.maximum(ref["tol_chi"], 1e-300)
        worst["chi"] = max(worst["chi"], float((np.abs(chi[p] - ref["chi"]) / tchi[None, :]).max()))
        worst["jac"] = max(worst["jac"], float((np.abs(jac[p] - ref["jac"]) / ref["tol_jac"][None, :]).max()))
        worst["dsignal"] = max(worst["dsignal"], float((np.abs(dsignal[p] - ref["dsignal"]) / ref["tol_dsignal"]).max()))
        share = max(share, ref["tol_dsignal_c0_share"])
        cn = chi[p][:, :N]
        t = tchi[:N].max()
        worst["sym"] = max(worst["sym"], float(np.abs(cn - cn.T).max() / t))
        worst["nsd"] = max(worst["nsd"], float(np.linalg.eigvalsh(0.5 * (cn + cn.T)).max() / t))
        if closed:
            worst["sum"] = max(worst["sum"], float((np.abs(chi[p].sum(axis=0)) / (N * tchi)).max()))
        for d in range(N - 1):
            if tcs[p][d] == 0.0:
                assert not chi[p][:, N + d].any(), (tag, p, d)
    print(f"[response] {tag}: worst err / tol: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + f"; largest share of the c0 term in tol_dsignal {share:.6f}")
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)
    return max(worst.values())
