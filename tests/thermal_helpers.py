"""Reference and tolerance of the thermal-state tests, one source for both tiers (tests/test_thermal_cpu.py through the host build
of csrc/qd_thermal.h, tests/test_gpu_thermal.py through the device).

Reference, per point: the Hamiltonian H over the oracle's kept list cut to the nv valid states (`hamiltonians`, the construction
of `_spectrum` in tests/test_gpu_levels.py), Hs = H - min(diag H) I, w, V = numpy.linalg.eigh(Hs), P = V^2 @ softmax(-w / kT).

Tolerance, with hs = ||Hs||_inf, hn = ||H||_inf, g = w[1] - w[0], n_max the largest occupation in the list:
    tol_occ = n_max * 4 * (1e-12 hs + 1e-13 hn) * min(1 / kT, 1 / g) + 1e-12,    tol_var = n_max * tol_occ
1e-12 hs is the project's eigenvalue bar taken as the backward error of each of the two decompositions; 1e-13 hn covers the
rounding of the diagonal energies, which device and oracle compute separately (the levels test records 7.2e-15 hn, this is one
order of margin); min(1 / kT, 1 / g) bounds the divided differences of exp(-x / kT), the condition of the Gibbs state; the
factor 4 is 2 for the normalisation times 2 for the two computations.  Every point is compared: no gap exemption."""
import numpy as np

import qd_oracle as O

KB_REF = 8.617333262145e-5          # the reference's conversion as written (ground_state.py:48): kT = KB_REF * T


def hnorm(A):
    return np.abs(A).sum(axis=1).max()


def softmax(x):
    e = np.exp(x - x.max())
    return e / e.sum()


def reference(Hm, kT):
    """(P (s,), weights in the order of eigh (s,), w (s,) of the shifted matrix) of one dense symmetric block"""
    Hs = Hm - np.min(np.diag(Hm)) * np.eye(Hm.shape[0])
    w, V = np.linalg.eigh(Hs)
    with np.errstate(under="ignore"):
        wt = softmax(-w / kT)
        return (V * V) @ wt, wt, w


def spectral_factor(Hm, kT):
    """(1e-12 hs + 1e-13 hn) * min(1 / kT, 1 / g): the bound of a population before the factors 4 and n_max"""
    s = Hm.shape[0]
    Hs = Hm - np.min(np.diag(Hm)) * np.eye(s)
    cond = 1.0 / kT
    if s > 1:
        w = np.linalg.eigvalsh(Hs)
        g = w[1] - w[0]
        if g > 0:
            cond = min(cond, 1.0 / g)
    return (1e-12 * hnorm(Hs) + 1e-13 * hnorm(Hm)) * cond


def tol_occ(Hm, kT, n_max):
    return n_max * 4.0 * spectral_factor(Hm, kT) + 1e-12


def tol_ztail(Hm, kT):
    return 4.0 * spectral_factor(Hm, kT) + 1e-300


def hamiltonians(dev, vg, vb, states, nv):
    """per point p: diag(F) + oracle.tunnel_hamiltonian on the first nv[p] states of states[p] -> list of (nv, nv) arrays"""
    N = dev.n_dot
    v_ext = np.concatenate([vg, vb], axis=1)
    with np.errstate(under="ignore"):
        tc = O.tunnel_couplings(O.effective_barrier_potential(vg, vb, dev.Cbg, dev.Cbb), dev.tc_base, dev.alpha)
    out = [None] * vg.shape[0]
    for k in np.unique(nv):
        sel = np.nonzero(nv == k)[0]
        if k == 0:
            continue
        st = states[sel, :k].astype(np.int64)
        F = O.free_energy_states(v_ext[sel], dev.cdd_inv_full, dev.cgd_full, st, N)
        with np.errstate(under="ignore"):
            Hm = F[:, :, None] * np.eye(k) + O.tunnel_hamiltonian(tc[sel], st)
        for i, p in enumerate(sel):
            out[p] = Hm[i]
    return out, tc


def point_reference(Hm, st, kT):
    """one point: (occ (N,), var (N,), ztail, tol_occ, tol_var, tol_ztail, P, w) from its block and its states (nv, N)"""
    st = np.asarray(st, np.float64)
    P, wt, w = reference(Hm, kT)
    occ = P @ st
    var = P @ (st * st) - occ * occ
    n_max = max(float(st.max()), 1.0)
    to = tol_occ(Hm, kT, n_max)
    return occ, var, float(wt[-1]), to, n_max * to, tol_ztail(Hm, kT), P, w


def compare_points(tag, Hs, states, nv, kT, occ, var=None, ztail=None):
    """the module's bound at every point; prints the worst err / tol first and returns it.  kT: scalar or per point"""
    kT = np.broadcast_to(np.asarray(kT, np.float64), (len(Hs),))
    worst = {"occ": 0.0, "var": 0.0, "ztail": 0.0}
    for p, Hm in enumerate(Hs):
        if Hm is None:                                  # no valid state (a closed sector out of reach): nothing to compare
            continue
        k = int(nv[p])
        o, v, z, to, tv, tz, _, _ = point_reference(Hm, states[p, :k], kT[p])
        worst["occ"] = max(worst["occ"], float(np.abs(occ[p] - o).max() / to))
        if var is not None:
            worst["var"] = max(worst["var"], float(np.abs(var[p] - v).max() / tv))
        if ztail is not None:
            worst["ztail"] = max(worst["ztail"], float(abs(ztail[p] - z) / tz))
    print(f"[thermal] {tag}: worst err / tol: occupations {worst['occ']:.2e}, variance {worst['var']:.2e}, ztail {worst['ztail']:.2e}")
    assert worst["occ"] <= 1.0 and worst["var"] <= 1.0 and worst["ztail"] <= 1.0, (tag, worst)
    return max(worst.values())
