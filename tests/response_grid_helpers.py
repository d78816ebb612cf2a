"""The axis chain of the charge-response grids, one source for both tiers (tests/test_response_blocks_cpu.py,
tests/test_gpu_response_grid.py): the physical direction u = dv/ds of an axis scalar, the two outputs a grid is plotted with as
contractions of response_helpers' reference, their tolerances, and an independent check of the chain, a central difference of the
reference thermal occupations with the kept list held fixed.

    u = dir in the physical frame;  u[:G] = vgm @ dir[:G], u[G:] = dir[G:] in the virtual one (vgm: the query's if given, else the env's)
    docc_axes[i][a] = sum_j jac[i][j] u_a[j],   dsignal_axes[a] = sum_j dsignal[j] u_a[j]
    tol_docc[a] = tol_jac . |u_a| + 64 eps sum_j |jac[i][j] u_a[j]|,   tol_dsignal_axes[a] likewise from tol_dsignal
"""
import numpy as np

import helpers as H
import qd_oracle as O
import response_helpers as RH
import thermal_helpers as TH

EPS = np.finfo(np.float64).eps


def open_lists(dev, v_ext, K):
    """the oracle's kept list of K states and the number of valid ones, per point"""
    N = dev.n_dot
    states, n_cont = O.candidate_states(v_ext, dev.cdd_inv_full, dev.cgd_full, N, k=K)
    cfg = O._delta_table(N)[None] + np.floor(n_cont)[:, None, :]
    return states, np.minimum(np.all(cfg >= 0, axis=-1).sum(axis=1), K)


def slot_vgm(N, st, vgm=None):
    L, G = H.layout(N), N + 1
    return np.asarray(st[L.s_vgm:L.s_vgm + G * G] if vgm is None else vgm, np.float64).reshape(G, G)


def axis_directions(N, st, frame, dx, dy, vgm=None):
    """u (2, 2N): the physical directions of one step of sx and of sy"""
    G = N + 1
    u = np.stack([np.asarray(dx, np.float64), np.asarray(dy, np.float64)]).copy()
    if frame == "virtual":
        u[:, :G] = u[:, :G] @ slot_vgm(N, st, vgm).T
    return u


def physical(N, par, st, frame, W, vgm=None):
    """v_ext (.., 2N) of the control values W (.., 2N) through the frame"""
    L, G = H.layout(N), N + 1
    W = np.asarray(W, np.float64)
    if frame == "physical":
        return W.copy()
    v = W.copy()
    v[..., :G] = W[..., :G] @ slot_vgm(N, st, vgm).T + par[L.origin:L.origin + G]
    return v


def axes_reference(ref, u):
    """(docc_axes (N, 2), tol (N, 2), dsignal_axes (2,), tol (2,)) from a point_reference dict and u (2, 2N)"""
    jac, ds = ref["jac"], ref["dsignal"]
    docc = jac @ u.T
    tdocc = (ref["tol_jac"] @ np.abs(u).T)[None, :] + 64 * EPS * (np.abs(jac) @ np.abs(u).T)
    dsa = ds @ u.T
    tdsa = ref["tol_dsignal"] @ np.abs(u).T + 64 * EPS * (np.abs(ds) @ np.abs(u).T)
    return docc, np.maximum(tdocc, 5e-324), dsa, np.maximum(tdsa, 5e-324)


def thermal_occupations(dev, v_ext, states, kT):
    """<n> (N,) of the reference thermal state at one point on a FIXED list of valid states (nv, N)"""
    st = np.asarray(states, np.int64)
    Hs, _ = TH.hamiltonians(dev, v_ext[None, :dev.n_dot + 1], v_ext[None, dev.n_dot + 1:], st[None], np.array([len(st)]))
    P, _, _ = TH.reference(Hs[0], kT)
    return P @ st.astype(np.float64)


def central_difference(N, par, st, dev, frame, W0, d, states, kT, h, vgm=None):
    """d<n>/ds (N,) along the control direction d (2N,) at the control point W0 by a central difference of step h in the scalar,
    the Hamiltonian rebuilt at W0 +- h d through the frame, the kept list fixed"""
    d = np.asarray(d, np.float64)
    up = thermal_occupations(dev, physical(N, par, st, frame, W0 + h * d, vgm), states, kT)
    dn = thermal_occupations(dev, physical(N, par, st, frame, W0 - h * d, vgm), states, kT)
    return (up - dn) / (2.0 * h)


def compare_axes(tag, refs, u, docc, dsa):
    """the bounds of axes_reference at every point with a reference (refs[p] None: zeros exactly in docc); prints and returns the
    worst err / tol"""
    worst = {"docc_axes": 0.0, "dsignal_axes": 0.0}
    for p, ref in enumerate(refs):
        if ref is None:
            assert not docc[p].any(), (tag, p)
            continue
        rd, td, rs, ts = axes_reference(ref, u)
        worst["docc_axes"] = max(worst["docc_axes"], float((np.abs(docc[p] - rd) / td).max()))
        worst["dsignal_axes"] = max(worst["dsignal_axes"], float((np.abs(dsa[p] - rs) / ts).max()))
    print(f"[response grid] {tag}: worst err / tol: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), (tag, worst)
    return max(worst.values())
