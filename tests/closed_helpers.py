"""Shared by the closed-regime tests (test_closed_cpu.py, test_gpu_closed.py): the CPU build of the closed front
(tests/hosttest_closed: qd_closed_centre, qd_candidates_closed, qd_closed_record of csrc/qd_closed.h) and the reference, which
nothing outside this file defines (DESIGN "closed regime"):

  m_ref        the minimiser of (n - v')^T A (n - v') over n >= 0, sum n = Q, by enumeration of the 2^N - 1 free sets with NumPy
               solves, keeping the feasible KKT point, the free dot of highest index formed as Q minus the others
  brute_list   a stable sort by energy over the box floor(m) + {-1,0,1,2}^N cut to the sector, candidates in index order
  reference    occupations from oracle.tunnel_hamiltonian + eigh on the kept states, signal from
               oracle.charge_sensor_open(n_open=...)

Devices are the draws of oracle.sample_episode: helpers.sample_blocks makes the same devices draw for draw
(test_device_model.py) as the parameter blocks the product reads, and helpers.dev_view hands those numbers to the oracle."""
import ctypes
import itertools
import os
import subprocess

import numpy as np

import helpers as H
import qd_oracle as O
from qadapt_hip.layout import layout

EPS = np.finfo(np.float64).eps
_LIB = None


def closed_lib():
    global _LIB
    if _LIB is None:
        hdir = os.path.join(H.ROOT, "tests", "hosttest_closed")
        subprocess.check_call(["make", "-s", "-C", hdir, "libqdsim_hosttest_closed.so"])
        _LIB = ctypes.CDLL(os.path.join(hdir, "libqdsim_hosttest_closed.so"))
    return _LIB


def _p(a, t=ctypes.c_double):
    return a.ctypes.data_as(ctypes.POINTER(t))


def host_closed(N, par, v_ext, Q, KC=32):
    """The host build at the rows of v_ext (n, 2N) with total charge Q (n,): front end, centre, record."""
    par = np.ascontiguousarray(par, np.float64); v_ext = np.ascontiguousarray(v_ext, np.float64)
    n = v_ext.shape[0]
    Q = np.ascontiguousarray(np.broadcast_to(np.asarray(Q, np.int32), (n,)))
    o = dict(vpp=np.zeros((n, N + 1)), tc=np.zeros((n, N - 1)), vd=np.zeros((n, N)), isa=np.zeros(n), m=np.zeros((n, N)),
             lam=np.zeros(n), rounds=np.zeros(n, np.int32), fl=np.zeros((n, N), np.int32), nvalid=np.zeros(n, np.int32),
             idx=np.zeros((n, KC), np.uint16), E=np.zeros((n, KC)), states=np.zeros((n, KC, N), np.int32),
             stats=np.zeros(4, np.uint64))
    i32, u16, u64 = ctypes.c_int32, ctypes.c_uint16, ctypes.c_uint64
    rc = closed_lib().qdhc_closed(N, KC, _p(par), ctypes.c_long(n), _p(v_ext), _p(Q, i32), _p(o["vpp"]), _p(o["tc"]), _p(o["vd"]),
                                  _p(o["isa"]), _p(o["m"]), _p(o["lam"]), _p(o["rounds"], i32), _p(o["fl"], i32),
                                  _p(o["nvalid"], i32), _p(o["idx"], u16), _p(o["E"]), _p(o["states"], i32), _p(o["stats"], u64))
    assert rc == 0, rc
    return o


def host_open_at(N, par, vd, centre, isa, KC=32):
    """The open host search (qd_candidates, reference order) with ncont := centre: idx, E (* isa), nvalid, fl"""
    par = np.ascontiguousarray(par, np.float64); vd = np.ascontiguousarray(vd, np.float64)
    centre = np.ascontiguousarray(centre, np.float64); isa = np.ascontiguousarray(isa, np.float64)
    n = vd.shape[0]
    o = dict(idx=np.zeros((n, KC), np.uint16), E=np.zeros((n, KC)), nvalid=np.zeros(n, np.int32), fl=np.zeros((n, N), np.int32))
    rc = closed_lib().qdhc_open_at(N, KC, _p(par), ctypes.c_long(n), _p(vd), _p(centre), _p(isa), _p(o["idx"], ctypes.c_uint16),
                                   _p(o["E"]), _p(o["nvalid"], ctypes.c_int32), _p(o["fl"], ctypes.c_int32))
    assert rc == 0, rc
    return o


def states_of(fl, idx):
    """(..., K, N) states of the indices idx (..., K) around the floors fl (..., N)"""
    N = fl.shape[-1]
    dig = np.stack([(idx.astype(np.int64) >> (2 * (N - 1 - i))) & 3 for i in range(N)], axis=-1) - 1
    return fl[..., None, :] + dig


# ------------------------------------------------------------------ the reference
def m_ref(A, v, Q):
    """(m, free): the constrained minimiser by enumeration.  On a free set F (n = 0 elsewhere) the KKT system is
    [[2 A_FF, 1], [1^T, 0]] [n_F; lambda] = [2 (A v)_F; Q]; the point kept is the one that is feasible (n_F >= 0, and
    g~ = 2 A (n - v) + lambda >= 0 on the clamped dots), in floating point the one whose worst violation is smallest."""
    N = len(v)
    if Q == 0:
        return np.zeros(N), ()
    b = A @ v
    best = None
    for r in range(1, N + 1):
        for F in itertools.combinations(range(N), r):
            F = list(F); k = len(F)
            M = np.zeros((k + 1, k + 1)); M[:k, :k] = 2 * A[np.ix_(F, F)]; M[:k, k] = 1; M[k, :k] = 1
            sol = np.linalg.solve(M, np.concatenate([2 * b[F], [Q]]))
            n = np.zeros(N); n[F] = sol[:k]
            n[F[-1]] = Q - n[F[:-1]].sum()                          # the lone-dot rule
            gt = 2 * (A @ n - b) + sol[k]
            C = [i for i in range(N) if i not in F]
            score = min(n[F].min(), gt[C].min() if C else np.inf)
            if best is None or score > best[0]:
                best = (score, n, tuple(F))
    return np.maximum(best[1], 0.0), best[2]


def brute_list(A, vd, fl, Q, K):
    """(states (nv, N), E (nv,), idx (nv,)) with nv <= K: every c = fl + delta, delta in {-1,0,1,2}^N in index order (dot 0 the
    most significant base-4 digit), c >= 0, sum c = Q, stably sorted by the NumPy energy; and the full sorted energies"""
    N = len(fl)
    idx = np.arange(4 ** N)
    delta = np.stack([(idx >> (2 * (N - 1 - i))) & 3 for i in range(N)], axis=1) - 1
    c = fl[None, :] + delta
    ok = (c >= 0).all(axis=1) & (c.sum(axis=1) == Q)
    c, idx = c[ok], idx[ok]
    d = c - vd[None, :]
    E = np.einsum("ki,ij,kj->k", d, A, d)
    order = np.argsort(E, kind="stable")
    return c[order][:K], E[order][:K], idx[order][:K], E[order]


def occupations_ref(dev, vg, vb, states, nvalid, K):
    """Per point: the ground state of diag(F) + tunnel Hamiltonian over the first min(nvalid, K) states (oracle code, eigh):
    (occ (n, N), rel_gap (n,)) with rel_gap = (lam1 - lam0) / ||H||_inf, inf for a single state"""
    vg = np.asarray(vg, float); vb = np.asarray(vb, float)
    n, N = vg.shape[0], dev.n_dot
    v_ext = np.concatenate([vg, vb], axis=1)
    tc = O.tunnel_couplings(O.effective_barrier_potential(vg, vb, dev.Cbg, dev.Cbb), dev.tc_base, dev.alpha)
    occ = np.zeros((n, N)); gap = np.full(n, np.inf)
    nv = np.minimum(nvalid, K)
    for k in np.unique(nv):
        sel = np.nonzero(nv == k)[0]
        st = states[sel, :k].astype(np.int64)
        F = O.free_energy_states(v_ext[sel], dev.cdd_inv_full, dev.cgd_full, st, N)
        Hm = F[:, :, None] * np.eye(k) + O.tunnel_hamiltonian(tc[sel], st)
        w, vec = np.linalg.eigh(Hm)
        occ[sel] = np.einsum("pm,pmd->pd", np.abs(vec[:, :, 0]) ** 2, st.astype(np.float64))
        if k > 1:
            gap[sel] = (w[:, 1] - w[:, 0]) / np.abs(Hm).sum(axis=2).max(axis=1)
    return occ, gap


def signal_ref(dev, vg, vb, occ, gamma=None):
    return O.charge_sensor_open(dev, vg, vb, n_open=occ, gamma=gamma)[0][:, 0]


# ------------------------------------------------------------------ inputs
def points(N, rng, n):
    """vg (n, N+1) from U(-0.5, 4) for two thirds of the points and U(-3, 3) for the rest, vb (n, N-1) from U(-2, 2)"""
    a = (2 * n + 2) // 3
    vg = np.concatenate([rng.uniform(-0.5, 4.0, (a, N + 1)), rng.uniform(-3.0, 3.0, (n - a, N + 1))])
    return vg, rng.uniform(-2.0, 2.0, (n, N - 1))


def q_values(N, qs):
    """the six total charges around Qs (clipped at 0)"""
    return [0, 1, max(int(qs) - 1, 0), int(qs), int(qs) + 1, 2 * N + 1]


def open_totals(dev, vg, vb):
    """rounded total of the open oracle's occupations, per point, and those occupations"""
    n = O.ground_state_open(dev, vg, vb)
    return np.rint(n.sum(axis=1)).astype(np.int64), n


def delta_bound(A, vd, Q):
    """64 kappa_2(A) eps max(1, |v'|_inf, Q)"""
    return 64 * np.linalg.cond(A) * EPS * max(1.0, float(np.abs(vd).max()), float(Q))


def sub_A(N, par):
    L = layout(N); G = N + 1
    return par[L.cdd_inv:L.cdd_inv + G * G].reshape(G, G)[:N, :N].copy()
