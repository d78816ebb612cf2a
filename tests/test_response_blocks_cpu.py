"""The charge response per hop component without a GPU: the epilogue of csrc/qd_response_blocks.h (D, G = V^T X V and dP inside the
components, the global Z and <X>, the chain rule, the sensor slope, the axis direction) compiled for the CPU with the 64 lanes as a
loop (tests/hosttest_response_blocks), behind the unchanged per-component thermal core, against the float64 reference of
tests/response_helpers.py as it is (chi_reference, tol_chi, block_check: pinned against mpmath in tests/test_response_cpu.py);
block-diagonal compositions with scattered members; the whole-block epilogue on one component of 32; the record path with the
chain rule on the oracle's open lists; the axis chain of the grids against a central difference of the reference occupations;
the header / ctypes agreement and the argument checks of qd_scan_grid_response on a handle that never reached a device; the Python
layer on a stub; the sanitizer program.

Measured worst err / tol (also in DESIGN 7, "Charge-response grids"): the families of every size 1..32 2.8e-3, the partitions
1.5e-3, one component of 32 against the whole-block epilogue 0 (of 2 tol_chi: with one component the two schedules run the same operations), the record path 3.7e-4.  The axis
chain: reference docc_axes against the central difference (h = 1e-5 in the axis scalar), worst |difference| / scale 3.8e-6 at
4 dots and 3.8e-7 at 2 (the scale: AXIS_BOUND below); a transposed matrix or a dropped barrier gives 0.3 and more."""
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
import response_grid_helpers as RG
import response_helpers as RH
import thermal_helpers as TH
import test_response_cpu as TRC
import test_thermal_blocks_cpu as TBC
from test_levels_cpu import _built_lib, _handle, _record_fields, n_valid

HDIR = os.path.join(H.ROOT, "tests", "hosttest_response_blocks")
WS_BYTES = 25008                                      # the figure of the header comment of csrc/qd_response_blocks.h
DP = ctypes.POINTER(ctypes.c_double)
_LIB = None

# The axis chain: reference against reference.  Central difference of the reference occupations with h = AXIS_H in the axis
# scalar against jac . u, relative to the scale |d<n>/ds| + h^2 |u|^3 / kT^3 / 6 n_max (the third derivative of a thermal
# occupation is at most of order n_max |dE/ds|^3 / kT^3, |dE/ds| <= |Lam u|_inf; the truncation of the central difference) plus the
# rounding 4 tol_occ / h of the two occupations.  AXIS_WORST is what that comparison measures on the CPU over the cases below,
# AXIS_BOUND ten times it.
AXIS_H = 1e-5
AXIS_WORST = 3.8e-6                                  # N = 4; 3.8e-7 at N = 2
AXIS_BOUND = 10 * AXIS_WORST


def blocks_lib():
    global _LIB
    if _LIB is None:
        subprocess.check_call(["make", "-s", "-C", HDIR, "libqdsim_hosttest_response_blocks.so"])
        _LIB = ctypes.CDLL(os.path.join(HDIR, "libqdsim_hosttest_response_blocks.so"))
        _LIB.qdhrb_response.argtypes = [ctypes.c_int, DP, ctypes.c_double, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), DP,
                                        ctypes.POINTER(ctypes.c_uint8), ctypes.c_int, DP, DP]
        _LIB.qdhrb_record.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_int32), DP, DP,
                                      ctypes.c_int, ctypes.c_int, ctypes.c_double, DP, ctypes.c_int, DP, DP, DP, DP, DP]
        _LIB.qdhrb_sensor_slope.argtypes = [ctypes.c_double] * 3
        _LIB.qdhrb_sensor_slope.restype = ctypes.c_double
        _LIB.qdhrb_axis_direction.argtypes = [ctypes.c_int, DP, ctypes.c_int, DP, DP]
    return _LIB


def host_block(A, kT, nt, Ts, poison=1):
    """dP (npert, s) and pop (s,) of the host-compiled per-component epilogue"""
    s = A.shape[0]
    kind, x, nb = TRC.pack_perts(nt, Ts)
    dP, pop = np.full((len(kind), 32), np.nan), np.full(32, np.nan)
    rc = blocks_lib().qdhrb_response(s, H._p(EC.packed(A), ctypes.c_double), kT, len(kind), H._p(kind, ctypes.c_int32),
                                     H._p(x, ctypes.c_double), H._p(nb, ctypes.c_uint8), poison, H._p(dP, ctypes.c_double),
                                     H._p(pop, ctypes.c_double))
    assert rc >= 0, (s, kT, rc)
    assert not dP[:, s:].any()
    return dP[:, :s], pop[:s]


def respect(Ts, A):
    """the sparse patterns cut to the links of A: an entry of a perturbation only where the block has one"""
    return [np.where(A != 0.0, T, 0.0) for T in Ts]


def partition_probe(A, seed):
    """occupation columns and two sparse patterns that respect the components of A: a chain over the members of every component
    in increasing order, and every third member with the next but one"""
    s = A.shape[0]
    rng = np.random.default_rng(7100 + seed)
    nt = rng.integers(0, 4, (s, 3)).astype(np.float64)
    lab = TBC.bfs_labels(A)
    T1, T2 = np.zeros((s, s)), np.zeros((s, s))
    for c in np.unique(lab):
        mem = np.flatnonzero(lab == c)
        for i in range(len(mem) - 1):
            T1[mem[i], mem[i + 1]] = T1[mem[i + 1], mem[i]] = -rng.uniform(0.3, 2.0)
        for i in range(0, len(mem) - 2, 3):
            T2[mem[i], mem[i + 2]] = T2[mem[i + 2], mem[i]] = -rng.uniform(0.5, 1.5)
    return nt, [T1, T2]


# ------------------------------------------------------------------ the families through the host build
@pytest.mark.parametrize("s", range(1, 33))
def test_families_of_every_size(s):
    """every block of response_helpers.family(s), probed with three occupation columns and two sparse patterns cut to the block's
    own links (a perturbation has an entry only where the Hamiltonian has one), from a NaN-filled workspace"""
    nt, Ts0 = RH.probe(s, 0)
    worst = {}
    for tag, A, kT in RH.family(s):
        Ts = respect(Ts0, A)
        dP, _ = host_block(A, kT, nt, Ts)
        assert np.isfinite(dP).all(), (tag, kT)
        if s == 1:
            assert not dP.any()                                          # one state: zero exactly
        r = RH.block_check(A, kT, nt, Ts, dP)
        assert r <= 1.0, (s, tag, kT, r)
        worst[RH.kind(tag)] = max(worst.get(RH.kind(tag), 0.0), r)
    print(f"[response blocks cpu] s={s}: worst err / tol per family: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_results_do_not_depend_on_what_the_workspace_held():
    for s in (2, 7, 31, 32):
        nt, Ts0 = RH.probe(s, 1)
        for tag, A, kT in RH.family(s)[::7]:
            Ts = respect(Ts0, A)
            a, _ = host_block(A, kT, nt, Ts, poison=0)
            b, _ = host_block(A, kT, nt, Ts, poison=1)
            assert np.array_equal(a, b), (s, tag)


# ------------------------------------------------------------------ compositions
@pytest.mark.parametrize("name", list(TBC.PARTITIONS))
def test_block_diagonal_compositions_with_scattered_members(name):
    """the partitions of test_thermal_blocks_cpu.py, dealt round-robin and under a random permutation, over three coupling scales
    and the temperatures of response_helpers; 32x1: chi_n = -cov / kT and the hop columns exactly 0.0"""
    sizes = TBC.PARTITIONS[name]
    rng = np.random.default_rng(sum(ord(c) for c in name) + 1)
    worst = 0.0
    for tscale in (1e-3, 1.0, 30.0):
        for k, perm in enumerate((TBC.interleave(sizes), rng.permutation(32))):
            A = TBC.composition(rng, sizes, tscale, perm)
            nt, Ts = partition_probe(A, k)
            for kT in RH.temperatures(A):
                dP, pop = host_block(A, kT, nt, Ts)
                assert np.isfinite(dP).all()
                r = RH.block_check(A, kT, nt, Ts, dP)
                assert r <= 1.0, (name, tscale, kT, r)
                worst = max(worst, r)
                if name == "32x1":
                    assert not Ts[0].any() and not dP[3:].any()            # nothing couples: the hop columns are zero exactly
                    chi = nt.T @ dP[:3].T
                    mean = pop @ nt
                    cov = (nt - mean).T @ ((nt - mean) * pop[:, None])
                    tol = RH.tol_chi(A, kT, nt.max(), [nt.max()] * 3)
                    assert np.all(np.abs(chi + cov / kT) <= tol.max()), (kT, float(np.abs(chi + cov / kT).max()))
    print(f"[response blocks cpu] partition {name}: worst err / tol {worst:.2e}")


def test_one_component_of_32_agrees_with_the_whole_block_epilogue():
    worst, met = 0.0, 0
    nt, Ts0 = RH.probe(32, 3)
    for tag, A, kT in RH.family(32)[::5]:
        if len(np.unique(TBC.bfs_labels(A))) != 1:
            continue
        met += 1
        Ts = respect(Ts0, A)
        a, _ = host_block(A, kT, nt, Ts)
        b, _ = TRC.host_block(A, kT, nt, Ts)
        n_max = max(float(nt.max()), 1.0)
        tol = RH.tol_chi(A, kT, n_max, [n_max] * 3 + [max(TH.hnorm(T), 1e-300) for T in Ts])
        r = float((np.abs(nt.T @ a.T - nt.T @ b.T) / (2.0 * tol[None, :])).max())
        assert r <= 1.0, (tag, kT, r)
        worst = max(worst, r)
    assert met >= 10
    print(f"[response blocks cpu] one component of 32 against the whole-block epilogue, {met} blocks: worst difference / (2 tol_chi) "
          f"{worst:.2e}")


def test_a_denormal_link_links_and_an_exact_zero_does_not():
    """two blocks of 4 joined by one entry: a denormal joins them into one component (the response moves by less than the
    tolerance), an exact zero leaves two; both within the bound, and the zero case equals the denormal one within 2 tol"""
    rng = np.random.default_rng(77)
    base = TBC.composition(rng, [4, 4], 0.3, np.arange(8))
    nt, Ts = partition_probe(base, 5)                           # (the same probes for both: those of the cut block)
    kT = 0.05
    outs, tols = [], []
    for link in (5e-324, 0.0):
        A = base.copy()
        A[3, 4] = A[4, 3] = -link
        assert len(np.unique(TBC.bfs_labels(A))) == (1 if link else 2)
        dP, _ = host_block(A, kT, nt, Ts)
        assert RH.block_check(A, kT, nt, Ts, dP) <= 1.0
        outs.append(nt.T @ dP.T)
        tols.append(RH.tol_chi(A, kT, nt.max(), [nt.max()] * 3 + [TH.hnorm(T) for T in Ts]))
    assert np.all(np.abs(outs[0] - outs[1]) <= (tols[0] + tols[1])[None, :])


def test_workspace_fits_the_stated_budget():
    """QdThermalBlocksWs is as it was; sizeof(QdResponseBlocksWs) is the figure of the header comment and six blocks fit the 160 KB
    of a CU, with the 256 B of the grid kernel's axis directions"""
    L = blocks_lib()
    hdr = open(os.path.join(H.ROOT, "rl-agent-for-qubit-array-tuning_amd", "csrc", "qd_response_blocks.h")).read()
    stated = int(re.search(r"sizeof\(QdResponseBlocksWs\) = ([\d ]+) B", hdr).group(1).replace(" ", ""))
    assert stated == WS_BYTES == L.qdhrb_ws_bytes() and L.qdhrb_thermal_blocks_ws_bytes() == 24680
    assert 6 * (stated + 256) <= 160 * 1024 < 7 * stated


# ------------------------------------------------------------------ the record path and the chain rule
def _host_record(N, idx, fl, tc, E, nv, K, kT, par, poison=1):
    chi, jac, dc0 = np.full((N, 2 * N - 1), np.nan), np.full((N, 2 * N), np.nan), np.full(2 * N, np.nan)
    occ, var = np.zeros(N), np.zeros(N)
    got = blocks_lib().qdhrb_record(N, H._p(idx, ctypes.c_uint16), H._p(np.ascontiguousarray(fl), ctypes.c_int32),
                                    H._p(np.ascontiguousarray(tc), ctypes.c_double), H._p(E, ctypes.c_double), nv, K, kT,
                                    H._p(np.ascontiguousarray(par), ctypes.c_double), poison, H._p(chi, ctypes.c_double),
                                    H._p(jac, ctypes.c_double), H._p(dc0, ctypes.c_double), H._p(occ, ctypes.c_double),
                                    H._p(var, ctypes.c_double))
    assert got == nv
    return chi, jac, dc0, occ, var


@pytest.mark.parametrize("N,K", [(2, 32), (3, 32), (4, 8), (4, 32), (8, 32), (8, 8)])
def test_record_path_against_the_oracles_hamiltonian(N, K):
    """the record path of qd_k_thermal_grid_response on the oracle's open lists at the kT of 100 K and of 1 K, through
    response_helpers.point_reference: chi, the jacobian and dc0/dv; with every coupling zero chi[:, :N] = -cov / kT, its diagonal
    -var / kT and the ln tc columns exactly 0.0; with one coupling zero among the others that column exactly 0.0"""
    rng = np.random.default_rng(300 * N + K)
    eb = H.sample_blocks(N, [61, 62])
    lay = H.layout(N)
    worst = 0.0
    for e in range(2):
        par = eb.params[e]
        dev = H.dev_view(N, par)
        n = 12
        vg = par[lay.vopt:lay.vopt + N + 1] + rng.uniform(-4, 4, (n, N + 1))
        if N <= 3:
            vg[: n // 2] -= 8.0
        vb = par[lay.vbopt:lay.vbopt + N - 1] + rng.uniform(-3, 3, (n, N - 1))
        v_ext = np.concatenate([vg, vb], axis=1)
        states, _ = O.candidate_states(v_ext, dev.cdd_inv_full, dev.cgd_full, N, k=K)
        F = O.free_energy_states(v_ext, dev.cdd_inv_full, dev.cgd_full, states, N)
        tc = O.tunnel_couplings(O.effective_barrier_potential(vg, vb, dev.Cbg, dev.Cbb), dev.tc_base, dev.alpha)
        nvs, floors = n_valid(v_ext, dev, N, K)
        for p in range(n):
            nv = int(nvs[p])
            idx, E = _record_fields(N, states[p], floors[p], F[p], nv)
            st = states[p, :nv].astype(np.int64)
            for cut in ("none", "one", "all"):
                t = np.ascontiguousarray(tc[p]).copy()
                if cut == "all":
                    t[:] = 0.0
                elif cut == "one":
                    t[p % (N - 1)] = 0.0
                Hm = np.diag(F[p, :nv]) + O.tunnel_hamiltonian(t[None], st[None])[0]
                for kT in (TH.KB_REF * 100, TH.KB_REF * 1):
                    chi, jac, dc0, occ, var = _host_record(N, idx, floors[p], t, E, nv, K, kT, par)
                    ref = RH.point_reference(dev, Hm, st, t, kT, v_ext[p], dev.gamma)
                    tchi = np.maximum(ref["tol_chi"], 1e-300)
                    r = max(float((np.abs(chi - ref["chi"]) / tchi[None, :]).max()),
                            float((np.abs(jac - ref["jac"]) / ref["tol_jac"][None, :]).max()))
                    tdc0 = 2.0 * np.abs(dev.cdd_inv_full[N, :N]).sum() * ref["tol_jac"] + 1e-15 * np.abs(ref["dc0"])
                    r = max(r, float((np.abs(dc0 - ref["dc0"]) / tdc0).max()))
                    assert r <= 1.0, (N, K, e, p, cut, kT, r)
                    worst = max(worst, r)
                    for d in range(N - 1):
                        if t[d] == 0.0:
                            assert not chi[:, N + d].any(), (cut, d)
                    if nv == 1:
                        assert not chi.any() and not jac.any()
                    if cut == "all":
                        P, _, _ = TH.reference(Hm, kT)
                        nf = st.astype(np.float64)
                        mean = P @ nf
                        cov = (nf - mean).T @ ((nf - mean) * P[:, None])
                        assert np.all(np.abs(chi[:, :N] + cov / kT) <= tchi[:N].max())
                        assert np.all(np.abs(np.diag(chi[:, :N]) + var / kT) <= tchi[:N].max())
    print(f"[response blocks cpu] record path N={N} K={K}: worst err / tol {worst:.2e}")


def test_a_record_without_a_valid_state_gives_zeros():
    N = 4
    par = H.sample_blocks(N, [61]).params[0]
    chi, jac, dc0, occ, var = _host_record(N, np.zeros(32, np.uint16), np.zeros(N, np.int32), np.zeros(N - 1), np.zeros(32), 0, 8,
                                           0.01, par)
    dev = H.dev_view(N, par)
    assert not chi.any() and not jac.any() and not occ.any()
    want = -2.0 * dev.cdd_inv_full[N, :N] @ dev.cgd_full[:N] - 2.0 * dev.cdd_inv_full[N, N] * dev.cgd_full[N]
    assert np.allclose(dc0, want, rtol=1e-14, atol=0)


def test_sensor_slope_is_the_derivative_of_the_sensor_expression():
    L = blocks_lib()
    rng = np.random.default_rng(5)
    for _ in range(200):
        c0, a, g = rng.uniform(-3, 3), rng.uniform(0.05, 0.5), rng.uniform(0.05, 1.0)
        rr = (c0 + 2.0 * a * np.arange(-5, 5)) / g
        want = float((-2.0 * rr / (g * (rr * rr + 1.0) ** 2)).sum())
        got = L.qdhrb_sensor_slope(c0, a, g)
        assert abs(got - want) <= 64 * np.finfo(float).eps * float(np.abs(2.0 * rr / (g * (rr * rr + 1.0) ** 2)).sum())


# ------------------------------------------------------------------ the axis chain, independently of the kernels
def _axis_cases(N):
    """(par, st, dev, frame, vgm or None, W0, dx, dy) over the oracle's device: both frames, the env's matrix and a query's own"""
    rng = np.random.default_rng(4400 + N)
    eb = H.sample_blocks(N, [71])
    par = eb.params[0]
    st = H.place(N, eb.state[0], "near", rng)
    L, G = H.layout(N), N + 1
    dev = H.dev_view(N, par)
    own = np.eye(G) + rng.normal(0, 0.15, (G, G))               # a query's matrix, far from the env's and not symmetric
    out = []
    for frame, vgm in (("physical", None), ("virtual", None), ("virtual", own)):
        for _ in range(3):
            gv, sv, bv = st[L.s_gate_v:L.s_gate_v + N], st[L.s_sensor_gt], st[L.s_barrier_v:L.s_barrier_v + N - 1]
            W0 = np.concatenate([gv, [sv], bv]) + np.concatenate([rng.uniform(-1, 1, N), [0.0], rng.uniform(-0.3, 0.3, N - 1)])
            if frame == "physical":
                W0 = RG.physical(N, par, st, "virtual", W0)
            dx, dy = rng.normal(size=2 * N), rng.normal(size=2 * N)
            dx[N] *= 0.1; dy[N] *= 0.1
            out.append((par, st, dev, frame, vgm, W0, dx, dy))
    return out


def _axis_ratio(N, case, kT, helper=RG.axis_directions):
    par, st, dev, frame, vgm, W0, dx, dy = case
    v = RG.physical(N, par, st, frame, W0, vgm)
    states, nv = RG.open_lists(dev, v[None], 8)
    kept = states[0, :int(nv[0])]
    Hs, tcs = TH.hamiltonians(dev, v[None, :N + 1], v[None, N + 1:], states, nv)
    ref = RH.point_reference(dev, Hs[0], kept, tcs[0], kT, v, dev.gamma)
    u = helper(N, st, frame, dx, dy, vgm)
    docc = ref["jac"] @ u.T
    worst = 0.0
    n_max = max(float(kept.max()), 1.0)
    Lam, Gam = RH.chain_matrices(dev)
    for a, d in enumerate((dx, dy)):
        fd = RG.central_difference(N, par, st, dev, frame, W0, d, kept, kT, AXIS_H, vgm)
        ua = RG.axis_directions(N, st, frame, dx, dy, vgm)[a]
        slope = float(np.abs(Lam @ ua).max() + np.abs(Gam @ ua).max() * max(TH.hnorm(Hs[0] - np.diag(np.diag(Hs[0]))), 0.0))
        scale = np.abs(docc[:, a]) + n_max * (AXIS_H ** 2) * slope ** 3 / kT ** 3 / 6.0 \
            + 4.0 * TH.tol_occ(Hs[0], kT, n_max) / AXIS_H + 1e-9 * n_max * slope / kT
        worst = max(worst, float((np.abs(fd - docc[:, a]) / scale).max()))
    return worst


@pytest.mark.parametrize("N", [2, 4])
def test_axis_chain_against_a_central_difference_of_the_reference_occupations(N):
    """reference docc_axes = jac . u in both frames, with the env's matrix and with a query's own, against a central difference
    of the reference thermal occupations, the kept list fixed and the Hamiltonian rebuilt at W0 +- h e_axis through the frame"""
    worst = 0.0
    for case in _axis_cases(N):
        for kT in (TH.KB_REF * 100, TH.KB_REF * 10):
            worst = max(worst, _axis_ratio(N, case, kT))
    print(f"[response blocks cpu] axis chain N={N}: worst |central difference - jac . u| / scale {worst:.2e} (bound {AXIS_BOUND})")
    assert worst <= AXIS_BOUND


def test_axis_check_catches_a_transposed_matrix_and_a_missing_barrier():
    """the comparison above is not blind: a helper with vgm transposed, and one that drops the barrier components, miss the bound"""
    N = 4

    def transposed(N, st, frame, dx, dy, vgm=None):
        u = np.stack([dx, dy]).astype(np.float64)
        if frame == "virtual":
            u[:, :N + 1] = u[:, :N + 1] @ RG.slot_vgm(N, st, vgm)
        return u

    def no_barriers(N, st, frame, dx, dy, vgm=None):
        u = RG.axis_directions(N, st, frame, dx, dy, vgm)
        u[:, N + 1:] = 0.0
        return u

    cases = _axis_cases(N)
    kT = TH.KB_REF * 100
    for broken, pick in ((transposed, [c for c in cases if c[4] is not None]), (no_barriers, cases)):
        assert max(_axis_ratio(N, c, kT, broken) for c in pick) > AXIS_BOUND, broken.__name__


def test_axis_direction_of_the_host_build():
    """qd_grid_axis_direction against the helper: the direction itself in the physical frame, vgm @ dir[:G] in the virtual one"""
    for N in (2, 4, 8):
        par, st, dev, _, _, W0, dx, dy = _axis_cases(N)[0]
        for frame, code in (("physical", 1), ("virtual", 0)):
            from grid_helpers import PHYSICAL, VIRTUAL
            u = np.zeros(2 * N)
            d = np.ascontiguousarray(dx)
            assert blocks_lib().qdhrb_axis_direction(N, H._p(np.ascontiguousarray(st), ctypes.c_double),
                                                     PHYSICAL if frame == "physical" else VIRTUAL, H._p(d, ctypes.c_double),
                                                     H._p(u, ctypes.c_double)) == 0
            want = RG.axis_directions(N, st, frame, dx, dy)[0]
            assert np.all(np.abs(u - want) <= 8 * np.finfo(float).eps * (np.abs(RG.slot_vgm(N, st)) @ np.abs(dx[:N + 1])).max())
            if frame == "physical":
                assert np.array_equal(u, dx)


# ------------------------------------------------------------------ the C entry point without a device
def test_prototype_and_struct_match_the_header():
    _lib, L = _built_lib()
    hdr = open(os.path.join(H.ROOT, "include", "qdsim.h")).read()
    assert "qd_scan_grid_response" in _lib.EXPORTS and hasattr(L, "qd_scan_grid_response")
    m = re.search(r"\bint qd_scan_grid_response\((.*?)\);", hdr, re.S)
    decl = [" ".join(a.split()) for a in m.group(1).split(",")]
    fn = L.qd_scan_grid_response
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(decl) == 17
    assert decl[10].startswith("const double* kT_dev")
    assert fn.argtypes[14]._type_ is _lib.QdScanGridOpts and decl[14].startswith("const qd_scan_grid_opts*")
    assert fn.argtypes[15]._type_ is _lib.QdGridResponseOpts and decl[15].startswith("const qd_grid_response_opts*")
    body = re.search(r"typedef struct qd_grid_response_opts \{(.*?)\} qd_grid_response_opts;", hdr, re.S).group(1)
    names = [ln.split(";")[0].split()[-1].lstrip("*") for ln in body.strip().splitlines()]
    assert names == [f[0] for f in _lib.QdGridResponseOpts._fields_] == [
        "struct_size", "reserved", "n_charge_dev", "var_dst", "ztail_dst", "chi_dst", "jac_dst", "dsignal_dst", "docc_axes_dst",
        "dsignal_axes_dst"]
    assert ctypes.sizeof(_lib.QdGridResponseOpts) == 72 and ctypes.sizeof(_lib.QdGridThermalOpts) == 32


def test_argument_checks_need_no_device():
    _lib, L = _built_lib()
    B = 3
    one = ctypes.c_void_p(64)                          # a device pointer that is never dereferenced

    def gopts(**kw):
        o = _lib.QdScanGridOpts(struct_size=ctypes.sizeof(_lib.QdScanGridOpts))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def ropts(**kw):
        o = _lib.QdGridResponseOpts(struct_size=ctypes.sizeof(_lib.QdGridResponseOpts), docc_axes_dst=64, dsignal_axes_dst=64)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def call(h, o, t, nq=1, nx=4, ny=4, kT=one, env=one):
        return L.qd_scan_grid_response(h, env, nq, nx, ny, one, one, one, one, one, kT, one, one, one,
                                       None if o is None else ctypes.byref(o), None if t is None else ctypes.byref(t), None)

    assert call(None, gopts(), ropts()) == _lib.QD_ERR_ARG
    h = _handle(L, 4, 8, B)
    try:
        def refused(rc, *words):
            msg = L.qd_last_error(h)
            assert rc == _lib.QD_ERR_ARG and msg.startswith(b"qd_scan_grid_response"), (rc, msg)
            assert all(w in msg for w in words), msg

        refused(call(h, gopts(), ropts(), kT=None), b"kT_dev")
        refused(call(h, gopts(), ropts(struct_size=32)), b"struct_size", b"qd_grid_response_opts")
        refused(call(h, gopts(struct_size=48), ropts()), b"struct_size", b"qd_scan_grid_opts")
        refused(call(h, gopts(noise_flags=_lib.QD_NOISE_LATCH), ropts()), b"QD_NOISE_LATCH")
        refused(call(h, gopts(noise_flags=_lib.QD_NOISE_LATCH | _lib.QD_NOISE_SENSOR), None), b"QD_NOISE_LATCH")
        refused(call(h, gopts(noise_flags=_lib.QD_NOISE_SENSOR), ropts(n_charge_dev=64)), b"closed regime")
        refused(call(h, gopts(), ropts(), nq=-1), b"nq")
        refused(call(h, gopts(), ropts(), nx=9, ny=8), b"nx*ny")
        refused(call(h, gopts(), ropts(), env=None), b"env_of_query_dev")
        refused(call(h, gopts(frame=7), ropts()), b"frame")
        assert call(h, gopts(), ropts(), nq=0) == 0 and call(h, None, None, nq=0) == 0
    finally:
        L.qd_destroy(h)
    hs = _handle(L, 3, 8, B, flags=_lib.QD_FLAG_VALIDATE)
    try:
        assert call(hs, gopts(), ropts()) == _lib.QD_ERR_STATE and b"QD_FLAG_VALIDATE" in L.qd_last_error(hs)
        assert L.qd_last_error(hs).startswith(b"qd_scan_grid_response")
    finally:
        L.qd_destroy(hs)


# ------------------------------------------------------------------ the Python layer
def test_python_layer_on_a_stub():
    from qadapt_hip.env import ModelFacade
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    sig = inspect.signature(VecQuantumDeviceEnv.scan_grid_response).parameters
    assert list(sig)[:12] == ["self", "env_ids", "x", "y", "x_range", "y_range", "nx", "ny", "gate_voltages", "barrier_voltages", "kT",
                              "sensor_voltage"]
    kw = ["n_charge", "frame", "vgm", "gamma", "noise", "serial", "stream_base", "occupations", "variance", "ztail", "response"]
    assert list(sig)[12:] == kw and all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in kw)
    assert sig["response"].default == ("dsignal_axes", "docc_axes")
    # scan_grid_thermal keeps its signature
    assert list(inspect.signature(VecQuantumDeviceEnv.scan_grid_thermal).parameters)[12:] == kw[:-1]
    assert list(inspect.signature(ModelFacade.do2d_response).parameters) == [
        "self", "x_gate", "x_min", "x_max", "x_points", "y_gate", "y_min", "y_max", "y_points", "T", "n_charge"]
    assert list(inspect.signature(ModelFacade.do1d_response).parameters) == ["self", "gate", "min", "max", "points", "T", "n_charge"]
    N = 4

    class Stub:
        def __init__(self, T):
            self.calls = []
            self._T_host = np.array([T])

        def scan_grid_response(self, *args, **kw):
            nx, ny = args[5], args[6]
            self.calls.append(dict(args=args, **kw))
            ds = np.zeros((1, ny, nx, 2)); ds[..., 1] = 2.0
            dn = np.zeros((1, ny, nx, N, 2)); dn[..., 0] = 1.0
            return {"raw": np.zeros((1, ny, nx)), "dsignal_axes": ds, "docc_axes": dn}

    model = ModelFacade(Stub(120.0), N)
    model.coulomb_peak_width = 0.3
    s, dsx, dsy, dnx, dny = model.do2d_response("P1", -1.0, 2.0, 7, "P2", 0.0, 3.0, 5)
    c = model._b.calls[-1]
    assert s.shape == (5, 7, 1) and dsx.shape == dsy.shape == (5, 7) and dnx.shape == dny.shape == (5, 7, N)
    assert not dsx.any() and np.all(dsy == 2.0) and np.all(dnx == 1.0) and not dny.any()
    assert c["n_charge"] is None and c["args"][9] == 8.617333262145e-5 * 120.0 and c["frame"] == "physical" and c["gamma"] == 0.3
    assert set(c["response"]) == {"dsignal_axes", "docc_axes"} and c["args"][3:7] == ((-1.0, 2.0), (0.0, 3.0), 7, 5)
    model.do2d_response("vP1", -1, 2, 3, "e1_2", 0, 3, 4, T=77.0, n_charge=3)
    c = model._b.calls[-1]
    assert c["n_charge"] == 3 and c["args"][9] == 8.617333262145e-5 * 77.0 and c["frame"] == "virtual"
    with pytest.raises(NotImplementedError):
        model.do2d_response("P1", 0, 1, 3, "vP2", 0, 1, 3)
    s, dsx, dsy, dnx, dny = model.do1d_response("P3", -1.0, 1.0, 9, T=50.0)
    c = model._b.calls[-1]
    assert s.shape == (9, 1) and dsx.shape == (9,) and dnx.shape == (9, N) and c["args"][5:7] == (9, 1)
    assert not np.asarray(c["args"][2]).any() and c["args"][4] == (0.0, 0.0)
    with pytest.raises(ValueError, match="raw"):
        ModelFacade(Stub(np.nan), N).do2d_response("P1", 0, 1, 3, "P2", 0, 1, 3)


def test_vec_env_refuses_before_the_device():
    from qadapt_hip import _lib
    from qadapt_hip.vec_env import VecQuantumDeviceEnv

    class Bare:
        N, R, noise_flags = 3, 8, _lib.QD_NOISE_SENSOR | _lib.QD_NOISE_LATCH | _lib.QD_NOISE_RADIAL
        RESPONSE_OUTPUTS = VecQuantumDeviceEnv.RESPONSE_OUTPUTS
        _noise_flags = VecQuantumDeviceEnv._noise_flags
        _scan_grid = VecQuantumDeviceEnv._scan_grid

        def _query_inputs(self, env_ids, gv, bv, sv):
            return 2, None, None, None, None

        def _to_dev(self, *a):
            raise AssertionError("reached the device")

    grid = lambda kT, **kw: VecQuantumDeviceEnv.scan_grid_response(Bare(), [0, 1], 0, 1, (0, 1), (0, 1), 4, 4, None, None, kT, **kw)   # noqa: E731
    with pytest.raises(ValueError, match="needs kT"):
        grid(None)
    with pytest.raises(ValueError, match="response must name"):
        grid(0.01, response=())
    with pytest.raises(ValueError, match="response must name"):
        grid(0.01, response=("chi", "dchi"))
    with pytest.raises(ValueError, match="latch"):
        grid(0.01, noise=("latch",))
    with pytest.raises(ValueError, match="kT must be finite"):
        grid(0.0)
    with pytest.raises(AssertionError, match="reached the device"):
        grid([0.01, 0.02], noise=("sensor",), response=("chi",))


def test_sanitizer_program_runs_clean():
    """the epilogue behind the per-component thermal core under AddressSanitizer and UBSan, as a stand-alone program in a child
    process; nothing is loaded into Python under a sanitizer"""
    subprocess.check_call(["make", "-s", "-C", HDIR, "qd_response_blocks_asan"])
    r = subprocess.run([os.path.join(HDIR, "qd_response_blocks_asan")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "response blocks asan ok" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
