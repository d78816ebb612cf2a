"""The per-component charge-response epilogue on the MI355X (run with -m gpu): csrc/qd_response_blocks.h behind
qd_levels_load_packed and the unchanged per-component thermal core in persistent single-wave blocks
(tests/gputest_response_blocks, the shape of qd_k_thermal_grid_response) on the matrices of tests/test_response_blocks_cpu.py --
response_helpers.family at every size 1..32 and the block-diagonal compositions with scattered members of
test_thermal_blocks_cpu.PARTITIONS -- within the CPU file's bound (response_helpers.tol_chi as it is), every block compared, from
LDS poisoned with NaN bits before every task; and a task list whose neighbours differ in size and partition, run by 1, 7 and 256
blocks with the workspace as found, poisoned once and poisoned before every task, and in reverse order: the same bits in all
runs, no NaN.  Worst err / tol measured on an MI355X: the 5 737 family blocks 2.0e-3 (near-degenerate, sizes 25..32), the 180
compositions 4.9e-4 (31+1); also in DESIGN 7, "Charge-response grids"."""
import ctypes
import os

import numpy as np
import pytest

import eig_cases as EC
import helpers as H
import response_helpers as RH
import test_thermal_blocks_cpu as TBC
from test_gpu_eig_device import same_bits
from test_response_blocks_cpu import partition_probe, respect
from test_response_cpu import pack_perts

pytestmark = pytest.mark.gpu

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(H.ROOT, "tests", "gputest_response_blocks", "libqdsim_gputest_response_blocks.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found: build it with __graft_entry__.build() (or make -C tests/gputest_response_blocks)")
        import torch  # noqa: F401  (first: the harness then shares torch's HIP runtime, as qadapt_hip._lib.lib() does)
        _LIB = ctypes.CDLL(path)
        dp, ip, ci, bp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_uint8)
        _LIB.qdgrb_response.argtypes = [ci, ip, dp, ci, dp, ci, ip, dp, bp, ci, ci, dp, dp, ctypes.c_char_p, ci]
        _LIB.qdgrb_response.restype = ci
        _LIB.qdgrb_record.argtypes = [ci, ctypes.POINTER(ctypes.c_uint16), ctypes.POINTER(ctypes.c_int32), dp, dp, dp, ci, ci,
                                      ctypes.c_double, dp, ci, dp, dp, dp, dp, ctypes.c_char_p, ci]
        _LIB.qdgrb_record.restype = ci
    return _LIB


def dev(tasks, blocks=0, poison=0):
    """one launch over tasks [(A, kT, nt, Ts)] with the same number of columns and patterns: dP (n, npert, 32), pop (n, 32)"""
    n = len(tasks)
    sizes = np.array([t[0].shape[0] for t in tasks], np.int32)
    smax = int(sizes.max())
    ld = smax * (smax + 1) // 2
    pk = np.zeros((n, ld))
    kT = np.array([t[1] for t in tasks], np.float64)
    packs = [pack_perts(t[2], t[3]) for t in tasks]
    kind = packs[0][0]
    assert all(np.array_equal(p[0], kind) for p in packs)
    x = np.ascontiguousarray(np.stack([p[1] for p in packs]))
    nb = np.ascontiguousarray(np.stack([p[2] for p in packs]))
    for t, task in enumerate(tasks):
        p = EC.packed(task[0])
        pk[t, :len(p)] = p
    dP, pop = np.zeros((n, len(kind), 32)), np.zeros((n, 32))
    err = ctypes.create_string_buffer(512)
    d, ci = ctypes.c_double, ctypes.c_int
    rc = lib().qdgrb_response(n, H._p(sizes, ci), H._p(pk, d), ld, H._p(kT, d), len(kind), H._p(kind, ci), H._p(x, d),
                              H._p(nb, ctypes.c_uint8), int(blocks), int(poison), H._p(dP, d), H._p(pop, d), err, len(err))
    assert rc == 0, (rc, err.value.decode())
    return dP, pop


def _check_all(tasks, tags, dP):
    assert np.isfinite(dP).all()
    worst = {}
    for t, (A, kT, nt, Ts) in enumerate(tasks):
        s = A.shape[0]
        assert not dP[t, :, s:].any(), tags[t]
        if s == 1:
            assert not dP[t].any()
        r = RH.block_check(A, kT, nt, Ts, dP[t, :, :s])
        assert r <= 1.0, (tags[t], r)
        k = tags[t][0]
        worst[k] = max(worst.get(k, 0.0), r)
    return worst


@pytest.mark.parametrize("sizes", [range(1, 9), range(9, 17), range(17, 25), range(25, 33)], ids=["1-8", "9-16", "17-24", "25-32"])
def test_families_of_every_size(sizes):
    """every block of the CPU tier's families in one launch per group of sizes, LDS poisoned before every task"""
    tasks, tags = [], []
    for s in sizes:
        nt, Ts0 = RH.probe(s, 0)
        for tag, A, kT in RH.family(s):
            tasks.append((A, kT, nt, respect(Ts0, A))); tags.append((RH.kind(tag), s, tag, kT))
    dP, _ = dev(tasks, poison=2)
    worst = _check_all(tasks, tags, dP)
    print(f"[response blocks device] sizes {sizes[0]}..{sizes[-1]}: {len(tasks)} blocks, worst err / tol per family: "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def _partition_tasks():
    tasks, tags = [], []
    for name, sizes in TBC.PARTITIONS.items():
        rng = np.random.default_rng(sum(ord(c) for c in name) + 1)
        for tscale in (1e-3, 1.0, 30.0):
            for k, perm in enumerate((TBC.interleave(sizes), rng.permutation(32))):
                A = TBC.composition(rng, sizes, tscale, perm)
                nt, Ts = partition_probe(A, k)
                for kT in RH.temperatures(A):
                    tasks.append((A, kT, nt, Ts)); tags.append((name, tscale, k, kT))
    return tasks, tags


def test_block_diagonal_compositions_with_scattered_members():
    """the partitions of the CPU tier (10x3+2, 16x2, 32x1, 31+1, 17+15, 1+2+..+7+4), the same matrices, in one launch; 32x1: the
    hop columns exactly 0.0"""
    tasks, tags = _partition_tasks()
    dP, _ = dev(tasks, poison=2)
    worst = _check_all(tasks, tags, dP)
    for t, tag in enumerate(tags):
        if tag[0] == "32x1":
            assert not dP[t, 3:].any()
    print(f"[response blocks device] {len(tasks)} compositions, worst err / tol per partition: "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_results_do_not_depend_on_neighbours_block_count_or_stale_lds():
    """a list in which a block of 32 states in one component is followed by one of 1 state, one of 32 in eleven components, one
    of 2 ...: 1, 7 and 256 persistent blocks, LDS as found, poisoned once and poisoned before every task, and the reverse order"""
    ptasks, _ = _partition_tasks()
    order = [32, 1, 2, 31, 5, 32, 17, 3, 24, 1, 9, 30, 4, 16, 7, 2]
    tasks = []
    for rep in range(4):
        for i, s in enumerate(order):
            nt, Ts0 = RH.probe(s, 0)
            fam = RH.family(s)
            tag, A, kT = fam[(7 * rep + s) % len(fam)]
            tasks.append((A, kT, nt, respect(Ts0, A)))
            tasks.append(ptasks[(13 * (rep * len(order) + i)) % len(ptasks)])
    base, pop0 = dev(tasks, blocks=0, poison=2)
    assert np.isfinite(base).all()
    for blocks in (1, 7, 256):
        for poison in (0, 1, 2):
            dP, pop = dev(tasks, blocks=blocks, poison=poison)
            assert same_bits(dP, base) and same_bits(pop, pop0), (blocks, poison)
    rev, _ = dev(tasks[::-1], blocks=5, poison=0)
    assert same_bits(rev[::-1], base)


def dev_record(N, idx, fl, tc, E, vpp, nvalid, K, kT, par, poison):
    """one point of the grid kernel's body on a hand-made record: chi (N, 2N-1), jac (N, 2N), dsignal (2N,), c0"""
    chi, jac, ds, c0 = np.full((N, 2 * N - 1), np.nan), np.full((N, 2 * N), np.nan), np.full(2 * N, np.nan), np.full(1, np.nan)
    err = ctypes.create_string_buffer(512)
    d = ctypes.c_double
    c = lambda a, t: np.ascontiguousarray(a, t)                             # noqa: E731
    rc = lib().qdgrb_record(N, H._p(c(idx, np.uint16), ctypes.c_uint16), H._p(c(fl, np.int32), ctypes.c_int32), H._p(c(tc, np.float64), d),
                            H._p(c(E, np.float64), d), H._p(c(vpp, np.float64), d), int(nvalid), K, kT, H._p(c(par, np.float64), d),
                            int(poison), H._p(chi, d), H._p(jac, d), H._p(ds, d), H._p(c0, d), err, len(err))
    assert rc == 0, (rc, err.value.decode())
    return chi, jac, ds, float(c0[0])


@pytest.mark.parametrize("N", [2, 4, 8])
def test_a_record_without_a_valid_state_gives_zeros_and_the_slope_at_no_charge(N):
    """nvalid = 0, the record the searches never produce, through the body of a point of qd_k_thermal_grid_response with LDS as found
    and poisoned with NaN bits: it counts as |0..0>, chi and the jacobian are zero exactly, and dsignal is S'(c0) dc0/dv at
    <n> = 0 (response_helpers.empty_reference) within 64 eps.  The same body on a record WITH valid states agrees with the host
    build of the same source within the sum of both tolerances (the harness is wired as the host one is)"""
    import qd_oracle as O
    import thermal_helpers as TH
    from test_levels_cpu import _record_fields, n_valid
    from test_response_blocks_cpu import _host_record
    rng = np.random.default_rng(4100 + N)
    par = H.sample_blocks(N, [61]).params[0]
    lay = H.layout(N)
    dev_ = H.dev_view(N, par)
    gamma = float(par[lay.scal + 1])
    worst = 0.0
    for p in range(6):
        v_ext = np.concatenate([par[lay.vopt:lay.vopt + N + 1] + rng.uniform(-4, 4, N + 1),
                                par[lay.vbopt:lay.vbopt + N - 1] + rng.uniform(-3, 3, N - 1)])
        vpp = dev_.cgd_full @ v_ext
        want = RH.empty_reference(dev_, v_ext, gamma)
        for poison in (0, 1):
            chi, jac, ds, c0 = dev_record(N, np.zeros(32), np.zeros(N), rng.uniform(0.01, 0.1, N - 1), np.zeros(32), vpp, 0, 8, 0.01,
                                          par, poison)
            assert not chi.any() and not jac.any(), (p, poison)
            r = np.abs(ds - want) / (64 * np.finfo(np.float64).eps * np.abs(want))
            assert np.all(r <= 1.0), (p, poison, float(r.max()))
            worst = max(worst, float(r.max()))
    print(f"[response blocks device] no valid state N={N}: zeros exactly, worst |dsignal - slope at <n> = 0| / (64 eps) {worst:.2e}")
    # a record with valid states: the device body against the host build
    K = 8
    v = np.concatenate([par[lay.vopt:lay.vopt + N + 1] + rng.uniform(-2, 2, (4, N + 1)),
                        par[lay.vbopt:lay.vbopt + N - 1] + rng.uniform(-1, 1, (4, N - 1))], axis=1)
    states, _ = O.candidate_states(v, dev_.cdd_inv_full, dev_.cgd_full, N, k=K)
    F = O.free_energy_states(v, dev_.cdd_inv_full, dev_.cgd_full, states, N)
    tc = O.tunnel_couplings(O.effective_barrier_potential(v[:, :N + 1], v[:, N + 1:], dev_.Cbg, dev_.Cbb), dev_.tc_base, dev_.alpha)
    nvs, floors = n_valid(v, dev_, N, K)
    kT = TH.KB_REF * 100
    for p in range(4):
        nv = int(nvs[p])
        idx, E = _record_fields(N, states[p], floors[p], F[p], nv)
        st = states[p, :nv].astype(np.int64)
        Hm = np.diag(F[p, :nv]) + O.tunnel_hamiltonian(tc[p][None], st[None])[0]
        ref = RH.point_reference(dev_, Hm, st, tc[p], kT, v[p], gamma)
        chi, jac, ds, c0 = dev_record(N, idx, floors[p], tc[p], E, dev_.cgd_full @ v[p], nv, K, kT, par, 1)
        hchi, hjac, _, _, _ = _host_record(N, idx, floors[p], tc[p], E, nv, K, kT, par)
        assert np.all(np.abs(chi - hchi) <= 2 * np.maximum(ref["tol_chi"], 5e-324)[None, :]), p
        assert np.all(np.abs(jac - hjac) <= 2 * ref["tol_jac"][None, :]), p
        assert np.all(np.abs(ds - ref["dsignal"]) <= ref["tol_dsignal"]), p


def test_bad_arguments_are_refused_before_a_launch():
    nt, Ts = RH.probe(4, 0)
    A = np.diag([0.0, 1.0, 2.0, 3.0])
    sizes = np.array([4], np.int32)
    kind, x, nb = pack_perts(nt, Ts)
    d, ci = ctypes.c_double, ctypes.c_int
    dP, pop = np.zeros((1, len(kind), 32)), np.zeros((1, 32))
    err = ctypes.create_string_buffer(256)

    def call(sizes=sizes, kT=0.1, nb=nb, poison=0, blocks=0):
        return lib().qdgrb_response(1, H._p(sizes, ci), H._p(EC.packed(A), d), 10, H._p(np.array([kT]), d), len(kind), H._p(kind, ci),
                                    H._p(np.ascontiguousarray(x[None]), d), H._p(np.ascontiguousarray(nb[None]), ctypes.c_uint8),
                                    blocks, poison, H._p(dP, d), H._p(pop, d), err, len(err))

    assert call(sizes=np.array([33], np.int32)) == 1 and call(sizes=np.array([0], np.int32)) == 1
    assert call(kT=0.0) == 1 and call(kT=np.nan) == 1 and call(poison=3) == 1 and call(blocks=-1) == 1
    far = nb.copy(); far[len(kind) - 2, 0, 0] = 4
    assert call(nb=far) == 1 and b"partner" in err.value
