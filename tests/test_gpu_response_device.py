"""The charge-response epilogue on the MI355X (run with -m gpu): csrc/qd_response.h behind qd_levels_load_packed and the unchanged
thermal core in persistent single-wave blocks (tests/gputest_response, the shape of qd_k_thermal_response) on the matrices of
tests/test_response_cpu.py -- response_helpers.family at every size 1..32: the eigen-solver families at kT = 1e-6 .. 1e3 hs and
the designed cases (exact degeneracies, level pairs at x = 1e-14, 1e-8, 1e-3, zero and denormal couplings) -- within the CPU
file's bound, every block compared, from LDS poisoned with NaN bits before every task; and a task list whose neighbours differ in
size, run by 1, 7 and 256 blocks with the workspace as found, poisoned once and poisoned before every task: the same bits in all
nine runs, no NaN.  Worst err / tol measured on an MI355X over the 5 737 blocks: 2.0e-3 (sizes 25..32; also in DESIGN 7, "Charge
response")."""
import ctypes
import os

import numpy as np
import pytest

import eig_cases as EC
import helpers as H
import response_helpers as RH
from test_gpu_eig_device import same_bits
from test_response_cpu import pack_perts

pytestmark = pytest.mark.gpu

_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(H.ROOT, "tests", "gputest_response", "libqdsim_gputest_response.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found: build it with __graft_entry__.build() (or make -C tests/gputest_response)")
        import torch  # noqa: F401  (first: the harness then shares torch's HIP runtime, as qadapt_hip._lib.lib() does)
        _LIB = ctypes.CDLL(path)
        dp, ip, ci, bp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_uint8)
        _LIB.qdgr_response.argtypes = [ci, ip, dp, ci, dp, ci, ip, dp, bp, ci, ci, dp, dp, ctypes.c_char_p, ci]
        _LIB.qdgr_response.restype = ci
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
    rc = lib().qdgr_response(n, H._p(sizes, ci), H._p(pk, d), ld, H._p(kT, d), len(kind), H._p(kind, ci), H._p(x, d),
                             H._p(nb, ctypes.c_uint8), int(blocks), int(poison), H._p(dP, d), H._p(pop, d), err, len(err))
    assert rc == 0, (rc, err.value.decode())
    return dP, pop


@pytest.mark.parametrize("sizes", [range(1, 9), range(9, 17), range(17, 25), range(25, 33)], ids=["1-8", "9-16", "17-24", "25-32"])
def test_families_of_every_size(sizes):
    """every block of the CPU tier's families in one launch per group of sizes, LDS poisoned before every task"""
    tasks, tags = [], []
    for s in sizes:
        nt, Ts = RH.probe(s, 0)
        for tag, A, kT in RH.family(s):
            tasks.append((A, kT, nt, Ts)); tags.append((s, tag, kT))
    dP, _ = dev(tasks, poison=2)
    assert np.isfinite(dP).all()
    worst = {}
    for t, (A, kT, nt, Ts) in enumerate(tasks):
        s = A.shape[0]
        assert not dP[t, :, s:].any(), tags[t]
        if s == 1:
            assert not dP[t].any()
        r = RH.block_check(A, kT, nt, Ts, dP[t, :, :s])
        assert r <= 1.0, (tags[t], r)
        k = RH.kind(tags[t][1])
        worst[k] = max(worst.get(k, 0.0), r)
    print(f"[response device] sizes {sizes[0]}..{sizes[-1]}: {len(tasks)} blocks, worst err / tol per family: "
          + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_results_do_not_depend_on_neighbours_block_count_or_stale_lds():
    """a list in which a block of 32 states is followed by one of 1, 2, 31, 5 ... states: 1, 7 and 256 persistent blocks, LDS as
    found, poisoned once and poisoned before every task"""
    order = [32, 1, 2, 31, 5, 32, 17, 3, 24, 1, 9, 30, 4, 16, 7, 2]
    tasks = []
    for rep in range(6):
        for s in order:
            nt, Ts = RH.probe(s, 0)
            fam = RH.family(s)
            tag, A, kT = fam[(7 * rep + s) % len(fam)]
            tasks.append((A, kT, nt, Ts))
    base, pop0 = dev(tasks, blocks=0, poison=2)
    assert np.isfinite(base).all()
    for blocks in (1, 7, 256):
        for poison in (0, 1, 2):
            dP, pop = dev(tasks, blocks=blocks, poison=poison)
            assert same_bits(dP, base) and same_bits(pop, pop0), (blocks, poison)
    rev, _ = dev(tasks[::-1], blocks=5, poison=0)
    assert same_bits(rev[::-1], base)


def test_bad_arguments_are_refused_before_a_launch():
    nt, Ts = RH.probe(4, 0)
    A = np.diag([0.0, 1.0, 2.0, 3.0])
    n = 1
    sizes = np.array([4], np.int32)
    kind, x, nb = pack_perts(nt, Ts)
    d, ci = ctypes.c_double, ctypes.c_int
    dP, pop = np.zeros((1, len(kind), 32)), np.zeros((1, 32))
    err = ctypes.create_string_buffer(256)

    def call(sizes=sizes, kT=0.1, nb=nb, poison=0, blocks=0):
        return lib().qdgr_response(n, H._p(sizes, ci), H._p(EC.packed(A), d), 10, H._p(np.array([kT]), d), len(kind), H._p(kind, ci),
                                   H._p(np.ascontiguousarray(x[None]), d), H._p(np.ascontiguousarray(nb[None]), ctypes.c_uint8),
                                   blocks, poison, H._p(dP, d), H._p(pop, d), err, len(err))

    assert call() == 0
    assert call(sizes=np.array([33], np.int32)) == 1 and call(sizes=np.array([0], np.int32)) == 1
    assert call(kT=0.0) == 1 and call(kT=np.nan) == 1 and call(poison=3) == 1 and call(blocks=-1) == 1
    far = nb.copy(); far[len(kind) - 2, 0, 0] = 4
    assert call(nb=far) == 1 and b"partner" in err.value
