"""The per-component energy-level core on the MI355X (run with -m gpu): csrc/qd_levels_blocks.h behind qd_levels_load_packed in
persistent single-wave blocks (tests/gputest_levels_blocks, the shape of qd_k_levels_grid) on the matrices of
tests/test_levels_blocks_cpu.py -- the families at every size 1..32, the block-diagonal compositions with scattered members at
every L, the exact cases -- within the CPU file's bar, 1e-12 ||A||_inf of numpy.linalg.eigvalsh, with the labels the workspace
shows on the device against a plain BFS; the device against the host build; and a task list whose neighbours differ in size and
partition, run by 1, 7 and 256 blocks with the workspace as found, poisoned once and poisoned before every task: the same bits
in all nine runs, no NaN.  Masks, member list, per-state bytes, t and the tridiagonal are all state a second point could
inherit.  The harness and the tests only feed matrices."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest

import eig_cases as EC
import helpers as H
import test_levels_blocks_cpu as LC
from test_gpu_eig_device import same_bits
from test_levels_cpu import BAR

pytestmark = pytest.mark.gpu

SIZES = [1] + EC.LANE_SIZES
_LIB = None
_WORST = {"lev": 0.0, "n": 0}


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(H.ROOT, "tests", "gputest_levels_blocks", "libqdsim_gputest_levels_blocks.so")
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found: build it with __graft_entry__.build() (or make -C tests/gputest_levels_blocks)")
        import torch  # noqa: F401  (first: the harness then shares torch's HIP runtime, as qadapt_hip._lib.lib() does)
        _LIB = ctypes.CDLL(path)
        dp, ip, ci = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.c_int
        _LIB.qdgl_levels_blocks.argtypes = [ci, ip, dp, ci, ip, ci, ci, dp, ip, ctypes.c_char_p, ci]
        _LIB.qdgl_levels_blocks.restype = ci
    return _LIB


def dev(mats, nlev, blocks=0, poison=0):
    """one launch: lev (n, 8; +inf from min(L, s) on), label (n, 32; -1 from s on)"""
    n = len(mats)
    sizes = np.array([A.shape[0] for A in mats], np.int32)
    smax = int(sizes.max())
    ld = smax * (smax + 1) // 2
    pk = np.zeros((n, ld))
    for t, A in enumerate(mats):
        p = EC.packed(A)
        pk[t, :len(p)] = p
    nl = np.ascontiguousarray(np.broadcast_to(np.asarray(nlev, np.int32), (n,)))
    r = types.SimpleNamespace(lev=np.zeros((n, 8)), label=np.zeros((n, 32), np.int32))
    err = ctypes.create_string_buffer(512)
    d, ci = ctypes.c_double, ctypes.c_int
    rc = lib().qdgl_levels_blocks(n, H._p(sizes, ci), H._p(pk, d), ld, H._p(nl, ci), int(blocks), int(poison), H._p(r.lev, d),
                                  H._p(r.label, ci), err, len(err))
    assert rc == 0, (rc, err.value.decode())
    return r


def check(A, L, r, t, tag):
    """the checks of test_levels_blocks_cpu.check on task t of the device result r"""
    s = A.shape[0]
    n = min(L, s)
    lev = r.lev[t]
    assert np.isfinite(lev[:n]).all() and np.all(np.isposinf(lev[n:])), (tag, lev)
    assert np.all(np.diff(lev[:n]) >= 0), (tag, lev)
    assert np.array_equal(r.label[t, :s], LC.bfs_labels(A)) and np.all(r.label[t, s:] == -1), (tag, r.label[t])
    hn = EC.hnorm(A)
    err = np.abs(lev[:n] - np.linalg.eigvalsh(A)[:n]).max()
    assert err <= BAR * hn, (tag, s, L, err / hn if hn else err)
    _WORST["lev"] = max(_WORST["lev"], float(err / hn) if hn else 0.0)
    _WORST["n"] += 1


@functools.lru_cache(maxsize=None)
def family(s):
    """(tag, A, L) of every task of size s: the blocks of test_levels_blocks_cpu.test_families_of_every_size at L = min(8, s)"""
    fam = [(("hop", t), A) for t, A in EC.scale_family(s)]
    if s >= 2:
        for sep in (1e-5, 1e-7, 3e-9):
            fam += [(("near", sep, tc), A) for tc, A, _ in EC.near_degenerate_family(s, sep)]
    fam += [(("mixed", k), A) for k, A in enumerate(EC.mixed_scale_family(s))]
    fam += [(("extreme", k), A) for k, A in enumerate(EC.extreme_scale_family(s, reps=60))]
    fam.append(("classical", EC.classical_block(s)))
    return [(tag, A, min(8, s)) for tag, A in fam]


@functools.lru_cache(maxsize=None)
def family_solved(s):
    tasks = family(s)
    return dev([A for _, A, _ in tasks], [L for _, _, L in tasks])


@pytest.mark.parametrize("s", SIZES)
def test_families_of_every_size(s):
    tasks, r = family(s), family_solved(s)
    for t, (tag, A, L) in enumerate(tasks):
        check(A, L, r, t, tag)


@functools.lru_cache(maxsize=None)
def compositions():
    """the block-diagonal compositions of the CPU file: every partition, dealt round-robin and randomly permuted, four scales,
    every L in 1..8; and its small sizes at every L"""
    out = []
    for name in LC.ALL_PARTITIONS:
        for tscale, A in LC.partition_cases(name):
            out += [((name, tscale, L), A, L) for L in range(1, 9)]
    rng = np.random.default_rng(11)
    for s in (2, 3, 4, 5, 7, 9):
        for sizes in ([s], [1] * s, [s - 1, 1], [2] + [1] * (s - 2)):
            A = LC.composition(rng, sizes, 0.3, rng.permutation(s))
            out += [(("small", s, tuple(sizes), L), A, L) for L in range(1, 9)]
    for a in (0.0, -3.5, 1e5, 1e-300):
        out += [(("one", a, L), np.array([[a]]), L) for L in (1, 2, 8)]
    out += [(("tail", L), EC.column_tail_block(), L) for L in range(1, 9)] + [("small entry", EC.small_entry_block(), 8)]
    return out


def test_block_diagonal_compositions_with_scattered_members():
    tasks = compositions()
    r = dev([A for _, A, _ in tasks], [L for _, _, L in tasks])
    for t, (tag, A, L) in enumerate(tasks):
        check(A, L, r, t, tag)
        if tag[0] == "one":
            assert r.lev[t, 0] == A[0, 0]


def test_exact_cases():
    """zero couplings: the sorted diagonal exactly; two identical components with interleaved members: levels 2k and 2k + 1
    bitwise equal; a denormal link and an exact zero"""
    rng = np.random.default_rng(5)
    mats, what = [], []
    for s in EC.LANE_SIZES:
        r2 = np.random.default_rng(500 + s)
        mats += [EC.classical_block(s), np.diag(4096.0 + r2.integers(0, 2 ** 20, s) / 2.0 ** 19)]; what += ["diag", "diag"]
    for m in (2, 3, 4, 7, 16):
        mats.append(np.kron(EC.hop_block(rng, m, 0.7), np.eye(2))); what.append("twins")
    r3 = np.random.default_rng(77)
    for scale in (0.4, 1.0, 37.0):
        A = LC.composition(r3, [3, 2, 4, 1], 0.1, np.arange(10)) * scale
        B = A.copy(); B[1, 4] = B[4, 1] = 5e-324
        C = A.copy(); C[1, 4] = C[4, 1] = 0.0; C[9, 0] = C[0, 9] = -0.0
        mats += [A, B, C]; what += ["links4", "links3", "links4"]
    r = dev(mats, 8)
    for t, (A, w) in enumerate(zip(mats, what)):
        s = A.shape[0]
        L = min(8, s)
        check(A, 8, r, t, (w, t))
        if w == "diag":
            assert np.array_equal(r.lev[t, :L], np.sort(np.diag(A))[:L]), (t, s)
            assert np.array_equal(r.label[t, :s], np.arange(s))
        elif w == "twins":
            assert r.label[t, :s].tolist() == [0, 1] * (s // 2)
            for k in range(L):
                assert r.lev[t, k] == r.lev[t, (k // 2) * 2], (t, r.lev[t])
        else:
            assert len(np.unique(r.label[t, :s])) == int(w[-1]), (t, r.label[t, :s])


@pytest.mark.parametrize("s", SIZES)
def test_device_against_host_build(s):
    """the same source with the 64 lanes as a loop: the same labels and the same levels BIT FOR BIT.  qd_rcp and qd_sqrt1 round
    correctly on the Householder step's arguments and the Sturm recurrence divides in IEEE on both sides, so both builds bisect
    the same tridiagonal (the finding of test_gpu_spectrum_device.py for the whole-block core)"""
    tasks, r = family(s), family_solved(s)
    for t, (tag, A, L) in enumerate(tasks):
        lev, lab, _, _, _ = LC.solve(A, L)
        assert np.array_equal(lab, r.label[t, :s]), tag
        assert same_bits(lev, r.lev[t, :L]), (tag, s, lev - r.lev[t, :L])


# ---------------------------------------------------------------------------------------------------------------
# independence from neighbours, block count and stale LDS
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_list():
    """(mats, L, what): neighbours that differ in size and partition -- one 32-state component then one state, then a 2 x 1
    partition of 2 states (a stale be at a component end); ten components of 3 and one of 2 then one 32-state component; a
    3-state component among singles then 16 pairs then 32 single states; the largest component first, then last; whole-block
    blocks of mixed sizes in between; L cycling through 1..8"""
    rng = np.random.default_rng(778)
    P = LC.ALL_PARTITIONS
    mats, what = [], []

    def add(A, name):
        mats.append(A); what.append(name)

    lane = {s: iter(list(EC.lane_mix_family(s, 40))) for s in (32, 31, 17, 7, 5, 4, 2)}
    for rnd in range(16):
        tscale = (1e-3, 1.0, 30.0, 1e-8)[rnd % 4]
        perm = rng.permutation(32) if rnd % 2 else LC.interleave(P["10x3+2"])
        add(next(lane[32]), "32"); add(np.array([[rng.uniform(-3, 3)]]), "1"); add(np.diag(rng.uniform(-1, 1, 2)), "2x1")
        add(LC.composition(rng, P["10x3+2"], tscale, perm), "10x3+2"); add(next(lane[32]), "32")
        add(next(lane[7]), "7"); add(next(lane[4]), "4")
        add(LC.composition(rng, [5, 3, 3, 2, 1], tscale, rng.permutation(14)), "5+3+3+2+1")
        add(LC.composition(rng, [4, 2], tscale, rng.permutation(6)), "4+2")
        add(LC.composition(rng, P["3+29x1"], tscale, rng.permutation(32)), "3+29x1")
        add(LC.composition(rng, P["16x2"], tscale, rng.permutation(32)), "16x2"); add(EC.classical_block(32), "32x1")
        add(LC.composition(rng, P["20+5+4+3"], tscale, np.arange(32)), "20+5+4+3")
        add(LC.composition(rng, P["3+4+5+20"], tscale, np.arange(32)), "3+4+5+20")
        add(LC.composition(rng, P["17+15"], tscale, rng.permutation(32)), "17+15"); add(next(lane[17]), "17")
        add(next(lane[31]), "31"); add(next(lane[2]), "2")
        add(LC.composition(rng, P["1+2+..+7+4"], tscale, rng.permutation(32)), "1+2+..+7+4"); add(next(lane[5]), "5")
    L = [1 + (3 * t + t // 20) % 8 for t in range(len(mats))]
    return mats, L, what


def test_mixed_list_has_the_neighbours_it_promises():
    mats, L, what = mixed_list()
    pairs = set(zip(what[:-1], what[1:]))
    assert lib().qdgl_ws_bytes() == LC.WS_BYTES                            # (the harness is built from the header the CPU file pins)
    assert len(mats) == 320 and set(L) == set(range(1, 9))
    assert {("32", "1"), ("1", "2x1"), ("10x3+2", "32"), ("7", "4"), ("3+29x1", "16x2"), ("16x2", "32x1"), ("31", "2")} <= pairs
    for A, name in zip(mats, what):
        if "+" in name or "x" in name:
            assert len(np.unique(LC.bfs_labels(A))) > 1, name


RUNS = [(blocks, poison) for blocks in (1, 7, 256) for poison in (0, 1, 2)]


@functools.lru_cache(maxsize=None)
def mixed_solved(blocks, poison):
    mats, L, _ = mixed_list()
    return dev(mats, L, blocks=blocks, poison=poison)


@pytest.mark.parametrize("blocks,poison", RUNS)
def test_core_does_not_depend_on_neighbours_blocks_or_stale_lds(blocks, poison):
    """one wave solving the whole list in order, seven blocks, 256 blocks, each with the workspace as found, poisoned once and
    poisoned before every task: the bits of (blocks = 256, poison = 2)"""
    mats, L, what = mixed_list()
    base, got = mixed_solved(256, 2), mixed_solved(blocks, poison)
    assert not np.isnan(got.lev).any(), (blocks, poison, np.argwhere(np.isnan(got.lev))[:8])
    for t in range(len(mats)):
        assert same_bits(got.lev[t], base.lev[t]), (blocks, poison, t, what[t], what[t - 1] if t else None)
        assert np.array_equal(got.label[t], base.label[t]), (blocks, poison, t, what[t])
    if (blocks, poison) == (1, 0):                         # equal bits are not two wrong answers
        for t, A in enumerate(mats):
            check(A, L[t], got, t, ("mixed list", t, what[t]))
        print(f"[levels blocks device] {_WORST['n']} tasks so far: worst |level - eigvalsh| / ||A||_inf {_WORST['lev']:.2e} (bar {BAR:.0e})")
