"""The per-component thermal core on the MI355X (run with -m gpu): csrc/qd_thermal_blocks.h behind qd_levels_load_packed in
persistent single-wave blocks (tests/gputest_thermal_blocks, the shape of qd_k_thermal_grid) on the matrices of
tests/test_thermal_blocks_cpu.py -- the families of eig_cases.py at every size 1..32 and the block-diagonal compositions with
scattered members -- within the CPU file's bars, with the structure the workspace shows on the device (labels against a plain
BFS, A exactly symmetric, A and V exactly zero between components); the device against the host build; and a task list whose
neighbours differ in size and partition, run by 1, 7 and 256 blocks with the workspace as found, poisoned once and poisoned
before every task: the same bits in all nine runs, no NaN.  Labels, member lists, item lists and the 32-entry round arrays are all
state a second point could inherit; the sensitivity of the last test to one removed initialisation is recorded in DESIGN 7."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest

import eig_cases as EC
import helpers as H
import thermal_helpers as TH
import test_thermal_blocks_cpu as BC
from test_gpu_eig_device import same_bits
from test_thermal_cpu import tol_ztail, _temperatures

pytestmark = pytest.mark.gpu

SIZES = [1] + EC.LANE_SIZES
EPS = np.finfo(np.float64).eps
OFF_BAR = 2.0 ** -56                                    # QD_TH_THRESH: what a converged sweep leaves off the diagonal
FIELDS = ("pop", "lam", "ztail", "sweeps", "label", "asym", "cross", "V")
_LIB = None
_WORST = {"pop": 0.0, "ztail": 0.0, "resid": 0.0, "orth": 0.0, "sweeps": 0, "n": 0, "dpop": 0.0, "dztail": 0.0}


def lib():
    global _LIB
    if _LIB is None:
        # QDSIM_GPUTEST_THERMAL_BLOCKS_LIB: a diagnostic build of the harness (a sensitivity check with a changed header, say)
        path = os.environ.get("QDSIM_GPUTEST_THERMAL_BLOCKS_LIB",
                              os.path.join(H.ROOT, "tests", "gputest_thermal_blocks", "libqdsim_gputest_thermal_blocks.so"))
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found: build it with __graft_entry__.build() (or make -C tests/gputest_thermal_blocks)")
        import torch  # noqa: F401  (first: the harness then shares torch's HIP runtime, as qadapt_hip._lib.lib() does)
        _LIB = ctypes.CDLL(path)
        dp, ip, ci = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.c_int
        _LIB.qdgb_thermal.argtypes = [ci, ip, dp, ci, dp, ci, ci, dp, dp, dp, ip, ip, dp, dp, dp, ctypes.c_char_p, ci]
        _LIB.qdgb_thermal.restype = ci
    return _LIB


def dev(mats, kT, blocks=0, poison=0, want_v=True):
    """one launch: pop, lam (n, 32; zero from s on), ztail, sweeps (n), label (n, 32; -1 from s on), asym, cross (n), V (n, 32, 32)"""
    n = len(mats)
    sizes = np.array([A.shape[0] for A in mats], np.int32)
    smax = int(sizes.max())
    ld = smax * (smax + 1) // 2
    pk = np.zeros((n, ld))
    for t, A in enumerate(mats):
        p = EC.packed(A)
        pk[t, :len(p)] = p
    kT = np.ascontiguousarray(np.broadcast_to(np.asarray(kT, np.float64), (n,)))
    r = types.SimpleNamespace(pop=np.zeros((n, 32)), lam=np.zeros((n, 32)), ztail=np.zeros(n), sweeps=np.zeros(n, np.int32),
                              label=np.zeros((n, 32), np.int32), asym=np.zeros(n), cross=np.zeros(n),
                              V=np.zeros((n, 32, 32)) if want_v else None)
    err = ctypes.create_string_buffer(512)
    d, ci = ctypes.c_double, ctypes.c_int
    rc = lib().qdgb_thermal(n, H._p(sizes, ci), H._p(pk, d), ld, H._p(kT, d), int(blocks), int(poison), H._p(r.pop, d), H._p(r.lam, d),
                            H._p(r.ztail, d), H._p(r.sweeps, ci), H._p(r.label, ci), H._p(r.V, d) if want_v else None,
                            H._p(r.asym, d), H._p(r.cross, d), err, len(err))
    assert rc == 0, (rc, err.value.decode())
    return r


def check(A, kT, r, t, tag, sum_bar=True):
    """the checks of test_thermal_blocks_cpu.check on task t of the device result r, and what the workspace shows on the device"""
    s = A.shape[0]
    P, lam, z, sw = r.pop[t, :s], r.lam[t, :s], r.ztail[t], int(r.sweeps[t])
    assert np.isfinite(P).all() and np.isfinite(lam).all() and np.isfinite(z), tag
    assert not r.pop[t, s:].any() and not r.lam[t, s:].any() and np.all(r.label[t, s:] == -1), tag
    assert 0 <= sw < 24, (tag, sw)
    assert np.array_equal(r.label[t, :s], BC.bfs_labels(A)), (tag, r.label[t, :s])
    assert r.asym[t] == 0.0 and r.cross[t] == 0.0, (tag, r.asym[t], r.cross[t])
    Pr, wt, _ = TH.reference(A, kT)
    rp = float(np.abs(P - Pr).max() / TH.tol_occ(A, kT, 1.0))
    rz = float(abs(z - wt[-1]) / tol_ztail(A, kT))
    assert rp <= 1.0 and rz <= 1.0, (tag, s, kT, rp, rz)
    assert P.min() >= 0.0 and (not sum_bar or abs(P.sum() - 1.0) <= 64 * EPS), (tag, P.sum(), P.min())
    V = r.V[t, :s, :s]
    assert np.isfinite(V).all() and not r.V[t, s:].any() and not r.V[t, :, s:].any(), tag
    hn = EC.hnorm(A)
    resid = float(np.abs(A @ V - V * lam[None, :]).max() / hn) if hn else 0.0
    orth = float(np.abs(V.T @ V - np.eye(s)).max())
    assert resid <= 1e-12 and orth <= 1e-13, (tag, resid, orth)
    for k, v in (("pop", rp), ("ztail", rz), ("resid", resid), ("orth", orth), ("sweeps", sw)):
        _WORST[k] = max(_WORST[k], v)
    _WORST["n"] += 1


@functools.lru_cache(maxsize=None)
def family(s):
    """(tag, A, kT) of every task of size s: the blocks of test_thermal_blocks_cpu.test_families_of_every_size at their three
    temperatures"""
    fam = [(("hop", t), A) for t, A in EC.scale_family(s)]
    if s >= 2:
        for sep in (1e-5, 1e-7, 3e-9):
            fam += [(("near", sep, tc), A) for tc, A, _ in EC.near_degenerate_family(s, sep)]
    fam += [(("mixed", k), A) for k, A in enumerate(EC.mixed_scale_family(s))]
    fam += [(("extreme", k), A) for k, A in enumerate(EC.extreme_scale_family(s, reps=60))]
    fam.append(("classical", EC.classical_block(s)))
    return [(tag, A, kT) for tag, A in fam for kT in _temperatures(A)]


@functools.lru_cache(maxsize=None)
def family_solved(s):
    tasks = family(s)
    return dev([A for _, A, _ in tasks], [kT for _, _, kT in tasks])


@pytest.mark.parametrize("s", SIZES)
def test_families_of_every_size(s):
    tasks, r = family(s), family_solved(s)
    for t, (tag, A, kT) in enumerate(tasks):
        check(A, kT, r, t, tag)


@functools.lru_cache(maxsize=None)
def compositions():
    """the block-diagonal compositions of the CPU file: every partition, dealt round-robin and randomly permuted, four scales"""
    out = []
    for name, sizes in BC.PARTITIONS.items():
        rng = np.random.default_rng(sum(ord(c) for c in name))
        for tscale in (1e-8, 1e-3, 1.0, 30.0):
            for perm in (BC.interleave(sizes), rng.permutation(32)):
                A = BC.composition(rng, sizes, tscale, perm)
                out += [((name, tscale), A, kT) for kT in _temperatures(A)]
    return out


def test_block_diagonal_compositions_with_scattered_members():
    tasks = compositions()
    r = dev([A for _, A, _ in tasks], [kT for _, _, kT in tasks])
    for t, (tag, A, kT) in enumerate(tasks):
        check(A, kT, r, t, tag)
        if tag[0] == "32x1":
            assert r.sweeps[t] == 0 and np.array_equal(r.V[t], np.eye(32))


@pytest.mark.parametrize("s", SIZES)
def test_device_against_host_build(s):
    """the same source with the 64 lanes as a loop, IEEE division and sqrt and libm's exp: the same labels and sweep counts are not
    promised (a rotation at the threshold may fall either way), the populations within the sum of both tolerances"""
    tasks, r = family(s), family_solved(s)
    for t, (tag, A, kT) in enumerate(tasks):
        _, P, _, _, z, lab, _ = BC.solve(A, kT)
        assert np.array_equal(lab, r.label[t, :s]), tag
        dp = float(np.abs(P - r.pop[t, :s]).max() / (2 * TH.tol_occ(A, kT, 1.0)))
        dz = float(abs(z - r.ztail[t]) / (2 * tol_ztail(A, kT)))
        assert dp <= 1.0 and dz <= 1.0, (tag, s, kT, dp, dz)
        _WORST["dpop"] = max(_WORST["dpop"], dp); _WORST["dztail"] = max(_WORST["dztail"], dz)


# ---------------------------------------------------------------------------------------------------------------
# independence from neighbours, block count and stale LDS
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_list():
    """(mats, kT, what): neighbours that differ in size and partition -- one 32-state component then one state; ten components
    of 3 and one of 2 (21 pair slots) then one 32-state component (16 pair slots, other members, other items); an odd component
    (an idle partner) then a smaller even one; 16 pairs then 32 single states; a whole-block family of mixed sizes in between"""
    rng = np.random.default_rng(777)
    P = BC.PARTITIONS
    mats, what = [], []

    def add(A, name):
        mats.append(A); what.append(name)

    lane = {s: iter(list(EC.lane_mix_family(s, 40))) for s in (32, 31, 17, 7, 5, 4, 2)}
    for rnd in range(16):
        tscale = (1e-3, 1.0, 30.0, 1e-8)[rnd % 4]
        perm = rng.permutation(32) if rnd % 2 else BC.interleave(P["10x3+2"])
        add(next(lane[32]), "32"); add(np.array([[rng.uniform(-3, 3)]]), "1")
        add(BC.composition(rng, P["10x3+2"], tscale, perm), "10x3+2"); add(next(lane[32]), "32")
        add(next(lane[7]), "7"); add(next(lane[4]), "4")
        add(BC.composition(rng, [5, 3, 3, 2, 1], tscale, rng.permutation(14)), "5+3+3+2+1")
        add(BC.composition(rng, [4, 2], tscale, rng.permutation(6)), "4+2")
        add(BC.composition(rng, P["16x2"], tscale, rng.permutation(32)), "16x2"); add(EC.classical_block(32), "32x1")
        add(BC.composition(rng, P["17+15"], tscale, rng.permutation(32)), "17+15"); add(next(lane[17]), "17")
        add(next(lane[31]), "31"); add(next(lane[2]), "2")
        add(BC.composition(rng, P["1+2+..+7+4"], tscale, rng.permutation(32)), "1+2+..+7+4"); add(next(lane[5]), "5")
    kT = [_temperatures(A)[t % 3] if A.shape[0] > 1 else 0.1 for t, A in enumerate(mats)]
    return mats, kT, what


def test_mixed_list_has_the_neighbours_it_promises():
    mats, _, what = mixed_list()
    pairs = set(zip(what[:-1], what[1:]))
    assert len(mats) == 256 and {("32", "1"), ("10x3+2", "32"), ("7", "4"), ("5+3+3+2+1", "4+2"), ("16x2", "32x1"), ("31", "2")} <= pairs
    for A, name in zip(mats, what):
        if "+" in name or "x" in name:
            assert len(np.unique(BC.bfs_labels(A))) > 1, name


RUNS = [(blocks, poison) for blocks in (1, 7, 256) for poison in (0, 1, 2)]


@functools.lru_cache(maxsize=None)
def mixed_solved(blocks, poison):
    mats, kT, _ = mixed_list()
    return dev(mats, kT, blocks=blocks, poison=poison)


@pytest.mark.parametrize("blocks,poison", RUNS)
def test_core_does_not_depend_on_neighbours_blocks_or_stale_lds(blocks, poison):
    """one wave solving the whole list in order, seven blocks, one block per task, each with the workspace as found, poisoned once
    and poisoned before every task: the bits of (blocks = 256, poison = 2), where every task starts from a freshly poisoned
    workspace of its own"""
    mats, kT, what = mixed_list()
    base, got = mixed_solved(256, 2), mixed_solved(blocks, poison)
    for name in FIELDS:
        a = getattr(got, name)
        assert not np.isnan(a).any(), (blocks, poison, name, np.argwhere(np.isnan(a))[:8])
    for t, A in enumerate(mats):
        for name in FIELDS:
            a, b = getattr(got, name)[t], getattr(base, name)[t]
            same = np.array_equal(a, b) if name in ("sweeps", "label") else same_bits(a, b)
            assert same, (blocks, poison, t, what[t], what[t - 1] if t else None, name)
    if (blocks, poison) == (1, 0):                         # equal bits are not two wrong answers
        for t, A in enumerate(mats):
            check(A, kT[t], got, t, ("mixed list", t, what[t]), sum_bar=False)


def test_worst_figures_are_reported():
    print(f"[thermal blocks device] {_WORST['n']} tasks: worst err / tol populations {_WORST['pop']:.2e}, ztail {_WORST['ztail']:.2e}; "
          f"residual {_WORST['resid']:.2e} ||A||_inf, orthogonality {_WORST['orth']:.2e}, sweeps {_WORST['sweeps']}; |device - host| / "
          f"(tol + tol) populations {_WORST['dpop']:.2e}, ztail {_WORST['dztail']:.2e}")
    assert _WORST["pop"] <= 1.0 and _WORST["ztail"] <= 1.0
