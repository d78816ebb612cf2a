"""What the designed devices of the ground-state tests (tests/gs_cases.py) contain, from the oracle alone.  No GPU needed.

tests/test_gpu_gs_designed.py runs the same members through the device code and takes its coverage bounds from the counts
asserted here, so a change of the sampler or of the recipe cannot quietly empty it: the block sizes that occur and that win
the selection, the full batch of 32-state blocks, the exactly-zero and the denormal couplings, and the share of pixels the
1e-6 rule excludes (relative gap <= helpers.GAP_MIN) -- at most 5 % per member; a member beyond that is changed, not the cap.
The members also go through the host build of the candidate search and through the pruning bound's CPU check
(test_gs_prune_cpu.check_pixels), which the sampler's scenes never gave a 32-state component."""
import numpy as np
import pytest

import gs_cases as GS
import helpers as H
from test_gs_prune_cpu import check_pixels

CAP = 0.05

# components / winners per block size over all channels, K = 32 (sizes that do not occur are left out)
CENSUS = {
    ("one_sector", 5, 16): (
        {32: 1024},
        {32: 1024}),
    ("one_sector", 5, 17): (
        {32: 1156},
        {32: 1156}),
    ("all_sizes", 5, 16): (
        {1: 445, 2: 75, 3: 13, 4: 82, 5: 31, 6: 49, 7: 23, 8: 54, 9: 54, 10: 60, 11: 62, 12: 59, 13: 67, 14: 89, 15: 72, 16: 60,
         17: 72, 18: 89, 19: 67, 20: 59, 21: 62, 22: 61, 23: 58, 24: 62, 25: 50, 26: 37, 27: 72, 28: 42, 29: 60, 30: 71, 31: 40,
         32: 92},
        {12: 1, 13: 15, 14: 30, 15: 26, 16: 30, 17: 46, 18: 59, 19: 52, 20: 58, 21: 62, 22: 61, 23: 58, 24: 62, 25: 50, 26: 37,
         27: 72, 28: 42, 29: 60, 30: 71, 31: 40, 32: 92}),
    ("cut_pair", 5, 16): (
        {1: 379, 2: 98, 3: 337, 4: 290, 5: 125, 6: 289, 7: 277, 8: 332, 9: 516, 10: 329, 11: 202, 12: 268, 13: 631, 14: 97,
         15: 9},
        {9: 52, 10: 100, 11: 54, 12: 201, 13: 511, 14: 97, 15: 9}),
    ("denormal_pair", 5, 16): (
        {32: 1024},
        {32: 1024}),
    ("cut_two", 5, 16): (
        {1: 1888, 2: 2163, 3: 1412, 4: 2316, 5: 1054, 6: 1071, 7: 194},
        {3: 8, 5: 88, 6: 750, 7: 178}),
    ("all_sizes", 8, 16): (
        {1: 5408, 2: 789, 3: 305, 4: 144, 5: 93, 6: 77, 7: 56, 8: 25, 9: 44, 10: 18, 11: 18, 12: 27, 13: 38, 14: 12, 15: 9,
         16: 41, 17: 32, 18: 23, 19: 21, 20: 21, 21: 44, 22: 37, 23: 52, 24: 44, 25: 60, 26: 89, 27: 98, 28: 227, 29: 485, 30: 278,
         31: 95, 32: 27},
        {3: 1, 4: 1, 5: 11, 6: 13, 7: 12, 8: 19, 9: 16, 10: 2, 11: 8, 12: 12, 13: 20, 14: 10, 15: 7, 16: 34, 17: 27, 18: 21,
         19: 21, 20: 21, 21: 44, 22: 37, 23: 52, 24: 44, 25: 60, 26: 89, 27: 98, 28: 227, 29: 485, 30: 278, 31: 95, 32: 27}),
}
# ("one_sector", 5, 16) with K kept states, channels GS.KEPT_CHANNELS
CENSUS_KEPT = {
    2: ({1: 952, 2: 36}, {1: 476, 2: 36}),
    3: ({1: 981, 2: 192, 3: 57}, {1: 263, 2: 192, 3: 57}),
    8: ({1: 112, 2: 60, 3: 9, 5: 9, 6: 60, 7: 112, 8: 331}, {5: 9, 6: 60, 7: 112, 8: 331}),
    9: ({1: 62, 2: 26, 3: 5, 6: 5, 7: 26, 8: 62, 9: 419}, {6: 5, 7: 26, 8: 62, 9: 419}),
    10: ({1: 6, 2: 6, 8: 6, 9: 6, 10: 500}, {8: 6, 9: 6, 10: 500}),
    11: ({1: 2, 10: 2, 11: 510}, {10: 2, 11: 510}),
    12: ({1: 2, 11: 2, 12: 510}, {11: 2, 12: 510}),
    13: ({1: 3, 12: 3, 13: 509}, {12: 3, 13: 509}),
    16: ({16: 512}, {16: 512}),
    17: ({17: 512}, {17: 512}),
    31: ({31: 512}, {31: 512}),
    32: ({32: 512}, {32: 512}),
}


def _as_dict(counts):
    return {s: int(c) for s, c in enumerate(counts) if c}


@pytest.mark.parametrize("name,N,R", GS.MEMBERS)
def test_census_of_the_members(name, N, R):
    comp, win = GS.size_counts(name, N, R)
    print(f"[gs census] {name} N={N} R={R}: components {_as_dict(comp)}\n    winners {_as_dict(win)}")
    assert (_as_dict(comp), _as_dict(win)) == CENSUS[(name, N, R)]
    assert win.sum() == (N - 1) * R * R


@pytest.mark.parametrize("K", GS.KEPT)
def test_census_of_the_kept_set_sizes(K):
    """one_sector with K kept states: a block of all K states in most pixels; up to K = 13 a few pixels keep a state whose hop
    partners all lie beyond the K-th, which leaves a block of K - 1 (from 16 states on every prefix of the list is one block).
    The GPU tier's reference for K < 32 is the Python oracle's k = K scan: it must name the first K states of the C oracle's
    list (no energies so close that NumPy's einsum and the canonical arithmetic order them differently)."""
    import qd_oracle as O
    N, R = 5, 16
    comp, win = GS.size_counts("one_sector", N, R, K, chs=GS.KEPT_CHANNELS)
    print(f"[gs census] one_sector N=5 R=16 K={K}: components {_as_dict(comp)}, winners {_as_dict(win)}")
    assert (_as_dict(comp), _as_dict(win)) == CENSUS_KEPT[K]
    assert comp[K] > 0 and win[K] > 0
    if K <= 13:
        assert comp[K - 1] > 0
    par, st = GS.make("one_sector", N, R)
    dev = H.dev_view(N, par); sv = H.state_view(N, st)
    for ch in GS.KEPT_CHANNELS:
        vg = O.sweep_voltages(sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, ch, -dev.window, dev.window, R)
        v_ext = np.concatenate([vg, np.broadcast_to(sv.barrier_v, (R * R, N - 1))], axis=1)
        assert np.array_equal(O.candidate_states(v_ext, dev.cdd_inv_full, dev.cgd_full, N, k=K)[0], GS.census("one_sector", N, R, ch, K)["states"])


def test_every_size_occurs_and_every_class_wins():
    """over the members and the kept-set sizes together (the recorded tables, which the two tests above tie to the oracle)"""
    comp = np.zeros(33, np.int64); win = np.zeros(33, np.int64)
    for c, w in list(CENSUS.values()) + list(CENSUS_KEPT.values()):
        for s, n in c.items():
            comp[s] += n
        for s, n in w.items():
            win[s] += n
    assert (comp[2:] > 0).all(), _as_dict(comp)
    for lo, hi in GS.CLASSES:
        assert win[lo:hi + 1].sum() > 0, (lo, hi)
    # the memory class more finely: every size 13..32 wins in some pixel
    assert (win[13:] > 0).all(), _as_dict(win)
    # with all 32 states kept, without the kept-set members: every size 2..32 occurs, every class from 3 states on wins
    comp32 = sum(np.bincount(list(c), weights=list(c.values()), minlength=33) for c, _ in CENSUS.values())
    assert (comp32[2:] > 0).all()


def test_one_sector_fills_a_batch():
    """QD_GS_PPB = 256 pixels per batch, each with one component of all 32 states: the pool's worst case, met exactly.  At
    17 x 17 the first batch of channel 0 is such a batch and the second one ends in an odd pixel."""
    assert GS.PPB == 256
    c = GS.census("one_sector", 5, 16, 0)
    assert len(c["sizes"]) == GS.PPB and all(s.tolist() == [32] for s in c["sizes"])
    c = GS.census("one_sector", 5, 17, 0)
    assert len(c["sizes"]) == 289 and all(s.tolist() == [32] for s in c["sizes"][:GS.PPB])
    assert all(s.tolist() == [32] for s in c["sizes"][GS.PPB:])          # (and the 33 pixels of the second batch)


@pytest.mark.parametrize("name", ["cut_pair", "cut_two", "denormal_pair"])
def test_couplings_are_zero_or_denormal_where_designed(name):
    N, R = 5, 16
    tiny = np.ldexp(1.0, -1022)
    for ch in GS.channels(N):
        tc = GS.census(name, N, R, ch)["tc"]
        special = GS.CUT.get(name, (1,))
        for d in range(N - 1):
            if d not in special:
                assert (tc[:, d] >= tiny).all() and np.isfinite(tc[:, d]).all(), (ch, d)
            elif name == "denormal_pair":
                assert ((tc[:, d] > 0.0) & (tc[:, d] < tiny)).all(), (ch, d, tc[:, d].min(), tc[:, d].max())
                assert (tc[:, d] > 1e-318).all() and (tc[:, d] < 1e-314).all()       # well inside the denormals
            else:
                assert (tc[:, d] == 0.0).all(), (ch, d, tc[:, d].max())


def test_cut_and_denormal_have_the_same_physics():
    """the same kept states, and ground vectors that agree far below the 1e-6 of the device tests wherever both resolve"""
    N, R = 5, 16
    for ch in GS.channels(N):
        a = GS.census("cut_pair", N, R, ch); b = GS.census("denormal_pair", N, R, ch)
        assert np.array_equal(a["states"], b["states"])
        ok = (a["rel_gap"] > H.GAP_MIN) & (b["rel_gap"] > H.GAP_MIN)
        assert ok.all()
        assert np.abs(a["ref"]["occ"] - b["ref"]["occ"])[ok].max() <= 1e-9


def test_exclusion_cap():
    for name, N, R in GS.MEMBERS:
        gaps = [GS.census(name, N, R, ch)["rel_gap"] for ch in GS.channels(N)]
        bad = sum(int((g <= H.GAP_MIN).sum()) for g in gaps); tot = sum(g.size for g in gaps)
        print(f"[gs cases] {name} N={N} R={R}: {bad} of {tot} pixels excluded (relative gap <= {H.GAP_MIN}): {bad / tot:.2%}")
        assert bad <= CAP * tot, (name, N, R, bad, tot)
        if name == "one_sector":
            assert not (gaps[0] <= H.GAP_MIN).any()
    for K in GS.KEPT:
        gaps = [GS.census("one_sector", 5, 16, ch, K)["rel_gap"] for ch in GS.KEPT_CHANNELS]
        bad = sum(int((g <= H.GAP_MIN).sum()) for g in gaps); tot = sum(g.size for g in gaps)
        print(f"[gs cases] one_sector N=5 R=16 K={K}: {bad} of {tot} pixels excluded: {bad / tot:.2%}")
        assert bad <= CAP * tot, (K, bad, tot)


@pytest.mark.parametrize("name,N,R", GS.MEMBERS)
def test_host_search_equals_the_c_oracle(name, N, R):
    par, st = GS.make(name, N, R)
    for ch in GS.channels(N):
        hf = H.host_front(N, par, st, ch, R)
        assert np.array_equal(hf["states"], GS.census(name, N, R, ch)["ref"]["states"]), ch
        assert (hf["nvalid"] == 32).all()


@pytest.mark.parametrize("name,N,R", [m for m in GS.MEMBERS if m[2] == 16])
def test_prune_bound_on_the_members(name, N, R):
    """the pruning bound's three assertions on Hamiltonians with components of up to 32 states; channels 0 and N - 2"""
    for ch in sorted({0, N - 2}):
        c = GS.census(name, N, R, ch)
        check_pixels((name, N, ch), c["F"], c["Ht"])


def test_solver_stats_counts_every_size_class():
    """solver_stats() on a stand-in for the library: the device keeps one task counter per size class (2 .. 8 states, 9-10,
    11-12, 13-32, then the wide blocks of the full space); "9+" is the three classes from 9 states on together.  It used to
    report the class of 9-10 states alone, so a scene of 32-state blocks showed no task of 9 or more states."""
    import types
    from qadapt_hip.vec_env import VecQuantumDeviceEnv

    class Lib:
        def qd_get_solver_stats(self, h, out):
            for i, v in enumerate([130, 260, 5, 40, 2, 3, 4, 5, 6, 7, 8, 10, 20, 60, 5, 0]):
                out[i] = v
            return 0

    s = VecQuantumDeviceEnv.solver_stats(types.SimpleNamespace(_h=None, _lib=Lib()))
    assert s["tasks_by_size"] == {"2": 2, "3": 3, "4": 4, "5": 5, "6": 6, "7": 7, "8": 8, "9+": 90}
    assert list(s["tasks_by_size"]) == GS.SIZE_KEYS
    assert s["wide_tasks"] == 5 and s["tasks"] == sum(s["tasks_by_size"].values()) + s["wide_tasks"]
