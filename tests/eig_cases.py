"""The matrices of the eigen-solver tests, one source for both tiers: tests/test_eig_solver_cpu.py and
tests/test_eig_wave_cpu.py run them through the host builds of csrc/qd_eig.h / csrc/qd_eig_wave.h,
tests/test_gpu_eig_device.py through the device code.  Every family is a generator with its own seeded rng that draws
in a fixed order, so a family is the same list of matrices wherever it is iterated.  Matrices are dense symmetric
float64 arrays; the solvers take the packed lower triangle (`packed`)."""
import numpy as np

import helpers as H

# ---------------------------------------------------------------------------------------------------------------
# per-lane solvers (2..32 states)
# ---------------------------------------------------------------------------------------------------------------
LANE_SIZES = list(range(2, 33))
CLASSICAL_SIZES = [2, 3, 4, 6, 8, 9, 12, 22]
NEAR_DEGENERATE = [(4, 1e-5), (4, 1e-7), (6, 1e-6), (8, 1e-8), (8, 3e-9), (12, 1e-6), (20, 1e-7)]
MIXED_SIZES = [3, 4, 5, 6, 7, 8, 10, 16, 32]
EXTREME_SIZES = [3, 5, 8, 9, 12, 20]


def packed(A):
    return np.ascontiguousarray(A[np.tril_indices(A.shape[0])], dtype=np.float64)


def hnorm(A):
    return np.abs(A).sum(axis=1).max()


def hop_block(rng, s, tscale, extra_edges=0.3):
    """connected block: random spanning tree + a few more edges, couplings -t*sqrt(k), diagonal O(1) >= 0"""
    A = np.zeros((s, s))
    for i in range(1, s):
        j = rng.integers(0, i)
        A[i, j] = A[j, i] = -tscale * rng.uniform(0.3, 3.0) * np.sqrt(rng.integers(1, 7))
    for _ in range(int(extra_edges * s)):
        i, j = rng.integers(0, s, 2)
        if i != j:
            A[i, j] = A[j, i] = -tscale * rng.uniform(0.3, 3.0) * np.sqrt(rng.integers(1, 7))
    A[np.diag_indices(s)] = rng.uniform(0, 4.0, s)
    A[rng.integers(0, s), rng.integers(0, s)] += 0.0
    return A


def coupling_scales(s):
    return (0.0 if s == 2 else 1e-22, 1e-8, 1e-3, 1.0, 30.0, 1e6, 1e14, 1e30, 1e44)


def scale_family(s):
    """(tscale, A): hop blocks of s states over nine coupling scales, 6 per scale"""
    rng = np.random.default_rng(100 + s)
    for tscale in coupling_scales(s):
        for rep in range(6):
            yield tscale, hop_block(rng, s, tscale)


def classical_block(s):
    """couplings of exactly zero: the lowest diagonal entry wins"""
    rng = np.random.default_rng(s)
    A = np.diag(rng.uniform(0, 3, s)); A[3 % s, 3 % s] = 0.0
    return A


def near_degenerate_block(rng, s, sep, tc):
    """(A, hn): two identical hop blocks of s // 2 states at coupling scale tc, linked by -sep * hn; hn is ||A||_inf
    before the link and the O(1) diagonal go in (the scale the bars are stated in)"""
    h = s // 2
    B = hop_block(rng, h, tc)
    A = np.zeros((s, s)); A[:h, :h] = B; A[h:2 * h, h:2 * h] = B
    if s > 2 * h:
        A[s - 1, s - 1] = 5.0 * tc; A[s - 1, 0] = A[0, s - 1] = -tc
    hn = np.abs(A).sum(axis=1).max()
    A[0, h] = A[h, 0] = -sep * hn                      # weak link between the halves
    A[np.diag_indices(s)] += rng.uniform(0, 1.0, s)    # O(1) free-energy differences
    return A, hn


def near_degenerate_family(s, sep):
    """(tc, A, hn): two weakly linked identical halves at tc ~ 1e14..1e20, lowest pair split by `sep` relative"""
    rng = np.random.default_rng(int(-np.log10(sep)) * 100 + s)
    for tc in (1e14, 1e20):
        A, hn = near_degenerate_block(rng, s, sep, tc)
        yield tc, A, hn


def lane_mix_family(s, n=64):
    """n blocks of s states whose Laguerre iteration counts differ, neighbours in the list of different kinds: hop blocks
    at coupling scales 1e-22, 1 and 1e44, and a near-degenerate pair (relative split 1e-7 at tc = 1e14)"""
    rng = np.random.default_rng(64000 + s)
    for i in range(n):
        if i % 4 == 3:
            yield near_degenerate_block(rng, s, 1e-7, 1e14)[0]
        else:
            yield hop_block(rng, s, (1e-22, 1.0, 1e44)[i % 4])


def iteration_count_family():
    rng = np.random.default_rng(5)
    for s in (3, 4, 5, 8):
        for tscale in (1e-3, 1.0, 1e9, 1e20):
            for _ in range(50):
                yield hop_block(rng, s, tscale)


def small_entry_block():
    """A pixel of the 6-dot `mid` scene: well separated ground state whose vector has an entry of 3e-7."""
    A = np.zeros((5, 5))
    A[np.diag_indices(5)] = [1.8211606185966067e-03, 9.0892916727111694e-02, 1.1252147134350532e-01,
                             1.9574221943041425e-01, 2.2405314073563976e-01]
    for i, j, v in ((0, 1, -6.2326547064007944e-03), (0, 4, -1.1348431758338040e+00), (1, 3, -8.7785459752451171e-05),
                    (2, 4, -5.1873123805475409e-03)):
        A[i, j] = A[j, i] = v
    return A


def mixed_scale_family(s):
    """couplings of one block spread over many decades (tc_i = tc_base exp(-alpha_i vb_i) differs per barrier), 40 blocks"""
    rng = np.random.default_rng(7 * s)
    for rep in range(40):
        A = np.zeros((s, s))
        for i in range(1, s):
            j = rng.integers(0, i)
            A[i, j] = A[j, i] = -10.0 ** rng.uniform(-9, 2)
        A[np.diag_indices(s)] = rng.uniform(0, 1.0, s)
        yield A


def column_tail_block():
    """A 10-state block of the random-action sweep (seed 1234, env 8, tc up to 2e45 next to couplings of 7e-5): after
    scaling, a Householder column has x0 ~ 1e-66 and a tail of ~1e-160."""
    rows = [[0.0], [-6.974298567106001e-05, 0.020594523099134676], [0.0, 0.0, 0.17739829741913127], [0.0, -0.025654117816680404, 0.0, 0.20331981604977045], [0.0, -1.9997155568046502e+45, 0.0, 0.0, 0.20989064725290518], [-5.121032850084054, 0.0, -1.9997155568046502e+45, 0.0, 0.0, 0.3314526208159805], [0.0, -5.121032850084054, 0.0, 0.0, 0.0, -6.974298567106001e-05, 0.3591142439254327], [0.0, 0.0, 0.0, -1.9997155568046502e+45, -0.025654117816680404, 0.0, 0.0, 0.3912569026942947], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -6.974298567106001e-05, 0.44611644657561556], [0.0, 0.0, -2971.837515200498, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.4715202777515515]]
    s = len(rows)
    A = np.zeros((s, s))
    for i, r in enumerate(rows):
        A[i, :i + 1] = r; A[:i + 1, i] = r
    return A


def extreme_scale_family(s, reps=200):
    """couplings from 1e-30 to 1e45 inside one block, diagonal up to 1e4"""
    rng = np.random.default_rng(900 + s)
    for rep in range(reps):
        A = np.zeros((s, s))
        for i in range(1, s):
            j = rng.integers(0, i)
            A[i, j] = A[j, i] = -10.0 ** rng.uniform(-30, 45) * (rng.random() < 0.9)
        for _ in range(s // 2):
            i, j = rng.integers(0, s, 2)
            if i != j: A[i, j] = A[j, i] = -10.0 ** rng.uniform(-30, 45)
        A[np.diag_indices(s)] = rng.uniform(0, 1.0, s) * 10.0 ** rng.integers(0, 5)
        yield A


# ---------------------------------------------------------------------------------------------------------------
# wave-per-block solver (33..64 states, and the small sizes it accepts)
# ---------------------------------------------------------------------------------------------------------------
WIDE_SIZES = list(range(33, 65))
WIDE_HOP_SIZES = [33, 44, 51, 64]
WIDE_SMALL_SIZES = (2, 3, 4, 7, 13, 32)
WIDE_SCALES = (1e-22, 1e-6, 1.0, 1e9, 1e44)
WIDE_HOP_SCALES = (1e-22, 1e-8, 1e-3, 1.0, 30.0, 1e6, 1e14, 1e30, 1e44)


def wide_random_family(s):
    """((s, scale, rep), A): random symmetric blocks over five scales, 3 per scale"""
    rng = np.random.default_rng(1000 + s)
    for scale in WIDE_SCALES:
        for rep in range(3):
            A = rng.normal(size=(s, s)) * scale
            yield (s, scale, rep), A + A.T


def wide_hop_family(s):
    """((s, tscale, rep), A): non-negative diagonal of O(1), non-positive couplings on a connected sparse graph"""
    rng = np.random.default_rng(7 + s)
    for tscale in WIDE_HOP_SCALES:
        for rep in range(3):
            yield (s, tscale, rep), hop_block(rng, s, tscale)


def wide_small_family():
    rng = np.random.default_rng(3)
    for s in WIDE_SMALL_SIZES:
        A = rng.normal(size=(s, s))
        yield s, A + A.T


def wide_degenerate_family():
    """two weakly coupled copies of the same block: the two lowest levels split by ~1e-11 ||A||, by ~1e-6 ||A||, not at all"""
    rng = np.random.default_rng(11)
    B = rng.normal(size=(24, 24)); B = B + B.T
    for eps in (1e-11, 1e-6, 0.0):
        A = np.zeros((48, 48))
        A[:24, :24] = B; A[24:, 24:] = B
        A[0, 24] = A[24, 0] = eps
        yield ("degenerate", eps), A


def wide_underflow_family():
    """couplings 60 decades apart inside one block: the reflector of a column whose tail is ~1e-160 of its head would
    need v0^2 ~ 1e-320 (the NaN case of the per-lane solver at tc ~ 2e45); and the same block scaled down"""
    rng = np.random.default_rng(12)
    s = 40
    A = np.diag(rng.uniform(0, 4, s))
    for i in range(1, s):
        A[i, i - 1] = A[i - 1, i] = -2e45 * rng.uniform(0.5, 2.0)
    for i in range(2, s):
        A[i, 0] = A[0, i] = -1e-115 * rng.uniform(0.5, 2.0)          # scaled: ~1e-160 next to x0 ~ 1
    A[5, 3] = A[3, 5] = -1e-15
    yield "underflow", A
    A2 = A / 2e45
    A2[np.diag_indices(s)] = rng.uniform(0, 4, s)
    yield "underflow, scaled", A2


def wide_sector_family(N, m, stride=1):
    """((N, m, e, ch, p, size), block, tcmax so far): every stride-th sector of more than 32 states out of the scenes of
    tests/wide_scenes.py (near / far / random actions: tunnel couplings up to ~1e45 occur) -- the blocks as the
    structure kernel hands them over, diagonal relative to the pixel's lowest free energy."""
    from test_full_charge_space import full_states, full_hamiltonian, pixel_inputs
    import wide_scenes as WS
    states = full_states(N, m)
    Q = states.sum(axis=1)
    wide = [np.flatnonzero(Q == q) for q in np.unique(Q) if (Q == q).sum() > 32]
    assert wide
    params, st = WS.scene(N, m)
    tcmax, k = 0.0, 0
    for e in range(len(params)):
        dev = H.dev_view(N, params[e]); sv = H.state_view(N, st[e])
        for ch in range(N - 1):
            F, tc, _, _ = pixel_inputs(dev, sv, ch, 4, states, vc=dev.vc)
            F = F - F.min(axis=1, keepdims=True)
            Hm = full_hamiltonian(F, tc, states)
            tcmax = max(tcmax, float(np.abs(tc).max()))
            for p in range(len(F)):
                for sel in wide:
                    if k % stride == 0:
                        yield (N, m, e, ch, p, len(sel)), Hm[p][np.ix_(sel, sel)], tcmax
                    k += 1
