"""The two one-point-per-wavefront eigen-solvers of the point queries ON THE DEVICE (run with -m gpu): the levels core
qd_levels_solve (csrc/qd_levels.h: Householder, Sturm-count multisection) and the thermal core qd_thermal_solve
(csrc/qd_thermal.h: round-robin cyclic Jacobi on a 32 x 33 block in LDS), called by the harness kernels of tests/gputest_eig
behind qd_levels_load_packed, in persistent single-wave blocks shaped like qd_k_levels / qd_k_thermal.  The matrices are those
tests/test_levels_cpu.py and tests/test_thermal_cpu.py run through the host builds (tests/eig_cases.py), the references
numpy.linalg.eigvalsh / eigh in float64 and thermal_helpers.reference, the bars those of the two CPU files, imported.

  1. every family at every size 1..32, both cores: every task is compared, none is exempt; the thermal block stays exactly
     symmetric (asym == 0) and ends with nothing above 2^-56 off the diagonal
  2. every section width of the multisection: L = 1..8 at s = 2, 3, 5, 8, 17, 32 (P = 64, 32, 21, 16, 12, 10, 9, 8 lanes per level)
  3. what the design states bit for bit: exact multiplicities come back bitwise equal; exactly zero couplings never rotate
     (no sweep, V = I, lam = diag(A), equal populations of a degenerate pair)
  4. what no other tier can run: a task's result does not depend on its neighbours in a persistent block, on the number of
     blocks, or on what the __shared__ workspace held before (left as found, poisoned with NaN before a block's first task,
     poisoned before every task): the same bits in all nine runs, and no NaN
  5. a measurement, not an assertion: device against host build of the same source (rcp / rsq + Newton and ocml's exp against
     IEEE division, sqrt and libm's exp), beside each build's distance from the reference

Every family is solved once per size (one launch for the levels; two for the thermal core, the one that asks for V and the one
that does not) and the results are shared by the tests.  s = 1 has no near-degenerate family (it needs two halves).

Measured on an MI355X (also in DESIGN 7):
  levels   worst |level - eigvalsh| / ||A||_inf over 5 148 tasks: device 2.15e-15, host build 2.15e-15 (bar 1e-12);
           |device - host build| = 0 on every level of every task: qd_rcp and qd_sqrt1 round correctly on the arguments the
           Householder step hands them (tests/test_gpu_eig_device.py measures 1.11e-16 for both), the Sturm recurrence divides
           in IEEE on both sides, so the two builds see the same T
  thermal  over 15 444 tasks: worst population err / tol device 4.36e-4, host build 5.23e-4; ztail err / tol device 2.45e-4,
           host build 2.45e-4; worst |P_device - P_host| / tol 3.68e-4, ztail 1.24e-4 (qd_sqrt_rsqrt's 1 / sqrt is 2.2e-16 where
           the host divides, and ocml's exp is not libm's); residual 1.61e-15 ||A||_inf, orthogonality 1.02e-14; most sweeps 10
           of the 24 allowed (host build 10); asym 0 on every task; off-diagonal left 2^-56 = 1.39e-17 at the most (the bar)
Sensitivity, checked once on a scratch build of the harness: without the line of qd_thermal_solve that zeroes row and column s of
an odd s, all nine thermal runs of 4 fail (seven on "no output is NaN" at asym, the two one-wave runs without a poison before
every task on the bits of pop) and the nine levels runs pass."""
import ctypes
import functools
import types

import numpy as np
import pytest

import eig_cases as EC
import helpers as H
import thermal_helpers as TH
import test_gpu_eig_device as GE
import test_levels_cpu as LC
import test_thermal_cpu as TC

pytestmark = pytest.mark.gpu

SIZES = [1] + EC.LANE_SIZES
EPS = TC.EPS
OFF_BAR = 2.0 ** -56                                    # QD_TH_THRESH: what a converged sweep leaves off the diagonal
same_bits = GE.same_bits


def lib():
    L = GE.lib()
    if not getattr(L, "_qdg_spectrum", False):
        dp, ip, ci = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.c_int
        L.qdg_levels.argtypes = [ci, ip, dp, ci, ci, ci, ci, dp, ctypes.c_char_p, ci]
        L.qdg_thermal.argtypes = [ci, ip, dp, ci, dp, ci, ci, dp, dp, dp, ip, dp, dp, dp, ctypes.c_char_p, ci]
        L.qdg_levels.restype = L.qdg_thermal.restype = ci
        L._qdg_spectrum = True
    return L


def _pack(mats):
    n = len(mats)
    sizes = np.array([A.shape[0] for A in mats], np.int32)
    smax = int(sizes.max())
    ld = smax * (smax + 1) // 2
    pk = np.zeros((n, ld))
    for t, A in enumerate(mats):
        p = EC.packed(A)
        pk[t, :len(p)] = p
    return n, sizes, pk, ld


def dev_levels(mats, L, blocks=0, poison=0):
    """one launch: lev (n, 8), +inf from min(L, s) on"""
    n, sizes, pk, ld = _pack(mats)
    lev = np.zeros((n, 8))
    err = ctypes.create_string_buffer(512)
    rc = lib().qdg_levels(n, H._p(sizes, ctypes.c_int), H._p(pk, ctypes.c_double), ld, int(L), int(blocks), int(poison),
                          H._p(lev, ctypes.c_double), err, len(err))
    assert rc == 0, (rc, err.value.decode())
    return lev


THERMAL_FIELDS = ("pop", "lam", "ztail", "sweeps", "asym", "off", "V")


def dev_thermal(mats, kT, blocks=0, poison=0, want_v=False):
    """one launch: pop, lam (n, 32; zero from s on), ztail, sweeps, asym, off (n), V (n, 32, 32) or None"""
    n, sizes, pk, ld = _pack(mats)
    kT = np.ascontiguousarray(np.broadcast_to(np.asarray(kT, np.float64), (n,)))
    r = types.SimpleNamespace(pop=np.zeros((n, 32)), lam=np.zeros((n, 32)), ztail=np.zeros(n), sweeps=np.zeros(n, np.int32),
                              asym=np.zeros(n), off=np.zeros(n), V=np.zeros((n, 32, 32)) if want_v else None)
    err = ctypes.create_string_buffer(512)
    d = ctypes.c_double
    rc = lib().qdg_thermal(n, H._p(sizes, ctypes.c_int), H._p(pk, d), ld, H._p(kT, d), int(blocks), int(poison), H._p(r.pop, d),
                           H._p(r.lam, d), H._p(r.ztail, d), H._p(r.sweeps, ctypes.c_int), H._p(r.V, d) if want_v else None,
                           H._p(r.asym, d), H._p(r.off, d), err, len(err))
    assert rc == 0, (rc, err.value.decode())
    return r


# ---------------------------------------------------------------------------------------------------------------
# the families of the two CPU files, per size: matrices, float64 reference (once), device results (once)
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def family(s):
    """the blocks test_families_of_every_size of both CPU files iterate, in their order, and the two regression matrices at
    their sizes (column tail: 10, small entries: 5)"""
    fam = [(("hop", t), A) for t, A in EC.scale_family(s)]
    if s >= 2:
        for sep in (1e-5, 1e-7, 3e-9):
            fam += [(("near", sep, tc), A) for tc, A, _ in EC.near_degenerate_family(s, sep)]
    fam += [(("mixed", k), A) for k, A in enumerate(EC.mixed_scale_family(s))]
    fam += [(("extreme", k), A) for k, A in enumerate(EC.extreme_scale_family(s, reps=60))]
    fam.append(("classical", EC.classical_block(s)))
    if s == 10:
        fam.append(("column tail", EC.column_tail_block()))
    if s == 5:
        fam.append(("small entries", EC.small_entry_block()))
    out = []
    for tag, A in fam:
        assert A.shape == (s, s)
        out.append(types.SimpleNamespace(tag=tag, A=A, s=s, hn=EC.hnorm(A), w=np.linalg.eigvalsh(A), kT=TC._temperatures(A)))
    return out


V_AT = 1                                                # the temperature of a block's three at which V is requested


@functools.lru_cache(maxsize=None)
def levels_solved(s):
    return dev_levels([c.A for c in family(s)], min(8, s))


@functools.lru_cache(maxsize=None)
def thermal_solved(s):
    """(with V: one task per block at kT[V_AT];  without: two tasks per block, the other two temperatures, block-major)"""
    cs = family(s)
    rest = [k for k in range(3) if k != V_AT]
    with_v = dev_thermal([c.A for c in cs], [c.kT[V_AT] for c in cs], want_v=True)
    without = dev_thermal([c.A for c in cs for _ in rest], [c.kT[k] for c in cs for k in rest])
    return with_v, without, rest


def thermal_tasks(s):
    """every thermal task of size s: (case, kT, result, index in the result)"""
    cs = family(s)
    with_v, without, rest = thermal_solved(s)
    for i, c in enumerate(cs):
        yield c, c.kT[V_AT], with_v, i
        for j, k in enumerate(rest):
            yield c, c.kT[k], without, len(rest) * i + j


def level_err(c, lev, L=None):
    """the checks of test_levels_cpu.check on one device result; returns |level - eigvalsh| / ||A||_inf"""
    n = min(8 if L is None else L, c.s)
    assert np.isfinite(lev[:n]).all() and np.all(np.isposinf(lev[n:])), (c.tag, c.s, lev)
    assert np.all(np.diff(lev[:n]) >= 0), (c.tag, c.s, lev)
    err = np.abs(lev[:n] - c.w[:n]).max()
    assert err <= LC.BAR * c.hn, (c.tag, c.s, err / c.hn if c.hn else err)
    return err / c.hn if c.hn else 0.0


def thermal_err(c, kT, r, t, cap, sum_bar=True):
    """the checks of test_thermal_cpu.check on task t of the device result r, and the two the workspace allows on the device;
    returns the figures.  sum_bar: the CPU file's |sum P - 1| <= 64 eps, a bar it states for its own families"""
    s, A = c.s, c.A
    P, lam, z, sw = r.pop[t, :s], r.lam[t, :s], r.ztail[t], int(r.sweeps[t])
    tag = (c.tag, s, kT)
    assert np.isfinite(P).all() and np.isfinite(lam).all() and np.isfinite(z), tag
    assert not r.pop[t, s:].any() and not r.lam[t, s:].any(), tag
    assert 0 <= sw < cap, (tag, sw)
    Pr, wt, _ = TH.reference(A, kT)
    rp = float(np.abs(P - Pr).max() / TH.tol_occ(A, kT, 1.0))
    rz = float(abs(z - wt[-1]) / TC.tol_ztail(A, kT))
    assert rp <= 1.0 and rz <= 1.0, (tag, rp, rz)
    assert P.min() >= 0.0 and (not sum_bar or abs(P.sum() - 1.0) <= 64 * EPS), (tag, P.sum(), P.min())
    assert r.asym[t] == 0.0, (tag, r.asym[t])                                  # exactly symmetric (step 2b)
    assert r.off[t] <= OFF_BAR, (tag, r.off[t])                                # (sw < cap: the last sweep rotated nothing)
    resid = orth = 0.0
    if r.V is not None:
        V = r.V[t, :s, :s]
        assert np.isfinite(V).all() and not r.V[t, s:].any() and not r.V[t, :, s:].any(), tag
        resid = float(np.abs(A @ V - V * lam[None, :]).max() / c.hn) if c.hn else 0.0
        orth = float(np.abs(V.T @ V - np.eye(s)).max())
        assert resid <= 1e-12 and orth <= 1e-13, (tag, resid, orth)
    return dict(pop=rp, ztail=rz, resid=resid, orth=orth, sweeps=sw, off=float(r.off[t]))


_WORST = {"levels": 0.0, "pop": 0.0, "ztail": 0.0, "resid": 0.0, "orth": 0.0, "sweeps": 0, "off": 0.0, "n_levels": 0, "n_thermal": 0}
_HOST = {"levels": 0.0, "dlevels": 0.0, "pop": 0.0, "ztail": 0.0, "dpop": 0.0, "dztail": 0.0, "sweeps": 0, "n": 0}


# ---------------------------------------------------------------------------------------------------------------
# 1. families at every size
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SIZES)
def test_levels_families_of_every_size(s):
    cs, lev = family(s), levels_solved(s)
    assert len(cs) >= 155 and lev.shape == (len(cs), 8)
    worst = max(level_err(c, lev[t]) for t, c in enumerate(cs))
    _WORST["levels"] = max(_WORST["levels"], worst); _WORST["n_levels"] += len(cs)
    print(f"[levels device] s={s}: {len(cs)} blocks, worst |level - eigvalsh| / ||A||_inf = {worst:.2e}")


@pytest.mark.parametrize("s", SIZES)
def test_thermal_families_of_every_size(s):
    cap = TC.thermal_lib().qdht_sweep_cap()
    worst = dict(pop=0.0, ztail=0.0, resid=0.0, orth=0.0, sweeps=0, off=0.0)
    n = with_v = 0
    for c, kT, r, t in thermal_tasks(s):
        f = thermal_err(c, kT, r, t, cap)
        worst = {k: max(v, f[k]) for k, v in worst.items()}
        n += 1; with_v += r.V is not None
    assert n == 3 * len(family(s)) and with_v == len(family(s))
    for k, v in worst.items():
        _WORST[k] = max(_WORST[k], v)
    _WORST["n_thermal"] += n
    print(f"[thermal device] s={s}: {n} tasks, worst err / tol populations {worst['pop']:.2e}, ztail {worst['ztail']:.2e}; residual "
          f"{worst['resid']:.2e} ||A||_inf, orthogonality {worst['orth']:.2e}, sweeps {worst['sweeps']} of {cap}, "
          f"off-diagonal left {worst['off']:.2e}")


# ---------------------------------------------------------------------------------------------------------------
# 2. every section width
# ---------------------------------------------------------------------------------------------------------------
SECTION_SIZES = (2, 3, 5, 8, 17, 32)


@functools.lru_cache(maxsize=None)
def section_blocks():
    rng = np.random.default_rng(3)
    out = []
    for s in SECTION_SIZES:
        A = EC.hop_block(rng, s, 1.0)
        out.append(types.SimpleNamespace(tag=("sections", s), A=A, s=s, hn=EC.hnorm(A), w=np.linalg.eigvalsh(A)))
    return out


@functools.lru_cache(maxsize=None)
def section_solved(L):
    return dev_levels([c.A for c in section_blocks()], L)


@pytest.mark.parametrize("L", range(1, 9))
def test_every_section_width(L):
    """Le = min(L, s) levels share the 64 lanes, P = 64 // Le each: 64, 32, 21, 16, 12, 10, 9, 8 (L = 3, 5, 6, 7 leave lanes
    without a level).  Fewer levels: other sections, the same eigenvalues"""
    full = section_solved(8)
    lev = section_solved(L)
    widths = set()
    for t, c in enumerate(section_blocks()):
        level_err(c, lev[t], L)
        n = min(L, c.s)
        widths.add(64 // n)
        assert np.abs(lev[t, :n] - full[t, :n]).max() <= 2 * LC.BAR * c.hn, (L, c.s)
    assert 64 // L in widths


# ---------------------------------------------------------------------------------------------------------------
# 3. bitwise properties
# ---------------------------------------------------------------------------------------------------------------
def test_exact_multiplicities_come_back_bitwise_equal():
    """the matrices of the CPU test of this name: levels k and k + 1 are the same bits exactly where the reference's are equal"""
    d = np.array([0.75, 0.25, 0.75, 1.5, 0.25, 0.25, 3.0, 1.5, 7.0])
    B = np.array([[0.3, -0.7], [-0.7, 1.1]])
    wB = np.linalg.eigvalsh(B)
    inter = np.zeros((5, 5)); inter[:2, :2] = B; inter[2:4, 2:4] = B + 0.2 * np.eye(2); inter[4, 4] = 0.1
    cases = [("repeats", np.diag(d), np.sort(d)), ("repeats + 4096", np.diag(d + 4096.0), np.sort(d) + 4096.0),
             ("two copies", np.kron(np.eye(2), B), np.repeat(wB, 2)), ("three copies", np.kron(np.eye(3), B), np.repeat(wB, 3)),
             ("interleaved components", inter, np.linalg.eigvalsh(inter))]
    lev = dev_levels([A for _, A, _ in cases], 8)
    for t, (tag, A, w) in enumerate(cases):
        n = min(8, A.shape[0])
        w = w[:n]
        assert np.all(np.isposinf(lev[t, n:])) and np.abs(lev[t, :n] - w).max() <= LC.BAR * EC.hnorm(A), (tag, lev[t])
        for k in range(n - 1):
            assert same_bits(lev[t, k], lev[t, k + 1]) == (w[k] == w[k + 1]), (tag, k, lev[t])
    assert len(set(np.linalg.eigvalsh(inter))) == 5


def test_zero_couplings_never_rotate():
    """the matrices of test_zero_couplings_give_the_classical_distribution at every size and its four temperatures: no sweep,
    V = I and lam = diag(A) bit for bit, P within 64 eps of the softmax of the shifted diagonal"""
    mats, kTs = [], []
    for s in EC.LANE_SIZES:
        rng = np.random.default_rng(500 + s)
        for A in (EC.classical_block(s), np.diag(4096.0 + rng.uniform(0, 2, s))):
            for kT in (1e-3, 0.05, 1.0, 30.0):
                mats.append(A); kTs.append(kT)
    r = dev_thermal(mats, kTs, want_v=True)
    for t, (A, kT) in enumerate(zip(mats, kTs)):
        s = A.shape[0]
        d = np.diag(A) - np.diag(A).min()
        with np.errstate(under="ignore"):
            ref = TH.softmax(-d / kT)
        assert r.sweeps[t] == 0 and r.asym[t] == 0.0 and r.off[t] == 0.0, (s, kT, r.sweeps[t])
        assert same_bits(r.V[t, :s, :s], np.eye(s)) and same_bits(r.lam[t, :s], np.diag(A)), (s, kT)
        assert np.abs(r.pop[t, :s] - ref).max() <= 64 * EPS, (s, kT, np.abs(r.pop[t, :s] - ref).max())
        assert abs(r.ztail[t] - ref.min()) <= 64 * EPS


def test_degenerate_lowest_pair_has_bitwise_equal_populations():
    """the exactly doubly degenerate lowest pair of the CPU test, as a diagonal with a repeat, with and without the offset;
    and two identical disconnected 2 x 2 blocks, which do rotate: the same rotations on the same entries"""
    mats, kTs = [], []
    for off in (0.0, 4096.0):
        for kT in (1e-3, 0.1, 10.0):
            mats.append(np.diag(np.array([0.75, 0.25, 1.5, 0.25, 3.0, 7.0]) + off)); kTs.append(kT)
    B = np.array([[0.3, -0.7], [-0.7, 1.1]])
    mats.append(np.kron(np.eye(2), B)); kTs.append(0.4)
    r = dev_thermal(mats, kTs, want_v=True)
    for t in range(6):
        A, P = mats[t], r.pop[t, :6]
        d = np.diag(A) - np.diag(A).min()
        with np.errstate(under="ignore"):
            ref = TH.softmax(-d / kTs[t])
        assert r.sweeps[t] == 0 and same_bits(r.V[t, :6, :6], np.eye(6)) and same_bits(r.lam[t, :6], np.diag(A)), t
        assert same_bits(P[1], P[3]) and P[1] > 0, (t, P)
        assert np.abs(P - ref).max() <= 64 * EPS, (t, P)
        if kTs[t] == 1e-3:
            assert P[1] == 0.5
    P = r.pop[6, :4]
    assert r.sweeps[6] > 0 and same_bits(P[0], P[2]) and same_bits(P[1], P[3]) and r.asym[6] == 0.0, P
    Pr, _, _ = TH.reference(mats[6], 0.4)
    assert np.abs(P - Pr).max() <= TH.tol_occ(mats[6], 0.4, 1.0)


# ---------------------------------------------------------------------------------------------------------------
# 4. independence from neighbours, block count and stale LDS
# ---------------------------------------------------------------------------------------------------------------
# neighbours in the list: 32 then 1, 32 then 31, an even size then a smaller odd one (8 -> 5, 16 -> 3, 30 -> 7, 12 -> 9, 22 -> 21)
MIX_CYCLE = (32, 1, 32, 31, 8, 5, 16, 3, 2, 17, 30, 7, 12, 9, 4, 22, 21)
MIX_ROUNDS = 16


@functools.lru_cache(maxsize=None)
def mixed_list():
    """(mats, kT): EC.lane_mix_family (hop blocks at scales 1e-22, 1 and 1e44, a near-degenerate pair) over the sizes of
    MIX_CYCLE, interleaved, each size starting at another kind; 1 x 1 blocks; a classical block behind every round"""
    rng = np.random.default_rng(4242)
    fams = {}
    for pos, s in enumerate(MIX_CYCLE):
        if s > 1 and s not in fams:
            fams[s] = iter(list(EC.lane_mix_family(s, 2 * MIX_ROUNDS + 4))[pos % 4:])
    mats = []
    for r in range(MIX_ROUNDS):
        for s in MIX_CYCLE:
            mats.append(np.array([[rng.uniform(-3, 3) * 10.0 ** rng.integers(-3, 4)]]) if s == 1 else next(fams[s]))
        mats.append(EC.classical_block(2 + (5 * r) % 31))
    kT = [TC._temperatures(A)[t % 3] for t, A in enumerate(mats)]
    return mats, kT


def test_mixed_list_has_the_neighbours_it_promises():
    mats, _ = mixed_list()
    sz = [A.shape[0] for A in mats]
    pairs = set(zip(sz[:-1], sz[1:]))
    assert len(mats) >= 256 and {(32, 1), (32, 31), (8, 5), (16, 3), (30, 7), (12, 9), (22, 21)} <= pairs
    assert sum(1 for a, b in pairs if a % 2 == 0 and b % 2 == 1 and 1 < b < a) >= 5
    big = sum(1 for A in mats if np.abs(A).max() > 1e40)
    tiny = sum(1 for A in mats if A.shape[0] > 1 and 0 < np.abs(A - np.diag(np.diag(A))).max() < 1e-20)
    classical = sum(1 for A in mats if A.shape[0] > 1 and not (A - np.diag(np.diag(A))).any())
    assert big >= 32 and tiny >= 32 and classical >= MIX_ROUNDS


RUNS = [(blocks, poison) for blocks in (1, 7, 0) for poison in (0, 1, 2)]


@functools.lru_cache(maxsize=None)
def mixed_levels(blocks, poison):
    return dev_levels(mixed_list()[0], 8, blocks=blocks, poison=poison)


@functools.lru_cache(maxsize=None)
def mixed_thermal(blocks, poison):
    mats, kT = mixed_list()
    return dev_thermal(mats, kT, blocks=blocks, poison=poison, want_v=True)


@pytest.mark.parametrize("blocks,poison", RUNS)
def test_levels_do_not_depend_on_neighbours_blocks_or_stale_lds(blocks, poison):
    """one wave solving the whole list in order, seven blocks, one block per task (the last tasks as second trips), each with
    the workspace as found, poisoned once and poisoned before every task: the bits of (blocks = 0, poison = 2), where every
    task but sixteen starts from a freshly poisoned workspace of its own"""
    mats, _ = mixed_list()
    base, got = mixed_levels(0, 2), mixed_levels(blocks, poison)
    assert not np.isnan(got).any(), (blocks, poison, np.argwhere(np.isnan(got))[:8])
    for t, A in enumerate(mats):
        assert same_bits(got[t], base[t]), (blocks, poison, t, A.shape[0], got[t], base[t])
    if (blocks, poison) == (1, 0):                         # equal bits are not two wrong answers
        for t, A in enumerate(mats):
            level_err(types.SimpleNamespace(tag=("mixed list", t), s=A.shape[0], hn=EC.hnorm(A), w=np.linalg.eigvalsh(A)), got[t])


@pytest.mark.parametrize("blocks,poison", RUNS)
def test_thermal_does_not_depend_on_neighbours_blocks_or_stale_lds(blocks, poison):
    mats, kT = mixed_list()
    base, got = mixed_thermal(0, 2), mixed_thermal(blocks, poison)
    for name in THERMAL_FIELDS:
        a = getattr(got, name)
        assert not np.isnan(a).any(), (blocks, poison, name, np.argwhere(np.isnan(a))[:8])
    for t, A in enumerate(mats):
        for name in THERMAL_FIELDS:
            a, b = getattr(got, name)[t], getattr(base, name)[t]
            assert np.array_equal(a, b) if name == "sweeps" else same_bits(a, b), (blocks, poison, t, A.shape[0], name)
    if (blocks, poison) == (1, 0):
        cap = TC.thermal_lib().qdht_sweep_cap()
        for t, A in enumerate(mats):
            c = types.SimpleNamespace(tag=("mixed list", t), A=A, s=A.shape[0], hn=EC.hnorm(A))
            # (sum P = sum_k w_k |V_k|^2 / Z carries the orthogonality error of V, up to 1e-13 by its own bar: at kT of ten times
            # the spread a 32-state block of this list misses 64 eps in the host build too, so that bar stays with its families)
            thermal_err(c, kT[t], got, t, cap, sum_bar=False)


# ---------------------------------------------------------------------------------------------------------------
# 5. distance from the host build (a measurement)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SIZES)
def test_device_against_host_build(s):
    """the same source with the 64 lanes as a loop, IEEE division and sqrt and libm's exp: what the rcp / rsq + Newton primitives
    and ocml's exp cost.  Printed, not asserted (each build meets the bars of 1 on its own)"""
    cs, lev = family(s), levels_solved(s)
    w = dict(levels=0.0, dlevels=0.0, pop=0.0, ztail=0.0, dpop=0.0, dztail=0.0, sweeps=0)
    for t, c in enumerate(cs):
        n = min(8, s)
        host = LC.solve(c.A, n)
        if c.hn:
            w["levels"] = max(w["levels"], np.abs(host[:n] - c.w[:n]).max() / c.hn)
            w["dlevels"] = max(w["dlevels"], np.abs(host[:n] - lev[t, :n]).max() / c.hn)
    for c, kT, r, t in thermal_tasks(s):
        sw, P, _, _, z = TC.solve(c.A, kT)
        Pr, wt, _ = TH.reference(c.A, kT)
        to, tz = TH.tol_occ(c.A, kT, 1.0), TC.tol_ztail(c.A, kT)
        w["pop"] = max(w["pop"], np.abs(P - Pr).max() / to); w["ztail"] = max(w["ztail"], abs(z - wt[-1]) / tz)
        w["dpop"] = max(w["dpop"], np.abs(P - r.pop[t, :s]).max() / to); w["dztail"] = max(w["dztail"], abs(z - r.ztail[t]) / tz)
        w["sweeps"] = max(w["sweeps"], sw)
    assert all(np.isfinite(v) for v in w.values())
    for k, v in w.items():
        _HOST[k] = max(_HOST[k], v)
    _HOST["n"] += 1
    print(f"[device vs host] s={s}: levels |dev - host| / ||A|| {w['dlevels']:.2e} (host against eigvalsh {w['levels']:.2e}); "
          f"populations |dev - host| / tol {w['dpop']:.2e}, ztail {w['dztail']:.2e} (host against the reference: {w['pop']:.2e}, "
          f"{w['ztail']:.2e}; host sweeps {w['sweeps']})")


def test_worst_figures_are_reported():
    """the figures of the docstring, over whatever of 1 and 5 ran in this session"""
    print(f"[spectrum device] levels: {_WORST['n_levels']} tasks, worst |level - eigvalsh| / ||A||_inf {_WORST['levels']:.2e} "
          f"(bar {LC.BAR:.0e}); host build {_HOST['levels']:.2e}; |device - host| / ||A||_inf {_HOST['dlevels']:.2e}")
    print(f"[spectrum device] thermal: {_WORST['n_thermal']} tasks, worst err / tol populations {_WORST['pop']:.2e}, ztail "
          f"{_WORST['ztail']:.2e}; residual {_WORST['resid']:.2e} ||A||_inf, orthogonality {_WORST['orth']:.2e}, sweeps "
          f"{_WORST['sweeps']}, off-diagonal left {_WORST['off']:.2e}; host build: populations {_HOST['pop']:.2e}, ztail "
          f"{_HOST['ztail']:.2e}, sweeps {_HOST['sweeps']}; |device - host| / tol populations {_HOST['dpop']:.2e}, ztail "
          f"{_HOST['dztail']:.2e}")
    assert _WORST["levels"] <= LC.BAR and _WORST["pop"] <= 1.0 and _WORST["ztail"] <= 1.0
