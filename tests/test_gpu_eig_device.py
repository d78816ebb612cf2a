"""The three dense eigen-solvers of the ground-state stage ON THE DEVICE (run with -m gpu): the register solver
qd_eig_lowest<S>, the memory solver qd_eig_lowest_mem and the wave-per-block solver qd_eig_wave_lowest, through the
product's own task wrappers (tests/gputest_eig), on the matrices that tests/test_eig_solver_cpu.py and
tests/test_eig_wave_cpu.py run through the host builds (tests/eig_cases.py), against numpy.linalg.eigh in float64.

  (a) per-lane solvers, every size 2..32;  (b) wide solver, every size 33..64 and the small sizes it accepts: the bars of
      the two CPU files, with the residual recomputed on the host from the returned vector;
  (c) what only exists on the device, bit for bit: lane independence under the lane-vote Laguerre loop, partial waves and
      blocks, stale LDS of a persistent block, aliased against separate output, product mode against validate mode;
      and the rcp / rsq + Newton primitives themselves against 80-bit arithmetic;
  (d) device against host build of the same source: what the rcp / rsq + Newton primitives cost.

Every family is solved once per instantiation, in one launch per size class, and the results are shared by the tests."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest

import helpers as H
import eig_cases as EC

pytestmark = pytest.mark.gpu

_LIB = None
_LDX = 64


def lib():
    global _LIB
    if _LIB is None:
        # QDSIM_GPUTEST_EIG_LIB: a diagnostic build of the harness (a sensitivity check with a changed header, say)
        path = os.environ.get("QDSIM_GPUTEST_EIG_LIB", os.path.join(H.ROOT, "tests", "gputest_eig", "libqdsim_gputest_eig.so"))
        if not os.path.exists(path):
            raise RuntimeError(f"{path} not found: build it with __graft_entry__.build() (or make -C tests/gputest_eig)")
        import torch  # noqa: F401  (first: the harness then shares torch's HIP runtime, as qadapt_hip._lib.lib() does)
        L = ctypes.CDLL(path)
        dp, ip, ci = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.c_int
        tail = [dp, dp, ci, dp, ip, ctypes.c_char_p, ci]
        L.qdg_eig_reg.argtypes = [ci, ci, ip, dp, ci, ci, ci] + tail
        L.qdg_eig_mem.argtypes = [ci, ip, dp, ci, ci, ci] + tail
        L.qdg_eig_wide.argtypes = [ci, ip, dp, ci, ci, ci, ci] + tail
        L.qdg_prims.argtypes = [ci, dp, dp, ctypes.c_char_p, ci]
        for f in (L.qdg_eig_reg, L.qdg_eig_mem, L.qdg_eig_wide, L.qdg_prims):
            f.restype = ci
        _LIB = L
    return _LIB


def lane_class(s):
    """solver of a block of s states: the register classes' S (9 and 11 run padded in 10 and 12), 'mem' above 12"""
    return s if s <= 8 else (10 if s <= 10 else (12 if s <= 12 else "mem"))


def dev_solve(mats, cls, validate=True, blocks=0, aliased=True, solo=False):
    """One launch: the blocks `mats`, in this order (task t = lane t of the launch for the per-lane classes), through the
    class `cls` (2..8, 10, 12: register; 'mem'; 'wide'); solo: every task in a launch of its own instead.
    Returns lam (n), x (n, 64; zero beyond the block), res (n), it (n)."""
    n = len(mats)
    sizes = np.array([A.shape[0] for A in mats], np.int32)
    smax = int(sizes.max())
    ld = smax * (smax + 1) // 2
    pk = np.zeros((n, ld))
    for t, A in enumerate(mats):
        p = EC.packed(A)
        pk[t, :len(p)] = p
    lam = np.zeros(n); x = np.zeros((n, _LDX)); res = np.zeros(n); it = np.zeros(n, np.int32)
    err = ctypes.create_string_buffer(512)
    tail = (H._p(lam, ctypes.c_double), H._p(x, ctypes.c_double), _LDX, H._p(res, ctypes.c_double), H._p(it, ctypes.c_int),
            err, len(err))
    head = (n, H._p(sizes, ctypes.c_int), H._p(pk, ctypes.c_double), ld, int(validate))
    L = lib()
    if cls == "wide":
        rc = L.qdg_eig_wide(*head, int(blocks), int(aliased), *tail)
    elif cls == "mem":
        rc = L.qdg_eig_mem(*head, int(solo), *tail)
    else:
        rc = L.qdg_eig_reg(int(cls), *head, int(solo), *tail)
    assert rc == 0, (cls, rc, err.value.decode())
    return types.SimpleNamespace(lam=lam, x=x, res=res, it=it)


def lane_solve(mats, validate=True):
    """blocks of 2..32 states, each through its own class: one launch per class present, input order kept inside a class"""
    n = len(mats)
    out = types.SimpleNamespace(lam=np.zeros(n), x=np.zeros((n, _LDX)), res=np.zeros(n), it=np.zeros(n, np.int32))
    groups = {}
    for t, A in enumerate(mats):
        groups.setdefault(lane_class(A.shape[0]), []).append(t)
    for cls, idx in groups.items():
        r = dev_solve([mats[t] for t in idx], cls, validate)
        out.lam[idx] = r.lam; out.x[idx] = r.x; out.res[idx] = r.res; out.it[idx] = r.it
    return out


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(b, np.float64).view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------
# the families: matrices, float64 reference (once), device results per instantiation (once)
# ---------------------------------------------------------------------------------------------------------------
def _case(tag, A, hn=None):
    w, V = np.linalg.eigh(A)
    hn = EC.hnorm(A) if hn is None else hn
    return types.SimpleNamespace(tag=tag, A=A, s=A.shape[0], hn=hn, w0=w[0], gap=(w[1] - w[0]) / hn, v0=V[:, 0].copy())


@functools.lru_cache(maxsize=None)
def cases(name):
    if name == "scales":
        return [_case((s, ts, k), A) for s in EC.LANE_SIZES for k, (ts, A) in enumerate(EC.scale_family(s))]
    if name == "classical":
        return [_case(s, EC.classical_block(s)) for s in EC.CLASSICAL_SIZES]
    if name == "near_degenerate":
        return [_case((s, sep, tc), A, hn) for s, sep in EC.NEAR_DEGENERATE for tc, A, hn in EC.near_degenerate_family(s, sep)]
    if name == "mixed":
        return [_case((s, k), A) for s in EC.MIXED_SIZES for k, A in enumerate(EC.mixed_scale_family(s))]
    if name == "extreme":
        return [_case((s, k), A) for s in EC.EXTREME_SIZES for k, A in enumerate(EC.extreme_scale_family(s, 40))]
    if name == "regressions":
        return [_case("small entries", EC.small_entry_block()), _case("column tail", EC.column_tail_block())]
    if name == "wide_random":
        return [_case(tag, A) for s in EC.WIDE_SIZES for tag, A in EC.wide_random_family(s)]
    if name == "wide_hop":
        return [_case(tag, A) for s in EC.WIDE_HOP_SIZES for tag, A in EC.wide_hop_family(s)]
    if name == "wide_small":
        return [_case(tag, A) for tag, A in EC.wide_small_family()]
    if name == "wide_degenerate":
        return [_case(tag, A) for tag, A in EC.wide_degenerate_family()]
    if name == "wide_underflow":
        return [_case(tag, A) for tag, A in EC.wide_underflow_family()]
    if name == "wide_sectors":
        # 432 sector blocks in the (4, 3) scene: every second one
        return [_case(tag, A) for tag, A, _ in EC.wide_sector_family(4, 3, stride=2)]
    raise KeyError(name)


LANE_FAMILIES = ("scales", "classical", "near_degenerate", "mixed", "extreme", "regressions")
WIDE_FAMILIES = ("wide_random", "wide_hop", "wide_small", "wide_degenerate", "wide_underflow", "wide_sectors")


def solved(name, validate=True):
    return _solved(name, bool(validate))


@functools.lru_cache(maxsize=None)
def _solved(name, validate):
    mats = [c.A for c in cases(name)]
    return dev_solve(mats, "wide", validate) if name.startswith("wide") else lane_solve(mats, validate)


def vec_err(x, v0):
    return min(np.abs(x - v0).max(), np.abs(x + v0).max())


def host_resid(c, lam, x):
    return np.linalg.norm(c.A @ x - lam * x)


class Worst:
    """largest figures of a family, printed for DESIGN.md"""
    def __init__(self):
        self.lam = self.res = self.vec = 0.0
        self.compared = 0

    def add(self, c, lam, res, err=None):
        self.lam = max(self.lam, abs(lam - c.w0) / c.hn); self.res = max(self.res, res / c.hn)
        if err is not None:
            self.vec = max(self.vec, err); self.compared += 1

    def __str__(self):
        return (f"|lam - w0| / ||A|| {self.lam:.2e}, residual / ||A|| {self.res:.2e}, "
                f"eigenvector difference {self.vec:.1e} over {self.compared} resolved blocks")


# the reported residual against its recomputation: the bar of test_eig_wave_cpu.check, whose 64-term argument covers the
# per-lane sizes (at most 32 terms per row) a fortiori
RES_AGREE = 3e-14


def check_lane(c, r, t, worst, lam_bar=4e-15, res_bar=4e-15, vec="resolved"):
    """the bars of tests/test_eig_solver_cpu.py on task t of the result r"""
    s, hn = c.s, c.hn
    lam, x, res, it = r.lam[t], r.x[t, :s], r.res[t], r.it[t]
    assert np.isfinite(lam) and np.isfinite(res) and np.all(np.isfinite(x)), c.tag
    assert not r.x[t, s:].any(), c.tag
    rh = host_resid(c, lam, x)
    if lam_bar is not None:
        assert abs(lam - c.w0) <= lam_bar * hn, (c.tag, lam, c.w0, abs(lam - c.w0) / hn)
    assert res <= res_bar * hn, (c.tag, res / hn)
    assert rh <= res_bar * hn, (c.tag, rh / hn)
    assert abs(rh - res) <= RES_AGREE * hn, (c.tag, rh / hn, res / hn)
    assert abs(np.linalg.norm(x) - 1) < 1e-14, c.tag
    err = None
    if vec == "resolved":
        if c.gap > 1e-9:
            # eigenvector error of any backward-stable solver ~ eps / gap
            err = vec_err(x, c.v0)
            assert err <= 2e-7 + 1e-15 / c.gap, (c.tag, err, c.gap)
    elif vec == "near_degenerate":
        err = vec_err(x, c.v0)
        assert err <= 1e-6 * max(1.0, 1e-9 / c.gap) + 2e-15 / c.gap, (c.tag, err, c.gap)
    assert 0 <= it <= 64, (c.tag, it)
    worst.add(c, lam, max(res, rh), err)


def check_wide(c, r, t, worst):
    """test_eig_wave_cpu.check on task t of the result r"""
    s, hn = c.s, c.hn
    lam, x, res, it = r.lam[t], r.x[t, :s], r.res[t], r.it[t]
    assert np.isfinite(x).all() and np.isfinite(lam) and np.isfinite(res), c.tag
    assert not r.x[t, s:].any(), c.tag
    assert abs(lam - c.w0) <= 1e-12 * hn, (c.tag, lam, c.w0, hn)
    rh = host_resid(c, lam, x)
    assert res <= 1e-13 * hn, (c.tag, res / hn)
    assert rh <= 1e-13 * hn, (c.tag, rh / hn)
    assert abs(np.linalg.norm(x) - 1) < 1e-13, c.tag
    assert abs(rh - res) <= RES_AGREE * hn, (c.tag, rh / hn, res / hn)
    err = None
    if c.gap > H.GAP_MIN:
        err = vec_err(x, c.v0)
        assert err <= 1e-8, (c.tag, err, c.gap)
    assert 1 <= it <= 64, (c.tag, it)
    worst.add(c, lam, max(res, rh), err)


# ---------------------------------------------------------------------------------------------------------------
# (a) per-lane solvers
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", EC.LANE_SIZES)
def test_lowest_pair_matches_eigh_over_scales(s):
    cs, r = cases("scales"), solved("scales")
    worst = Worst()
    idx = [t for t, c in enumerate(cs) if c.s == s]
    assert len(idx) == 54
    for t in idx:
        check_lane(cs[t], r, t, worst)
    print(f"device, scales, s={s}: {worst}")
    assert worst.compared > 0


def test_classical_limit():
    cs, r = cases("classical"), solved("classical")
    worst = Worst()
    for t, c in enumerate(cs):
        check_lane(c, r, t, worst)
        k = int(np.argmin(np.diag(c.A)))
        assert r.lam[t] == pytest.approx(c.A[k, k], abs=1e-15) and abs(abs(r.x[t, k]) - 1) < 1e-12
    print(f"device, classical: {worst}")
    assert worst.compared > 0


def test_near_degenerate_lowest_pair_at_huge_coupling():
    cs, r = cases("near_degenerate"), solved("near_degenerate")
    worst = Worst()
    for t, c in enumerate(cs):
        check_lane(c, r, t, worst, res_bar=2e-14, vec="near_degenerate")
    print(f"device, near-degenerate: {worst}")
    assert worst.compared == len(cs) == 14


@pytest.mark.parametrize("s", EC.MIXED_SIZES)
def test_mixed_coupling_scales_inside_one_block(s):
    cs, r = cases("mixed"), solved("mixed")
    worst = Worst()
    idx = [t for t, c in enumerate(cs) if c.s == s]
    assert len(idx) == 40
    for t in idx:
        check_lane(cs[t], r, t, worst)
    print(f"device, mixed scales, s={s}: {worst}")
    assert worst.compared > 0


@pytest.mark.parametrize("s", EC.EXTREME_SIZES)
def test_extreme_scale_mix_never_gives_nan(s):
    """the first 40 matrices per size of the CPU test's 200: its finiteness and residual bar"""
    cs, r = cases("extreme"), solved("extreme")
    worst = Worst()
    idx = [t for t, c in enumerate(cs) if c.s == s]
    assert len(idx) == 40
    for t in idx:
        check_lane(cs[t], r, t, worst, lam_bar=None, res_bar=1e-14, vec=None)
    print(f"device, extreme scale mix, s={s}: residual / ||A|| {worst.res:.2e}")


def test_regression_matrices():
    cs, r = cases("regressions"), solved("regressions")
    worst = Worst()
    small, tail = cs
    # the 5x5 block with a vector entry of 3e-7: the absolute bars of the CPU test, every entry to relative accuracy
    check_lane(small, r, 0, worst)
    x = r.x[0, :5]
    v0 = small.v0 * np.sign(small.v0[0]) * np.sign(x[0])
    assert r.res[0] <= 2e-15 and host_resid(small, r.lam[0], x) <= 2e-15 and abs(r.lam[0] - small.w0) <= 1e-15
    assert np.all(np.abs(x - v0) <= 1e-13 * np.abs(v0) + 1e-20), (x, v0)
    # the 10-state block whose column tail underflowed
    check_lane(tail, r, 1, worst)
    print(f"device, regression matrices: {worst}")
    assert worst.compared > 0


# ---------------------------------------------------------------------------------------------------------------
# (b) wide solver
# ---------------------------------------------------------------------------------------------------------------
def _check_wide_family(name, select=lambda c: True):
    cs, r = cases(name), solved(name)
    worst = Worst()
    n = 0
    for t, c in enumerate(cs):
        if select(c):
            check_wide(c, r, t, worst); n += 1
    return n, worst


@pytest.mark.parametrize("s", EC.WIDE_SIZES)
def test_random_symmetric_blocks_of_every_wide_size(s):
    n, worst = _check_wide_family("wide_random", lambda c: c.s == s)
    print(f"device, wide random, s={s}: {worst}")
    assert n == 15 and worst.compared > 0


@pytest.mark.parametrize("s", EC.WIDE_HOP_SIZES)
def test_hop_type_blocks_over_coupling_scales(s):
    n, worst = _check_wide_family("wide_hop", lambda c: c.s == s)
    print(f"device, wide hop, s={s}: {worst}")
    assert n == 27 and worst.compared > 0


def test_small_sizes_run_too():
    n, worst = _check_wide_family("wide_small")
    print(f"device, wide solver on small sizes: {worst}")
    assert n == len(EC.WIDE_SMALL_SIZES) and worst.compared > 0


def test_degenerate_trio_and_underflowing_tails():
    """the 48x48 pairs split by ~1e-11 ||A||, ~1e-6 ||A|| and not at all (none of them resolves its ground vector: the
    eigenvalue, residual and norm bars are what they check) and the 40x40 blocks whose Householder tails underflow"""
    n3, w3 = _check_wide_family("wide_degenerate")
    n2, w2 = _check_wide_family("wide_underflow")
    print(f"device, wide degenerate trio: {w3}")
    print(f"device, wide underflow pair: {w2}")
    assert n3 == 3 and n2 == 2 and w3.compared + w2.compared > 0


def test_real_sector_blocks():
    n, worst = _check_wide_family("wide_sectors")
    print(f"device, (4,3) sector blocks: {n} blocks, {worst}")
    assert 200 <= n <= 400 and worst.compared > 0


# ---------------------------------------------------------------------------------------------------------------
# (c) device-only structure: exact equalities
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(4,), (7,), (8,), (9, 10), (11, 12), (20,)], ids=str)
def test_lanes_do_not_disturb_each_other(sizes):
    """64 tasks of one class with different Laguerre iteration counts in ONE wave (converged lanes idle next to lanes
    still iterating, under the lane vote) against each task alone in a launch of one active lane"""
    fams = [list(EC.lane_mix_family(s)) for s in sizes]
    mats = [fams[t % len(sizes)][t] for t in range(64)]
    cls = lane_class(sizes[-1])
    packed64 = dev_solve(mats, cls)
    assert len(set(packed64.it.tolist())) >= 3, sorted(set(packed64.it.tolist()))
    alone = dev_solve(mats, cls, solo=True)
    for t in range(64):
        assert same_bits(alone.lam[t], packed64.lam[t]) and same_bits(alone.x[t], packed64.x[t]), (sizes, t)
        assert same_bits(alone.res[t], packed64.res[t]) and alone.it[t] == packed64.it[t], (sizes, t)


@pytest.mark.parametrize("cls", [3, 8, 10, 12, "mem"], ids=str)
@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_partial_waves_and_blocks(cls, n):
    """task counts that leave a wave or a block partly filled: every task as in the full launches of (a)"""
    cs, r = cases("scales"), solved("scales")
    idx = [t for t, c in enumerate(cs) if lane_class(c.s) == cls]
    idx = [idx[(7 * k) % len(idx)] for k in range(n)]
    got = dev_solve([cs[t].A for t in idx], cls)
    assert same_bits(got.lam, r.lam[idx]) and same_bits(got.x, r.x[idx]), (cls, n)
    assert same_bits(got.res, r.res[idx]) and np.array_equal(got.it, r.it[idx]), (cls, n)


def _by_tag(name, tag):
    return next(c for c in cases(name) if c.tag == tag)


def test_persistent_block_keeps_nothing_from_the_task_before():
    """one persistent block (the workspace in LDS is reused from task to task): a block solved first, after a 64-state
    block at scale 1e44 and after a 2-state block gives the same bits"""
    a33 = _by_tag("wide_random", (33, 1.0, 0)).A
    a64 = _by_tag("wide_random", (64, 1.0, 0)).A
    big = _by_tag("wide_random", (64, 1e44, 0)).A
    two = _by_tag("wide_small", 2).A
    for target, befores in ((a33, (big, two)), (a64, (a33, two))):
        first = dev_solve([target], "wide", blocks=1)
        for before in befores:
            r = dev_solve([before, target], "wide", blocks=1)
            assert same_bits(r.lam[1], first.lam[0]) and same_bits(r.x[1], first.x[0]), (target.shape, before.shape)
            assert same_bits(r.res[1], first.res[0]) and r.it[1] == first.it[0], (target.shape, before.shape)


@pytest.mark.parametrize("validate", [True, False])
def test_aliased_output_equals_separate_output(validate):
    """the product hands the record itself to the wide solver as its output"""
    for name in ("wide_random", "wide_small", "wide_underflow"):
        a = solved(name, validate)
        b = dev_solve([c.A for c in cases(name)], "wide", validate, aliased=False)
        assert same_bits(a.lam, b.lam) and same_bits(a.x, b.x) and same_bits(a.res, b.res), name
        assert np.array_equal(a.it, b.it), name


@pytest.mark.parametrize("name", LANE_FAMILIES + WIDE_FAMILIES)
def test_product_mode_equals_validate_mode(name):
    """VALIDATE = false is what the benchmark times: same eigenvalue and vector, bit for bit"""
    v, p = solved(name, True), solved(name, False)
    assert same_bits(v.lam, p.lam), name
    assert same_bits(v.x, p.x), name
    assert not p.res.any() and not p.it.any()


def test_reciprocal_and_square_root_primitives():
    """qd_rcp, qd_rcp1, qd_sqrt1, qd_sqrt_rsqrt as the device compiles them (rcp / rsq builtin + Newton steps; the host
    build divides and calls sqrt) against 80-bit arithmetic, over what the solvers can pass them: after the scaling to
    ||A|| in [1, 2) every argument is a pivot, a norm or a minor of magnitude 1e-300 .. 1e300 (the guards of qd_eig.h add
    1e-300 or drop the column below that).  Random mantissas at log-uniform magnitudes, exact powers of two, and the
    neighbours of 1, 2 and 4.  Bars: qd_eig.h documents the two-step forms at <= 2.4e-16 (qd_sqrt1: ~1 ulp = 2.2e-16); the
    one-step qd_rcp1 squares the builtin's documented 4.6e-8 and rounds twice: 2.12e-15 + 2.2e-16 <= 2.4e-15."""
    rng = np.random.default_rng(2024)
    x = [rng.uniform(1.0, 10.0, 1 << 16) * 10.0 ** rng.integers(-300, 300, 1 << 16), 2.0 ** np.arange(-996, 997, 4.0)]
    for c in (1.0, 2.0, 4.0):
        x.append(np.array([np.nextafter(c, 0.0), c, np.nextafter(c, 8.0)]))
    x = np.ascontiguousarray(np.concatenate(x))
    assert x.min() >= 1e-300 and x.max() <= 1e301
    n = len(x)
    out = np.zeros((5, n))
    err = ctypes.create_string_buffer(512)
    rc = lib().qdg_prims(n, H._p(x, ctypes.c_double), H._p(out, ctypes.c_double), err, len(err))
    assert rc == 0, err.value.decode()
    assert np.isfinite(out).all()
    xl = x.astype(np.longdouble)
    assert np.finfo(np.longdouble).eps < 1e-18
    rcp, sq = 1 / xl, np.sqrt(xl)
    worst = {}
    for name, got, ref, bar in (("qd_rcp", out[0], rcp, 2.4e-16), ("qd_rcp1", out[1], rcp, 2.4e-15), ("qd_sqrt1", out[2], sq, 2.4e-16),
                                ("qd_sqrt_rsqrt: sqrt", out[3], sq, 2.4e-16), ("qd_sqrt_rsqrt: 1 / sqrt", out[4], 1 / sq, 2.4e-16)):
        rel = float(np.max(np.abs(got.astype(np.longdouble) - ref) / ref))
        worst[name] = rel
        print(f"device {name}: largest relative error {rel:.2e} (bar {bar:.1e})")
    for name, bar in (("qd_rcp", 2.4e-16), ("qd_rcp1", 2.4e-15), ("qd_sqrt1", 2.4e-16), ("qd_sqrt_rsqrt: sqrt", 2.4e-16),
                      ("qd_sqrt_rsqrt: 1 / sqrt", 2.4e-16)):
        assert worst[name] <= bar, (name, worst[name])


# ---------------------------------------------------------------------------------------------------------------
# (d) device against the host build of the same source
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LANE_FAMILIES + WIDE_FAMILIES)
def test_device_against_host_build(name):
    """Both builds are within the family's bar of eigh, so they are within twice the bar of each other; the figures are
    the direct measure of the rcp / rsq + Newton substitution."""
    wide = name.startswith("wide")
    if wide:
        from test_eig_wave_cpu import solve
    else:
        from test_eig_solver_cpu import solve
    cs, r = cases(name), solved(name)
    dlam = dvec = hlam = hres = 0.0
    compared = 0
    for t, c in enumerate(cs):
        lam, x, res, it = solve(c.A)
        dlam = max(dlam, abs(r.lam[t] - lam) / c.hn)
        hlam = max(hlam, abs(lam - c.w0) / c.hn); hres = max(hres, res / c.hn)
        if c.gap > (H.GAP_MIN if wide else 1e-9):
            dvec = max(dvec, vec_err(r.x[t, :c.s], x)); compared += 1
    print(f"{name}: max |lam_dev - lam_host| / ||A|| {dlam:.2e}, max vector difference {dvec:.1e} over {compared} resolved "
          f"blocks; host build against eigh: |lam - w0| / ||A|| {hlam:.2e}, residual / ||A|| {hres:.2e}")
    if name != "extreme":                                  # (no eigenvalue bar in that family)
        assert dlam <= 2 * (1e-12 if wide else 4e-15)
    assert compared > 0 or name == "wide_degenerate"       # (no block of the trio resolves its ground vector)
