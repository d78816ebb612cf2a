"""The three exact-percentile kernels on adversarial inputs (run with -m gpu): qd_k_percentile with cached keys (n <= 32 768),
qd_k_percentile re-reading memory, and the grid-wide qd_k_sel_* select, on the families and sizes of tests/pct_cases.py,
bit for bit against np.percentile.  test_pct_cases_cpu.py shows that the kernels' rank and interpolation arithmetic IS
np.percentile's on these inputs, so a mismatch here is a selection bug: the wave-vote histogram shortcut, the bin pick at the
edge of a run of ties, the `cnt_le > in` decision, negative keys, partial blocks, the boundary between the two single-block
paths.  Then the many-block launch of qd_k_percentile and the placement kernel through qd_probe_compose."""
import ctypes

import numpy as np
import pytest

import pct_cases as PC
import qd_oracle as O
import update_helpers as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    with U.Handle(2, 1, R=8) as h:                       # one small handle: qd_time_select only borrows its select scratch
        yield h


def _select(h, z, single_block):
    """qd_time_select on the rows of z (F, n) float64: (F, 2) percentiles"""
    import torch
    F, n = z.shape
    zd = torch.from_numpy(np.ascontiguousarray(z)).cuda()
    out = torch.full((F, 2), -7.0, dtype=torch.float64).cuda()
    ms = ctypes.c_float(0)
    for f in range(F):
        rc = h.lib.qd_time_select(h.h, ctypes.c_void_p(zd[f].data_ptr()), n, int(single_block), 1,
                                  ctypes.c_void_p(out[f].data_ptr()), ctypes.byref(ms), h.stream())
        assert rc == 0, h.lib.qd_last_error(h.h)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("n", PC.SIZES)
def test_select_on_adversarial_families(handle, n):
    fam = PC.families(n)
    z = np.stack([a for _, a in fam])
    one = _select(handle, z, single_block=1)              # n <= 32 768: keys cached in registers; above: memory re-read
    grid = _select(handle, z, single_block=0)
    bad = []
    for f, (name, a) in enumerate(fam):
        ref = PC.numpy_percentiles(a)
        if not PC.same_percentiles(name, one[f], ref):
            bad.append((name, "single block", one[f].tolist(), ref.tolist()))
        if not PC.same_percentiles(name, grid[f], ref):
            bad.append((name, "grid", grid[f].tolist(), ref.tolist()))
        # the two device routes agree bit for bit (NaN with NaN), the zeros family included
        same = (U.bits(one[f]) == U.bits(grid[f])) | (np.isnan(one[f]) & np.isnan(grid[f]))
        if not same.all():
            bad.append((name, "routes differ", one[f].tolist(), grid[f].tolist()))
    assert not bad, (n, bad)


# ------------------------------------------------------------------ qd_probe_compose: many blocks, and the placement
STACK = ("const", "const_neg", "one_high", "one_low", "two_valued_lo+0", "two_valued_hi+1", "signs", "denormals", "zeros_pm",
         "few_levels", "ulp_cluster", "sorted", "reversed", "nan_last")
NX, NY = 7, 2


def _compose(h, stack, mode):
    """qd_probe_compose of channel 0 of the scans stack (nq, P): (composite (NY*R, NX*R) float32, plohi)"""
    import torch
    nq, P = stack.shape
    R = int(round(P ** 0.5))
    raw = torch.from_numpy(np.ascontiguousarray(stack).reshape(nq, 1, P)).cuda()
    comp = torch.full((NY * R, NX * R), -7.0, dtype=torch.float32).cuda()
    pl = torch.full((nq if mode else 1, 2), -7.0, dtype=torch.float64).cuda()
    rc = h.lib.qd_probe_compose(h.h, ctypes.c_void_p(raw.data_ptr()), NX, NY, 0, mode, ctypes.c_void_p(comp.data_ptr()),
                                ctypes.c_void_p(pl.data_ptr()), h.stream())
    assert rc == 0, h.lib.qd_last_error(h.h)
    torch.cuda.synchronize()
    return comp.cpu().numpy(), pl.cpu().numpy()


def _block(comp, q, R, flip):
    i, j = q // NY, q % NY
    jb = NY - 1 - j if flip else j
    return comp[jb * R:(jb + 1) * R, i * R:(i + 1) * R]


def _same_pair(got, ref):
    return bool(np.all((U.bits(got) == U.bits(ref)) | (np.isnan(got) & np.isnan(ref))))


@pytest.mark.parametrize("R", [8, 33])
def test_compose_on_adversarial_scans(R):
    """per-scan mode is the many-block launch of qd_k_percentile with n = P (64: one wave of a block; 1089: one past a
    block); global mode the grid-wide select over the whole stack"""
    P = R * R
    assert NX * NY == len(STACK)
    stack = np.stack([PC.family(P, name) for name in STACK])
    finite = np.stack([PC.family(P, name) for name in STACK[:-1]] + [PC.family(P, "few_levels") + 0.5])
    perm = np.random.default_rng(5).permutation(len(STACK))
    with U.Handle(2, 1, R=R) as h:
        comp, pl = _compose(h, stack, 1)
        comp_p, pl_p = _compose(h, stack[perm], 1)
        gcomp_nan, gpl_nan = _compose(h, stack, 0)
        gcomp, gpl = _compose(h, finite, 0)
    for q, name in enumerate(STACK):
        scan = stack[q]
        ref = PC.numpy_percentiles(scan)
        assert _same_pair(pl[q], ref) if name != "zeros_pm" else np.array_equal(pl[q], ref), (name, pl[q], ref)
        img = _block(comp, q, R, flip=True)
        want = O.normalise_image(scan.reshape(R, R))
        assert img.dtype == np.float32 and want.dtype == np.float32
        diff = img.view(np.uint32) != want.view(np.uint32)
        assert not diff.any(), (name, int(diff.sum()), img[diff][:4], want[diff][:4])
        if name in ("const", "const_neg", "nan_last"):
            assert not img.any()
    assert np.isnan(pl[len(STACK) - 1]).all()
    # no scan depends on its neighbours
    for k, q in enumerate(perm):
        assert _same_pair(pl_p[k], pl[q]), (k, q)
        assert np.array_equal(_block(comp_p, k, R, True).view(np.uint32), _block(comp, q, R, True).view(np.uint32)), (k, q)
    # global mode: a NaN anywhere gives NaN percentiles and the zero image
    assert np.isnan(gpl_nan).all() and not gcomp_nan.any()
    whole = np.zeros((NY * R, NX * R))
    for q in range(len(STACK)):
        _block(whole, q, R, flip=False)[:] = finite[q].reshape(R, R)
    ref = PC.numpy_percentiles(whole.ravel())
    assert _same_pair(gpl[0], ref), (gpl, ref)
    want = O.normalise_image(whole)
    diff = gcomp.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), (int(diff.sum()), gcomp[diff][:4], want[diff][:4])
