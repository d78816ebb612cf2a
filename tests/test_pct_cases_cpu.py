"""CPU tier of the adversarial percentile suite (tests/pct_cases.py): the families are what their names say, and the
host restatement of the kernels' rank and interpolation arithmetic equals np.percentile on all of them -- so a device
mismatch on these inputs (test_gpu_percentile_adversarial.py) is a selection bug, not a difference in definition."""
import numpy as np
import pytest

import pct_cases as PC


def test_the_case_list():
    assert len(PC.SIZES) == 20 and 32768 in PC.SIZES and 32769 in PC.SIZES
    names = [name for name, _ in PC.families(401)]
    assert len(names) == len(set(names)) == 23
    assert len(PC.SIZES) * len(names) == 460
    for n in PC.SIZES:
        fam = PC.families(n)
        assert [name for name, _ in fam] == names
        assert all(z.shape == (n,) and z.dtype == np.float64 for _, z in fam)
        assert PC.families(n) is fam                                   # drawn once, shared


@pytest.mark.parametrize("n", PC.SIZES)
def test_families_meet_their_conditions(n):
    f = dict(PC.families(n))
    assert np.all(f["const"] == 0.25) and np.all(f["const_neg"] == -3.5)
    assert np.sum(f["one_high"] == 2.0) == 1 and np.sum(f["one_high"] == 1.0) == n - 1
    assert np.sum(f["one_low"] == -2.0) == 1 and np.sum(f["one_low"] == 1.0) == n - 1
    for which, tag, (lo, hi) in ((0, "lo", (0.0, 1.0)), (1, "hi", (1.0, 3.0))):
        ip = PC.ranks(n, PC.PCTS[which])[0]
        for d in PC.TIE_OFFSETS:
            s = np.sort(f[f"two_valued_{tag}{d:+d}"])
            assert set(np.unique(s)) <= {lo, hi}
            end = ip + d                                               # sorted index of the last `lo`
            if 0 <= end < n - 1:
                assert s[end] == lo and s[end + 1] == hi, (tag, d)
            else:                                                      # the run cannot end there: clamped to none or all
                assert np.all(s == (hi if end < 0 else lo))
            if n >= 1023:                                              # from here on every offset of both ranks is real
                assert 0 <= end < n - 1
    if n >= 200:
        assert (f["signs"] > 0).any() and (f["signs"] < 0).any()
        mag = np.log10(np.abs(f["signs"][f["signs"] != 0]))
        assert mag.max() - mag.min() > 500
        d = f["denormals"]
        assert (d > 0).any() and (d < 0).any() and np.all(np.abs(d) < 2.3e-308)
        z = f["zeros_pm"]
        assert (z == 0).sum() > n // 5 and np.signbit(z[z == 0]).any() and not np.signbit(z[z == 0]).all()
        assert set(np.unique(f["few_levels"])) == {0.0, 1.0, 2.0}
        u = np.unique(f["ulp_cluster"])
        assert u.size == 8 and np.all(np.diff(u) == 2.0 ** -52)
        assert np.isposinf(f["many_inf"]).sum() == n // 50 == np.isneginf(f["many_inf"]).sum()
        assert set(np.unique(f["huge"])) == {-1.7e308, 1e308, 1.7e308}
    if n >= 3:
        assert np.isposinf(f["one_inf_each"]).sum() <= 1 and np.isneginf(f["one_inf_each"]).sum() == 1
        assert np.all(np.diff(f["sorted"]) >= 0) and np.all(np.diff(f["reversed"]) <= 0)
    assert np.isnan(f["nan_last"][-1]) and not np.isnan(f["nan_last"][:-1]).any()
    for name, z in f.items():
        if name != "nan_last":
            assert not np.isnan(z).any(), name


@pytest.mark.parametrize("n", PC.SIZES)
def test_rank_arithmetic_equals_numpy_on_the_families(n):
    for name, z in PC.families(n):
        got, ref = PC.kernel_percentiles(z), PC.numpy_percentiles(z)
        assert PC.same_percentiles(name, got, ref), (name, n, got, ref)


def test_rank_arithmetic_equals_numpy_at_every_image_size():
    """n = C*R*R, C = 1..7, R = 1..128 in steps that keep the test quick, plus every R at C = 1"""
    rng = np.random.default_rng(PC.SEED)
    sizes = sorted({c * r * r for c in range(1, 8) for r in range(1, 129, 7)} | {r * r for r in range(1, 129)})
    for n in sizes:
        for kind in range(3):
            z = (rng.normal(0, 1, n), rng.uniform(0.1, 0.9, n), np.round(rng.normal(0, 3, n)))[kind]
            assert PC.same_percentiles("", PC.kernel_percentiles(z), PC.numpy_percentiles(z)), (n, kind)


def test_keys_order_as_the_values_do():
    z = np.array([-np.inf, -1.7e308, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1.7e308, np.inf])
    k = PC.keys(z)
    assert np.all(np.diff(k.astype(object)) > 0)
