"""CPU tier of tests/update_helpers.py: the matrix families of test_gpu_update_kernel.py meet their input conditions, and
numpy's own pseudo-inverse and solve, measured against the extended-precision references, are what the recorded
constants say -- the device's bars are 8 times those figures."""
import numpy as np
import pytest

import update_helpers as U


@pytest.mark.parametrize("G", range(3, 10))
def test_pinv_families_meet_their_input_conditions(G):
    cases = U.pinv_cases(G)
    names = [c["name"] for c in cases]
    assert len(names) == len(set(names)) == 22
    for c in cases:
        U.check_pinv_case_conditions(c)
        assert np.array_equal(U.product(c["cdd_inv"], c["means"]), c["target"]), c["name"]
        assert np.all(np.abs(c["means"]) <= 1.0)
    by = {c["name"]: c for c in cases}
    for name in ("dup_column", "dep_row", "zero_column", "clamped_one_pair"):
        assert by[name]["rank"] == G - 1, name
    assert by["zero"]["rank"] == 0 and by["random"]["rank"] == G
    assert 0.9e13 < by["graded_1e+13"]["kappa"] < 1.1e13


def test_numpy_stays_inside_the_bars_given_to_the_device():
    """measured here: 5.123 and 0.1262 (NUMPY_PINV_WORST, NUMPY_SOLVE_WORST); another LAPACK build may differ in the last
    bits, so the assertion is the device's own bar, not the figure"""
    worst_p, at_p = U.measure_numpy_pinv()
    worst_s, at_s = U.measure_numpy_solve()
    print(f"numpy pinv worst ratio {worst_p:.4f} at {at_p}; numpy solve worst ratio {worst_s:.4f} at {at_s}")
    assert worst_p <= U.C_PINV and worst_s <= U.C_SOLVE
    assert U.C_PINV == 8 * U.NUMPY_PINV_WORST and U.C_SOLVE == 8 * U.NUMPY_SOLVE_WORST


def test_solve_families():
    for G in range(3, 10):
        cases = U.solve_cases(G)
        by = {c["name"]: c for c in cases}
        assert by["zero_leading_pivot"]["vgm"][0, 0] == 0.0
        assert sum(c["singular"] for c in cases) == 1 and np.linalg.matrix_rank(by["singular"]["vgm"]) == G - 1
        p = by["permuted_diagonal"]["vgm"]
        assert ((p != 0).sum(axis=0) == 1).all() and ((p != 0).sum(axis=1) == 1).all() and not np.diag(p).any()
        assert 0.9e10 < by["graded_1e+10"]["kappa"] < 1.1e10
