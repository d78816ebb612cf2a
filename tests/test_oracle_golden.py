"""Pin the oracle against fixtures produced by the reference's own importable
modules (tests/golden/make_golden.py): Kalman traces (a19) and sweep grids (a5)."""
import os

import numpy as np

import qd_oracle as O


def test_kalman_traces_match_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "kalman_traces.npz"))
    for c in range(int(g["n_cases"])):
        n = int(g[f"c{c}_n_dots"])
        k = O.KalmanOracle(n)
        values = g[f"c{c}_values"]; log_vars = g[f"c{c}_log_vars"]
        for t in range(values.shape[0]):
            k.update_from_cnn(values[t], log_vars[t])
            # same float64 operations in the same order -> bit-exact
            assert np.array_equal(k.means, g[f"c{c}_means"][t])
            assert np.array_equal(k.vars, g[f"c{c}_variances"][t])
            assert np.array_equal(k.full_matrix(), g[f"c{c}_full"][t])


def test_kalman_readme_example():
    # SURVEY §8c captured example
    k = O.KalmanOracle(4)
    k.update_from_scan(1, [(-0.05, -4.0), (0.02, -3.5), (0.01, -1.0)])
    m = k.full_matrix()
    assert abs(m[1, 2] - 0.25176684) < 1e-8
    assert abs(m[1, 3] - 0.1688609) < 1e-7
    assert m[0, 2] == 0.15


def test_sweep_grids_match_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "sweep_grids.npz"))
    for c in range(int(g["n_cases"])):
        R = int(g[f"c{c}_R"]); ch = int(g[f"c{c}_ch"]); w = float(g[f"c{c}_window"])
        vg = O.sweep_voltages(g[f"c{c}_vgm"], g[f"c{c}_origin"], g[f"c{c}_gate_voltages"],
                              float(g[f"c{c}_sensor"]), ch, -w, w, R)
        assert np.array_equal(vg, g[f"c{c}_vg_flat"])


def test_direct_and_nn_mode_updaters_match_reference(golden_dir):
    """update_method "direct" (DirectUpdater.py) and the legacy 2-output nearest_neighbour mode of both
    updaters, against traces of the reference classes themselves."""
    g = np.load(os.path.join(golden_dir, "updater_variants.npz"))
    for c in range(int(g["n_cases"])):
        n = int(g[f"c{c}_n_dots"]); kind = str(g[f"c{c}_kind"])
        values = g[f"c{c}_values"]; log_vars = g[f"c{c}_log_vars"]
        cls = O.DirectOracle if kind == "direct" else O.KalmanOracle
        k = cls(n, include_nnn=values.shape[-1] == 3)
        for t in range(values.shape[0]):
            k.update_from_cnn(values[t], log_vars[t])
            assert np.array_equal(k.means, g[f"c{c}_means"][t]), (c, t)
            assert np.array_equal(k.vars, g[f"c{c}_variances"][t]), (c, t)
            assert np.array_equal(k.full_matrix(), g[f"c{c}_full"][t]), (c, t)


def test_updaters_on_float32_inputs_match_reference(golden_dir):
    """Both updaters, n_dots 2..8, 3 and 2 outputs, on inputs that are float32 numbers (what the device is fed) and that
    cross both ends of the log-variance clamp, the acceptance gate and the +-1 mean clamp: traces of the reference
    classes themselves, with their accepted / rejected counters."""
    g = np.load(os.path.join(golden_dir, "updater_traces_f32.npz"))
    assert int(g["n_cases"]) == 7 * 2 * 2
    seen = set()
    for c in range(int(g["n_cases"])):
        n = int(g[f"c{c}_n_dots"]); kind = str(g[f"c{c}_kind"])
        values = g[f"c{c}_values"]; log_vars = g[f"c{c}_log_vars"]
        assert values.dtype == np.float32 and log_vars.dtype == np.float32 and values.shape[0] == 8
        seen.add((n, kind, values.shape[-1]))
        cls = O.DirectOracle if kind == "direct" else O.KalmanOracle
        k = cls(n, include_nnn=values.shape[-1] == 3)
        count = [0, 0]
        inner = k._update

        def counted(i, j, delta, R, inner=inner, count=count):
            ok = inner(i, j, delta, R)
            count[0 if ok else 1] += 1
            return ok
        k._update = counted
        for t in range(values.shape[0]):
            k.update_from_cnn(values[t], log_vars[t])
            assert np.array_equal(k.means, g[f"c{c}_means"][t]), (c, t)
            assert np.array_equal(k.vars, g[f"c{c}_variances"][t]), (c, t)
            assert np.array_equal(k.full_matrix(), g[f"c{c}_full"][t]), (c, t)
            assert count == [int(g[f"c{c}_accepted"][t]), int(g[f"c{c}_rejected"][t])], (c, t)
        # what the fixture is for: every case gates both ways, clamps a mean and has log-variances beyond both clamp ends
        assert count[0] > 0 and count[1] > 0, c
        assert (np.abs(g[f"c{c}_means"]) == 1.0).any(), c
        assert (log_vars < -6).any() and (log_vars > 2).any(), c
    assert seen == {(n, kind, o) for n in range(2, 9) for kind in ("kalman", "direct") for o in (3, 2)}
