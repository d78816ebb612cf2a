"""Probe scans and device-range maps, CPU tier: the tile plans against a literal loop restatement of the reference's
two scripts, the `env.array._get_obs` facade on a stub backend, and the argument checks of qd_probe / qd_probe_compose
that need no GPU."""
import ctypes
import os

import numpy as np
import pytest
import yaml

from qadapt_hip import device_map as M
from qadapt_hip import device_model as DM
from qadapt_hip.env import QuantumDeviceEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ tile plans
def _full_range_loops(plunger_min, plunger_max, obs_window_size):
    """map_full_device_range.py:66-122, restated statement by statement."""
    v0_range = plunger_max[0] - plunger_min[0]
    v1_range = plunger_max[1] - plunger_min[1]
    n_scans_x = int(np.ceil(v0_range / obs_window_size))
    n_scans_y = int(np.ceil(v1_range / obs_window_size))
    if n_scans_x > 1:
        step_x = v0_range / n_scans_x
    else:
        step_x = 0
    if n_scans_y > 1:
        step_y = v1_range / n_scans_y
    else:
        step_y = 0
    centres, positions = [], []
    for i in range(n_scans_x):
        for j in range(n_scans_y):
            center_v0 = plunger_min[0] + (i + 0.5) * step_x
            center_v1 = plunger_min[1] + (j + 0.5) * step_y
            scan_min_v0 = center_v0 - obs_window_size / 2
            scan_max_v0 = center_v0 + obs_window_size / 2
            scan_min_v1 = center_v1 - obs_window_size / 2
            scan_max_v1 = center_v1 + obs_window_size / 2
            centres.append((center_v0, center_v1))
            positions.append((scan_min_v0, scan_max_v0, scan_min_v1, scan_max_v1))
    return n_scans_x, n_scans_y, step_x, step_y, centres, positions


def _centred_loops(gt0, gt1, half_range, scan_window_size):
    """map_device_range.py:36-88, restated statement by statement (the script's 20 and 3.0 as arguments)."""
    v0_min = gt0 - half_range
    v0_max = gt0 + half_range
    v1_min = gt1 - half_range
    v1_max = gt1 + half_range
    v0_range = v0_max - v0_min
    v1_range = v1_max - v1_min
    n_scans_x = int(np.ceil(v0_range / scan_window_size))
    n_scans_y = int(np.ceil(v1_range / scan_window_size))
    step_x = scan_window_size
    step_y = scan_window_size
    centres, positions = [], []
    for i in range(n_scans_x):
        for j in range(n_scans_y):
            scan_min_v0 = v0_min + i * step_x
            scan_max_v0 = scan_min_v0 + scan_window_size
            scan_min_v1 = v1_min + j * step_y
            scan_max_v1 = scan_min_v1 + scan_window_size
            center_v0 = (scan_min_v0 + scan_max_v0) / 2
            center_v1 = (scan_min_v1 + scan_max_v1) / 2
            centres.append((center_v0, center_v1))
            positions.append((center_v0, center_v1, scan_min_v0, scan_max_v0, scan_min_v1, scan_max_v1))
    return (v0_min, v0_max, v1_min, v1_max), n_scans_x, n_scans_y, step_x, step_y, centres, positions


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("pmin,pmax,window,shape", [
    ((-43.7, -51.2), (41.9, 38.4), 3.4, None),                 # an 80-100 V range with a 3-4 V window: 26 x 27
    ((-10.0, -8.0), (6.0, 8.0), 4.0, (4, 4)),                  # ceil lands exactly on both axes
    ((0.0, -3.0), (12.0, 6.0), 3.0, (4, 3)),                   # exact again, different counts per axis
    ((1.25, -0.5), (3.0, 9.7), 3.7, (1, 3)),                   # a single scan on the x axis (step 0: it sits at the minimum)
    ((5.0, 5.0), (6.5, 7.0), 3.2, (1, 1)),                     # a single scan per axis
    ((-30.000001, 2.3), (17.77, 2.3 + 7 * 3.3), 3.3, None),    # ceil within rounding of an integer on the y axis
])
def test_full_range_plan_equals_the_scripts_loops(pmin, pmax, window, shape):
    pmin, pmax = np.array(pmin), np.array(pmax)
    nx, ny, sx, sy, centres, positions = _full_range_loops(pmin, pmax, window)
    plan = M.tile_plan_full_range(pmin, pmax, window)
    assert (plan["n_scans_x"], plan["n_scans_y"]) == (nx, ny)
    if shape is not None:
        assert (nx, ny) == shape
    assert _same_bits(plan["step_x"], sx) and _same_bits(plan["step_y"], sy)
    assert len(plan["positions"]) == nx * ny and plan["centres"].shape == (nx * ny, 2)
    assert _same_bits(plan["centres"], centres)
    assert _same_bits(plan["positions"], positions)
    # query order: scan (i, j) at i * ny + j
    i, j = nx - 1, ny // 2
    assert plan["centres"][i * ny + j, 0] == pmin[0] + (i + 0.5) * sx


@pytest.mark.parametrize("gt0,gt1,half,window,shape", [
    (3.172, -7.91, 20.0, 3.0, (14, 14)),                       # the script's own numbers: ceil(40 / 3) = 14
    (np.float32(11.3), np.float32(-2.6), 20.0, 3.0, None),     # float32 ground truths, as the info dict carries them
    (0.0, 0.0, 6.0, 3.0, (4, 4)),                              # ceil lands exactly
    (-14.4, 21.05, 1.5, 3.0, (1, 1)),                          # a single scan per axis
    (2.0, 5.0, 10.0, 3.7, None),
])
def test_centred_plan_equals_the_scripts_loops(gt0, gt1, half, window, shape):
    bounds, nx, ny, sx, sy, centres, positions = _centred_loops(gt0, gt1, half, window)
    plan = M.tile_plan_centred(gt0, gt1, half, window)
    assert (plan["n_scans_x"], plan["n_scans_y"]) == (nx, ny)
    if shape is not None:
        assert (nx, ny) == shape
    assert _same_bits([plan[k] for k in ("v0_min", "v0_max", "v1_min", "v1_max")], bounds)
    assert _same_bits(plan["step_x"], sx) and _same_bits(plan["step_y"], sy)
    assert _same_bits(plan["centres"], centres)
    assert _same_bits(plan["positions"], positions)
    # edge to edge: the first scan starts at the minimum and the last one covers the maximum
    assert plan["positions"][0][2] == bounds[0] and plan["positions"][-1][3] >= bounds[1]


def test_centred_plan_defaults_are_the_scripts():
    assert M.tile_plan_centred(1.0, 2.0)["positions"] == M.tile_plan_centred(1.0, 2.0, 20.0, 3.0)["positions"]
    assert M.tile_plan_centred(1.0, 2.0)["n_scans_x"] == 14


# ------------------------------------------------------------------ the array facade on a stub backend
class StubBackend:
    """Shape-faithful stand-in for VecQuantumDeviceEnv with B = 1 that records its probe calls."""

    def __init__(self, N, R):
        self.N, self.R = N, R
        self.probes = []

    def _obs(self):
        N, R = self.N, self.R
        return {"image": np.zeros((1, R, R, N - 1), np.float32), "obs_gate_voltages": np.zeros((1, N), np.float32),
                "obs_barrier_voltages": np.zeros((1, N - 1), np.float32)}

    def reset(self, seed=None, **kw):
        return self._obs()

    def step(self, actions):
        return self._obs(), np.zeros((1, 2 * self.N - 1)), np.array([False]), np.array([False])

    def device_state(self):
        N = self.N
        return {"gate_ground_truth": np.ones((1, N), np.float32), "barrier_ground_truth": np.zeros((1, N - 1), np.float32),
                "sensor_ground_truth": np.array([0.5]), "current_gate_voltages": np.full((1, N), 2.0),
                "current_barrier_voltages": np.full((1, N - 1), 3.0),
                "virtual_gate_matrix": -np.eye(N + 1)[None], "virtual_gate_origin": np.zeros((1, N + 1))}

    def probe(self, env_ids, gate_voltages, barrier_voltages, sensor_voltage=None, window=None, normalised=False):
        self.probes.append(dict(env_ids=env_ids, gate_voltages=np.array(gate_voltages), window=window,
                                barrier_voltages=np.array(barrier_voltages), sensor_voltage=sensor_voltage))
        N, R = self.N, self.R
        raw = np.arange((N - 1) * R * R, dtype=np.float64).reshape(1, N - 1, R, R)
        return {"raw": raw}


def _env(tmp_path, N=4, R=6):
    cfg = DM.load_yaml(None, "env_config.yaml")
    cfg["capacitance_model"]["update_method"] = None
    cfg["simulator"].update(num_dots=N, resolution=R)
    p = tmp_path / "env.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return QuantumDeviceEnv(config_path=str(p), backend=StubBackend(N, R))


def test_array_facade_surface_and_get_obs(tmp_path):
    N, R = 4, 6
    env = _env(tmp_path, N, R)
    a = env.array
    assert (a.num_dots, a.num_barrier_voltages, a.obs_image_size) == (N, N - 1, R)
    assert a.obs_voltage_min == -a.obs_voltage_max and a.obs_voltage_max > 0
    # what the env already exposed stays
    assert hasattr(a, "barrier_alpha") and hasattr(a.model, "cgd_full")
    assert np.array_equal(a.gate_ground_truth, np.ones(N, np.float32))
    a.obs_voltage_min, a.obs_voltage_max = -1.75, 1.75
    gates, barriers = np.array([1.0, 2.0, 3.0, 4.0]), [5.0, 6.0, 7.0]
    obs = a._get_obs(gates, barriers)
    assert set(obs) == {"image", "obs_gate_voltages", "obs_barrier_voltages"}
    assert obs["obs_gate_voltages"] is gates and obs["obs_barrier_voltages"] is barriers
    img = obs["image"]
    assert img.shape == (R, R, N - 1) and img.dtype == np.float64
    # channel c of the image is channel c of the probe's (C, R, R) signal, pixel for pixel
    assert img[2, 3, 1] == 1 * R * R + 2 * R + 3
    call = env._b.probes[-1]
    assert list(call["env_ids"]) == [0] and call["window"] == 1.75 and call["sensor_voltage"] is None
    assert call["gate_voltages"].shape == (1, N) and np.array_equal(call["gate_voltages"][0], gates)
    assert np.array_equal(call["barrier_voltages"][0], barriers)
    a._get_obs(gates, barriers, sensor_voltage=0.25)
    assert env._b.probes[-1]["sensor_voltage"] == 0.25
    # the probe is stateless for the wrapper too: no step was counted
    assert env.current_step == 0


def test_array_facade_keeps_the_reference_assertions(tmp_path):
    env = _env(tmp_path, 4, 6)
    a = env.array
    with pytest.raises(AssertionError, match="Incorrect gate voltage shape, expected 4, got 3"):
        a._get_obs(np.zeros(3), np.zeros(3))
    with pytest.raises(AssertionError, match="Incorrect barrier voltage shape, expected 3, got 4"):
        a._get_obs(np.zeros(4), np.zeros(4))
    with pytest.raises(AssertionError, match="Barrier voltages must be provided"):      # qarray_base_class.py:142
        a._get_obs(np.zeros(4))
    assert env._b.probes == []


def test_asymmetric_window_is_refused_by_name(tmp_path):
    env = _env(tmp_path, 4, 6)
    env.array.obs_voltage_min, env.array.obs_voltage_max = -3.0, 1.5               # qarray_base_class.py:1297-1298
    with pytest.raises(ValueError) as ei:
        env.array._get_obs(np.zeros(4), np.zeros(3))
    assert "-3.0" in str(ei.value) and "1.5" in str(ei.value) and env._b.probes == []


# ------------------------------------------------------------------ C ABI without a GPU
def _built_lib():
    from qadapt_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is missing: run __graft_entry__.build() before the tests (no test compiles it)")
    return _lib, _lib.lib()


def test_probe_symbols_and_prototypes():
    _lib, L = _built_lib()
    for name in ("qd_probe", "qd_probe_compose", "qd_time_select"):
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert len(L.qd_probe.argtypes) == 11 and L.qd_probe.argtypes[2] is ctypes.c_int
    assert len(L.qd_probe_compose.argtypes) == 9
    assert (_lib.QD_MAP_GLOBAL, _lib.QD_MAP_PER_SCAN) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "qdsim.h")).read()
    assert "#define QD_MAP_GLOBAL 0" in hdr and "#define QD_MAP_PER_SCAN 1" in hdr
    # a null handle is an argument error, not a crash
    assert L.qd_probe(None, None, 1, None, None, None, None, None, None, None, None) == _lib.QD_ERR_ARG
    assert L.qd_probe_compose(None, None, 1, 1, 0, 0, None, None, None) == _lib.QD_ERR_ARG


def test_probe_argument_checks_need_no_device():
    """QD_ERR_ARG cases are found before anything touches the device.  Without a GPU qd_create fails with QD_ERR_HIP and
    still hands out the partial handle (qdsim.h), which is all these checks need; with one it is a full handle."""
    _lib, L = _built_lib()
    from qadapt_hip.vec_env import make_qd_config
    cfg = make_qd_config(DM.load_yaml(None, "env_config.yaml"), DM.load_yaml(None, "qarray_config.yaml"), 4, 8, 2)
    h = ctypes.c_void_p()
    L.qd_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    if not h:
        pytest.fail("qd_create handed out no handle")
    try:
        one = ctypes.c_void_p(64)                  # never dereferenced: every call below returns before a launch
        args = lambda ids, nq, g, b: L.qd_probe(h, ids, nq, g, b, None, None, None, None, None, None)   # noqa: E731
        assert args(None, 1, one, one) == _lib.QD_ERR_ARG and b"env_of_query" in L.qd_last_error(h)
        assert args(one, 1, None, one) == _lib.QD_ERR_ARG and b"gate_v_dev" in L.qd_last_error(h)
        assert args(one, 1, one, None) == _lib.QD_ERR_ARG
        assert args(one, -1, one, one) == _lib.QD_ERR_ARG and b"nq < 0" in L.qd_last_error(h)
        assert args(one, 0, one, one) == 0                                     # nq == 0 does nothing
        comp = lambda raw, nx, ny, ch, mode, dst: L.qd_probe_compose(h, raw, nx, ny, ch, mode, dst, None, None)  # noqa: E731
        assert comp(None, 1, 1, 0, 0, one) == _lib.QD_ERR_ARG
        assert comp(one, 1, 1, 0, 0, None) == _lib.QD_ERR_ARG
        assert comp(one, 0, 1, 0, 0, one) == _lib.QD_ERR_ARG
        assert comp(one, 1, 1, 3, 0, one) == _lib.QD_ERR_ARG and b"channel" in L.qd_last_error(h)     # C = 3: channels 0..2
        assert comp(one, 1, 1, -1, 0, one) == _lib.QD_ERR_ARG
        assert comp(one, 1, 1, 0, 2, one) == _lib.QD_ERR_ARG and b"mode" in L.qd_last_error(h)
        assert comp(one, 256, 256, 0, 0, one) == _lib.QD_ERR_ARG                                      # > 65535 scans
        big = make_qd_config(DM.load_yaml(None, "env_config.yaml"), DM.load_yaml(None, "qarray_config.yaml"), 2, 257, 1)
        hb = ctypes.c_void_p()
        L.qd_create(ctypes.byref(big), 0, ctypes.byref(hb))
        if hb:                                                               # P = 257^2: 65535 scans hold >= 2^32 values
            try:
                rc = L.qd_probe_compose(hb, one, 255, 257, 0, 0, one, None, None)
                assert rc == _lib.QD_ERR_ARG and b"2^32" in L.qd_last_error(hb)
            finally:
                L.qd_destroy(hb)
    finally:
        L.qd_destroy(h)
