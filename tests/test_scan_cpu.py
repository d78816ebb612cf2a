"""Axis scans (qd_scan2d), CPU tier: the scan front end (csrc/qd_pixel.h: qd_scan_voltages, compiled for the host in
tests/hosttest_scan) against qd_pixel_voltages bit for bit on adjacent virtual plungers, against qd_point_front in the
physical frame, and against the reference composer's grids (tests/golden/axis_grids.npz); the argument checks, prototype
and export of qd_scan2d; the control names of scan2d and the `_get_charge_sensor_data` mirror on a stub backend.
No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import yaml

import helpers as H
import points_helpers as PH
import scan_helpers as SH
from qadapt_hip import device_model as DM
from qadapt_hip.env import QuantumDeviceEnv
from qadapt_hip.layout import layout

ROOT = H.ROOT
EPS = np.finfo(np.float64).eps


def _scene(N, seed, mode="mid"):
    eb = H.sample_blocks(N, [seed])
    rng = np.random.default_rng(seed)
    return eb.params[0], H.place(N, eb.state[0], mode, rng), rng


# ------------------------------------------------------------------ adjacent virtual plungers = the env's front end
@pytest.mark.parametrize("N", [2, 3, 4, 5, 6, 7, 8])
def test_adjacent_axes_reproduce_qd_pixel_voltages_bit_for_bit(N):
    """Every channel c, R in {1, 2, 8, 12}, axes (c, c+1), ranges fl(v + (-w)), fl(v + w): v_ext, vpp and tc of every pixel
    have the bits of qd_pixel_voltages.  The env's own window and one unlike it."""
    L = layout(N)
    par, st, rng = _scene(N, 500 + N)
    st[L.s_sensor_gt] = rng.uniform(-1, 1)
    for w in (float(par[L.scal + 2]), 0.37 * float(par[L.scal + 2])):
        p2 = par.copy(); p2[L.scal + 2] = w
        for R in (1, 2, 8, 12):
            for c in range(N - 1):
                ref = SH.pixel_voltages(N, p2, st, c, R)
                rg = SH.adjacent_ranges(st[L.s_gate_v:L.s_gate_v + N], c, w)
                got = SH.scan_voltages(N, par, st, c, c + 1, rg, R)
                for name, a, b in zip(("v_ext", "vpp", "tc"), got, ref):
                    assert PH.same(a, b), (name, R, c)


def test_peak_width_pair_is_qd_peak_width_on_adjacent_plungers():
    for N in (2, 4, 8):
        L = layout(N)
        par, st, rng = _scene(N, 520 + N)
        for a in (-1.0, 0.0, 0.01, 0.05):
            p2 = par.copy(); p2[L.scal + 3] = a
            for c in range(N - 1):
                w = SH.peak_width(N, p2, st, c)
                assert SH.peak_width_pair(N, p2, st, c, c + 1) == w and SH.peak_width_pair(N, p2, st, c + 1, c) == w
            if N > 2 and a > 0:
                v = st[L.s_gate_v:L.s_gate_v + N]
                want = min(max(p2[L.scal + 1] - abs(a * (abs(v[0]) + abs(v[N - 1])) / 2.0), 0.0), 1.0)
                assert SH.peak_width_pair(N, p2, st, 0, N - 1) == want


# ------------------------------------------------------------------ physical frame = the point front end
def _general_cases(N):
    cases = [(0, N - 1), (N - 1, 0), (0, N), (N, 1), (0, N + 1), (2 * N - 1, 1)]
    if N >= 3:
        cases += [(N + 1, 2 * N - 1), (2, 0), (N + 2, N)]
    return cases


@pytest.mark.parametrize("N", [2, 4, 8])
def test_physical_frame_is_the_point_front_end(N):
    """v_ext has the bits of W (the query's voltages with the two linspaces on the swept controls: no matrix, no origin);
    vpp and tc have the bits of qd_point_front at that v_ext.  Every kind of control as an axis."""
    L = layout(N)
    par, st, rng = _scene(N, 540 + N)
    st[L.s_sensor_gt] = rng.uniform(-1, 1)
    for R in (5, 8):
        for ax, ay in _general_cases(N):
            rg = np.array([-3.25, 7.5, 11.0, -2.0]) + rng.uniform(-1, 1, 4)
            v_ext, vpp, tc = SH.scan_voltages(N, par, st, ax, ay, rg, R, SH.PHYSICAL)
            W = SH.numpy_grid(N, st, None, ax, ay, rg, R, SH.PHYSICAL).reshape(R * R, 2 * N)
            keep = [i for i in range(2 * N) if i not in (ax, ay)]
            assert PH.same(v_ext[:, keep], W[:, keep])
            for axis, lo, hi, along in ((ax, rg[0], rg[1], "x"), (ay, rg[2], rg[3], "y")):
                line = np.array([lo + i * ((hi - lo) / (R - 1)) for i in range(R - 1)] + [hi])     # qd_linspace
                grid = v_ext[:, axis].reshape(R, R)
                assert PH.same(grid, np.broadcast_to(line[None, :] if along == "x" else line[:, None], (R, R)))
            pv, pt = SH.point_front(N, par, v_ext)
            assert PH.same(vpp, pv) and PH.same(tc, pt), (R, ax, ay)


@pytest.mark.parametrize("N", [2, 4, 8])
def test_virtual_frame_on_any_axes_matches_numpy(N):
    """Virtual frame, every kind of control as an axis: the gate part within the dot-product bound of the NumPy grid, the
    barrier part bit-equal to W; x along columns; x_lo == x_hi repeats one column."""
    L = layout(N); G = N + 1
    par, st, rng = _scene(N, 560 + N)
    st[L.s_sensor_gt] = rng.uniform(-1, 1)
    origin = par[L.origin:L.origin + G]
    vgm = st[L.s_vgm:L.s_vgm + G * G].reshape(G, G)
    R = 8
    for ax, ay in _general_cases(N):
        rg = np.array([-3.25, 7.5, 11.0, -2.0]) + rng.uniform(-1, 1, 4)
        v_ext, _, _ = SH.scan_voltages(N, par, st, ax, ay, rg, R)
        want = SH.numpy_grid(N, st, origin, ax, ay, rg, R).reshape(R * R, 2 * N)
        Wg = SH.numpy_grid(N, st, None, ax, ay, rg, R, SH.PHYSICAL).reshape(R * R, 2 * N)
        bound = (G + 1) * EPS * (np.abs(Wg[:, :G]) @ np.abs(vgm).T + np.abs(origin))
        assert np.all(np.abs(v_ext[:, :G] - want[:, :G]) <= bound)
        assert PH.same(v_ext[:, G:], Wg[:, G:])
        flat = rg.copy(); flat[1] = flat[0]
        v1, vpp1, tc1 = SH.scan_voltages(N, par, st, ax, ay, flat, R)
        for a in (v1, vpp1, tc1):
            a = a.reshape(R, R, -1)
            assert PH.same(a, np.broadcast_to(a[:, :1], a.shape))


# ------------------------------------------------------------------ the reference composer's grids
def test_golden_axis_grids():
    """GateVoltageComposer.do2d(..., gate_voltages, True) of the reference on non-adjacent and reversed pairs, asymmetric
    and reversed ranges, N in {2, 4, 8}, R in {5, 8}: the gate part of v_ext within (G+1) eps (|VGM| |W| + |origin|) per
    element, with the SAME orientation (x along columns)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "axis_grids.npz"))
    n = int(z["n_cases"])
    seen_N, seen_R, kinds = set(), set(), set()
    for c in range(n):
        g = lambda k: z[f"c{c}_{k}"]     # noqa: E731
        N, R, xd, yd = int(g("n_dot")), int(g("R")), int(g("x_dot")), int(g("y_dot"))
        L = layout(N); G = N + 1
        seen_N.add(N); seen_R.add(R)
        rg = g("ranges")
        kinds |= {"nonadjacent"} if abs(xd - yd) > 1 else set()
        kinds |= {"reversed_pair"} if xd > yd else set()
        kinds |= {"reversed_range"} if rg[0] > rg[1] else set()
        kinds |= {"asymmetric"} if abs((rg[0] + rg[1]) / 2 - g("gate_voltages")[xd - 1]) > 1e-9 else set()
        par = np.zeros(L.size); st = np.zeros(L.s_size)
        par[L.origin:L.origin + G] = g("origin")
        st = SH.query_state(N, st, g("gate_voltages"), np.zeros(N - 1), float(g("sensor")), g("vgm"))
        v_ext, _, _ = SH.scan_voltages(N, par, st, xd - 1, yd - 1, rg, R)
        got = v_ext[:, :G].reshape(R, R, G)
        ref = g("vg")
        W = SH.numpy_grid(N, st, None, xd - 1, yd - 1, rg, R, SH.PHYSICAL)[:, :, :G]
        bound = (G + 1) * EPS * (np.abs(W) @ np.abs(g("vgm")).T + np.abs(g("origin")))
        assert np.all(np.abs(got - ref) <= bound), (c, float(np.abs(got - ref).max()))
        # orientation: the transposed grid is NOT within the bound (the two sweeps differ)
        assert not np.all(np.abs(got.transpose(1, 0, 2) - ref) <= bound), c
    assert seen_N == {2, 4, 8} and seen_R == {5, 8}
    assert kinds == {"nonadjacent", "reversed_pair", "reversed_range", "asymmetric"}


# ------------------------------------------------------------------ C ABI without a GPU
def _built_lib():
    from qadapt_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is missing: run __graft_entry__.build() before the tests (no test compiles it)")
    return _lib, _lib.lib()


def test_scan2d_symbol_and_prototype():
    _lib, L = _built_lib()
    assert "qd_scan2d" in _lib.EXPORTS_WITH_DIGITS and hasattr(L, "qd_scan2d")
    at = L.qd_scan2d.argtypes
    assert len(at) == 13 and at[2] is ctypes.c_int and L.qd_scan2d.restype is ctypes.c_int
    assert at[11]._type_ is _lib.QdScanOpts and ctypes.sizeof(_lib.QdScanOpts) == 56
    hdr = open(os.path.join(ROOT, "include", "qdsim.h")).read()
    assert "int qd_scan2d(qd_handle* h, const int32_t* env_of_query_dev, int nq, const int32_t* axes_dev," in hdr
    assert f"#define QD_SCAN_VIRTUAL {_lib.QD_SCAN_VIRTUAL}" in hdr and f"#define QD_SCAN_PHYSICAL {_lib.QD_SCAN_PHYSICAL}" in hdr
    assert L.qd_scan2d(None, None, 1, None, None, None, None, None, None, None, None, None, None) == _lib.QD_ERR_ARG   # no crash


def _handle(L, N, R, B, flags=0, qconfig=None):
    from qadapt_hip.vec_env import make_qd_config
    cfg = make_qd_config(DM.load_yaml(None, "env_config.yaml"), qconfig or DM.load_yaml(None, "qarray_config.yaml"), N, R, B,
                         flags=flags)
    h = ctypes.c_void_p()
    L.qd_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    if not h:
        pytest.fail("qd_create handed out no handle")
    return h


def test_scan2d_argument_checks_need_no_device():
    """Without a GPU qd_create fails with QD_ERR_HIP and still hands out the partial handle (qdsim.h), which is all these
    checks need: each returns before anything touches the device."""
    _lib, L = _built_lib()
    B = 3
    h = _handle(L, 4, 8, B)
    one = ctypes.c_void_p(64)                      # a device pointer that is never dereferenced

    def opts(**kw):
        o = _lib.QdScanOpts(struct_size=ctypes.sizeof(_lib.QdScanOpts))
        for k, v in kw.items():
            setattr(o, k, v)
        return ctypes.byref(o)

    def call(hh=h, env=one, nq=1, axes=one, rng=one, gv=one, bv=one, o=None):
        return L.qd_scan2d(hh, env, nq, axes, rng, gv, bv, None, one, None, None, o, None)

    try:
        assert call(env=None) == _lib.QD_ERR_ARG and b"env_of_query_dev" in L.qd_last_error(h)
        assert call(axes=None) == _lib.QD_ERR_ARG and call(rng=None) == _lib.QD_ERR_ARG
        assert call(gv=None) == _lib.QD_ERR_ARG and b"gate_v_dev" in L.qd_last_error(h)
        assert call(bv=None) == _lib.QD_ERR_ARG
        assert call(nq=-1) == _lib.QD_ERR_ARG and b"nq < 0" in L.qd_last_error(h)
        assert call(o=opts(struct_size=8)) == _lib.QD_ERR_ARG and b"struct_size" in L.qd_last_error(h)
        assert call(o=opts(frame=2)) == _lib.QD_ERR_ARG and b"frame" in L.qd_last_error(h)
        assert call(o=opts(frame=-1)) == _lib.QD_ERR_ARG
        assert call(o=opts(frame=_lib.QD_SCAN_PHYSICAL, vgm_dev=64)) == _lib.QD_ERR_ARG and b"vgm_dev" in L.qd_last_error(h)
        assert call(o=opts(noise_flags=_lib.QD_NOISE_RADIAL)) == _lib.QD_ERR_ARG and b"radial" in L.qd_last_error(h)
        assert call(o=opts(noise_flags=_lib.QD_NOISE_SENSOR | _lib.QD_NOISE_RADIAL)) == _lib.QD_ERR_ARG
        assert call(o=opts(noise_flags=8)) == _lib.QD_ERR_ARG
        assert call(nq=0) == 0 and call(nq=0, o=opts(noise_flags=_lib.QD_NOISE_SENSOR | _lib.QD_NOISE_LATCH)) == 0
    finally:
        L.qd_destroy(h)
    hv = _handle(L, 4, 8, B, flags=_lib.QD_FLAG_VALIDATE)
    try:
        assert call(hh=hv) == _lib.QD_ERR_STATE and b"QD_FLAG_VALIDATE" in L.qd_last_error(hv)
        assert call(hh=hv, axes=None) == _lib.QD_ERR_ARG                 # the argument checks come first
    finally:
        L.qd_destroy(hv)
    from qadapt_hip.vec_env import override_charge_states
    q = override_charge_states(DM.load_yaml(None, "qarray_config.yaml"), "all")
    q["simulator"]["model"]["max_charge_carriers"] = 2
    hf = _handle(L, 3, 8, B, qconfig=q)
    try:
        assert call(hh=hf) == _lib.QD_ERR_STATE and b"full charge-state space" in L.qd_last_error(hf)
    finally:
        L.qd_destroy(hf)


# ------------------------------------------------------------------ control names
def test_control_names():
    from qadapt_hip.vec_env import scan_control_index as idx, scan_control_indices as idxs
    N = 4
    assert [idx(f"vP{k}", N) for k in range(1, N + 1)] == [0, 1, 2, 3]
    assert [idx(f"P{k}", N, "physical") for k in range(1, N + 1)] == [0, 1, 2, 3]
    assert idx("S", N) == N and idx("S", N, "physical") == N
    assert [idx(f"B{k}", N) for k in range(1, N)] == [N + 1, N + 2, N + 3]
    assert idx(0, N) == 0 and idx(np.int64(2 * N - 1), N) == 2 * N - 1
    for bad in ("vP0", "vP5", "B4", "B0", "Q1", "vP", "", "e1_2"):
        with pytest.raises(ValueError):
            idx(bad, N)
    with pytest.raises(ValueError, match="physical frame"):
        idx("P1", N, "virtual")
    with pytest.raises(ValueError, match="virtual frame"):
        idx("vP1", N, "physical")
    for bad in (-1, 2 * N):
        with pytest.raises(ValueError):
            idx(bad, N)
    with pytest.raises(TypeError):
        idx(1.5, N)
    assert idxs("B2", N, "virtual", 3).tolist() == [N + 2] * 3 and idxs("B2", N, "virtual", 3).dtype == np.int32
    assert idxs(["vP1", 5, "S"], N, "virtual", 3).tolist() == [0, 5, N]
    with pytest.raises(ValueError):
        idxs(["vP1", "vP2"], N, "virtual", 3)


# ------------------------------------------------------------------ the array facade on a stub backend
class StubBackend:
    """Shape-faithful stand-in for VecQuantumDeviceEnv with B = 1 that records its scan2d calls."""

    def __init__(self, N, R):
        self.N, self.R = N, R
        self.calls = []

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

    def scan2d(self, env_ids, x, y, x_range, y_range, gate_voltages, barrier_voltages, sensor_voltage=None, **kw):
        self.calls.append(dict(env_ids=list(env_ids), x=x, y=y, x_range=tuple(x_range), y_range=tuple(y_range),
                               gv=np.array(gate_voltages), bv=np.array(barrier_voltages), sv=sensor_voltage, kw=kw))
        R = self.R
        out = {"raw": np.arange(R * R, dtype=np.float64).reshape(1, R, R)}
        if kw.get("occupations"):
            out["occupations"] = np.zeros((1, R, R, self.N))
        return out


def _env(tmp_path, N=4, R=6):
    cfg = DM.load_yaml(None, "env_config.yaml")
    cfg["capacitance_model"]["update_method"] = None
    cfg["simulator"].update(num_dots=N, resolution=R)
    p = tmp_path / "env.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return QuantumDeviceEnv(config_path=str(p), backend=StubBackend(N, R))


def test_get_charge_sensor_data_mirror(tmp_path):
    N, R = 4, 6
    env = _env(tmp_path, N, R)
    arr = env.array
    arr.obs_voltage_min, arr.obs_voltage_max = -1.5, 2.5               # (an asymmetric window is fine for one image)
    gv, bv = np.array([1.0, -2.0, 3.0, 4.5]), np.array([0.1, 0.2, 0.3])
    z = arr._get_charge_sensor_data(1, 3, gv, bv)
    assert isinstance(z, np.ndarray) and z.shape == (R, R) and z.dtype == np.float64
    c = env._b.calls[-1]
    assert (c["x"], c["y"]) == (0, 2) and c["env_ids"] == [0] and c["sv"] is None
    assert c["x_range"] == (1.0 - 1.5, 1.0 + 2.5) and c["y_range"] == (3.0 - 1.5, 3.0 + 2.5)
    assert c["gv"].shape == (1, N) and c["bv"].shape == (1, N - 1) and np.array_equal(c["gv"][0], gv)
    arr._get_charge_sensor_data(4, 2, gv, bv, 0.25)                     # a reversed pair, with a sensor voltage
    c = env._b.calls[-1]
    assert (c["x"], c["y"], c["sv"]) == (3, 1, 0.25)
    arr._get_charge_sensor_data(N + 1, 2, gv, bv, 0.25)                 # the sensor gate sweeps around its own voltage
    c = env._b.calls[-1]
    assert c["x"] == N and c["x_range"] == (0.25 - 1.5, 0.25 + 2.5)
    n = len(env._b.calls)
    for g1, g2 in ((1, 1), (0, 2), (1, N + 2)):
        with pytest.raises(ValueError):
            arr._get_charge_sensor_data(g1, g2, gv, bv)
    with pytest.raises(AssertionError):
        arr._get_charge_sensor_data(1, 2, gv[:3], bv)
    with pytest.raises(AssertionError, match="Barrier voltages must be provided"):
        arr._get_charge_sensor_data(1, 2, gv, None)
    assert len(env._b.calls) == n and env.current_step == 0
    out = arr.scan2d("vP1", "B2", (-1, 1), (2, 0), gv, bv, occupations=True, frame="virtual")
    assert out["raw"].shape == (R, R) and out["occupations"].shape == (R, R, N)
    assert env._b.calls[-1]["kw"] == {"occupations": True, "frame": "virtual"} and env._b.calls[-1]["x"] == "vP1"
