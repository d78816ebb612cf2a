"""Affine axis scans (qd_scan_affine), CPU tier: the affine front end (csrc/qd_pixel.h: qd_affine_voltages, compiled for the
host in tests/hosttest_affine) against qd_scan_voltages bit for bit on unit directions, against the reference composer's
combination-axis grids (tests/golden/affine_grids.npz) and against NumPy in the physical frame; the axis resolver
scan_axis_vector; the argument checks, prototype and export of qd_scan_affine; the `env.array.scan_affine` mirror on a stub
backend.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import yaml

import affine_helpers as AH
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
    par, st = eb.params[0], H.place(N, eb.state[0], mode, rng)
    st[layout(N).s_sensor_gt] = rng.uniform(-1, 1)
    return par, st, rng


# ------------------------------------------------------------------ unit directions = the scan front end
def _unit_cases(N):
    """plunger, sensor and barrier axes, in both orders"""
    cases = [(0, N - 1), (N - 1, 0), (0, N), (N, 1), (0, N + 1), (2 * N - 1, 1)]
    if N >= 3:
        cases += [(N + 1, 2 * N - 1), (N + 2, N)]
    return cases


@pytest.mark.parametrize("N", [2, 4, 8])
def test_unit_directions_reproduce_qd_scan_voltages_bit_for_bit(N):
    """dx = e_ax, dy = e_ay and a base point with 0 at those two controls: v_ext, vpp and tc of every pixel have the bits of
    qd_scan_voltages(ax, ay) -- both frames, plunger, sensor and barrier axes, a reversed range, R in {5, 8}."""
    L = layout(N)
    par, st, rng = _scene(N, 700 + N)
    for frame in (SH.VIRTUAL, SH.PHYSICAL):
        for R in (5, 8):
            for ax, ay in _unit_cases(N):
                rg = np.array([-3.25, 7.5, 11.0, -2.0]) + rng.uniform(-1, 1, 4)         # y sweeps downwards
                ref = SH.scan_voltages(N, par, st, ax, ay, rg, R, frame)
                W0 = AH.base_point(N, st)
                W0[[ax, ay]] = 0.0
                st0 = SH.query_state(N, st, W0[:N], W0[N + 1:], W0[N])
                got = AH.affine_voltages(N, par, st0, AH.unit(N, ax), AH.unit(N, ay), rg, R, frame)
                for name, a, b in zip(("v_ext", "vpp", "tc"), got, ref):
                    assert np.isfinite(b).all()
                    assert PH.same(a, b), (name, frame, R, ax, ay)


# ------------------------------------------------------------------ the reference composer's combination axes
def test_golden_affine_grids():
    """GateVoltageComposer.do2d(x, ..., y, ...) of the reference on e x U, e x vP and U x vP pairs (non-adjacent and reversed
    dot pairs, asymmetric and reversed ranges, N in {2, 4, 8}, R in {5, 8}).  The composer holds the other gates at 0 and
    adds its origin once per vP axis, sqrt(2) times per U axis and never per e axis; the front end adds it once, so the
    surplus (multiplicity - 1) origin is taken off the reference.  Gate part of v_ext within (G+1) eps (|VGM| |W| + |origin|)
    per element (the bound of test_golden_axis_grids), same orientation (x along columns)."""
    from qadapt_hip.vec_env import scan_axis_vector
    z = np.load(os.path.join(ROOT, "tests", "golden", "affine_grids.npz"))
    n = int(z["n_cases"])
    seen_N, seen_R, kinds = set(), set(), set()
    for c in range(n):
        g = lambda k: z[f"c{c}_{k}"]     # noqa: E731
        N, R, xa, ya = int(g("n_dot")), int(g("R")), str(g("x_axis")), str(g("y_axis"))
        L = layout(N); G = N + 1
        seen_N.add(N); seen_R.add(R)
        rg = g("ranges")
        pair = tuple(sorted((xa[0], ya[0])))
        kinds.add({("U", "e"): "e_x_U", ("e", "v"): "e_x_vP", ("U", "v"): "U_x_vP"}[pair])
        for a in (xa, ya):
            if a[0] in "eU":
                i, j = (int(t) for t in a[1:].split("_"))
                kinds |= {"nonadjacent"} if abs(i - j) > 1 else set()
                kinds |= {"reversed_pair"} if i > j else set()
        kinds |= {"reversed_range"} if rg[0] > rg[1] else set()
        kinds |= {"asymmetric"} if abs(rg[0] + rg[1]) > 1e-9 else set()
        mult = float(g("origin_multiplicity"))
        want_mult = sum({"e": 0.0, "U": np.sqrt(2.0), "v": 1.0}[a[0]] for a in (xa, ya))
        assert mult == want_mult
        par = np.zeros(L.size); st = np.zeros(L.s_size)
        par[L.origin:L.origin + G] = g("origin")
        st = SH.query_state(N, st, np.zeros(N), np.zeros(N - 1), 0.0, g("vgm"))
        dx, dy = scan_axis_vector(xa, N), scan_axis_vector(ya, N)
        v_ext, _, _ = AH.affine_voltages(N, par, st, dx, dy, rg, R)
        got = v_ext[:, :G].reshape(R, R, G)
        ref = g("vg") - (mult - 1.0) * g("origin")
        W = AH.numpy_w(np.zeros(2 * N), dx, dy, rg, R)[:, :, :G]
        bound = (G + 1) * EPS * (np.abs(W) @ np.abs(g("vgm")).T + np.abs(g("origin")))
        worst = float((np.abs(got - ref) / bound).max())
        print(f"[golden affine] case {c} N={N} R={R} {xa} x {ya}: worst |diff| / bound {worst:.3f}")
        assert np.all(np.abs(got - ref) <= bound), (c, worst)
        # orientation: the transposed grid is NOT within the bound (the two sweeps differ)
        assert not np.all(np.abs(got.transpose(1, 0, 2) - ref) <= bound), c
        assert PH.same(v_ext[:, G:], np.zeros((R * R, N - 1)))
    assert seen_N == {2, 4, 8} and seen_R == {5, 8}
    assert kinds == {"e_x_U", "e_x_vP", "U_x_vP", "nonadjacent", "reversed_pair", "reversed_range", "asymmetric"}


# ------------------------------------------------------------------ dense directions, physical frame
@pytest.mark.parametrize("N", [2, 4, 8])
def test_physical_frame_dense_directions_match_numpy(N):
    """v_ext = W in the physical frame, W[i] = fma(sy, dy[i], fma(sx, dx[i], W0[i])) against NumPy's W0 + sx dx + sy dy.
    Tolerance from the operation count: the front end rounds twice (two fmas), NumPy four times (two products, two sums),
    each by at most eps / 2 of a partial sum bounded by S = |W0| + |sx dx| + |sy dy| -- 3 eps S; sx and sy themselves are
    start + i * step on both sides with the same three roundings (difference, quotient, product-sum), so they may differ
    by at most 3 eps (|lo| + |hi|) each.  With |sx| <= max(|lo|, |hi|) the bound used is
    6 eps (|W0| + (|x_lo| + |x_hi|) |dx| + (|y_lo| + |y_hi|) |dy|) per element.  vpp and tc have the bits of qd_point_front at
    that v_ext."""
    par, st, rng = _scene(N, 740 + N)
    for R in (5, 8):
        for k in range(4):
            dx, dy = rng.normal(0, 1, 2 * N), rng.normal(0, 1, 2 * N)
            rg = np.array([-3.25, 7.5, 11.0, -2.0]) + rng.uniform(-1, 1, 4)
            v_ext, vpp, tc = AH.affine_voltages(N, par, st, dx, dy, rg, R, AH.PHYSICAL)
            want = AH.numpy_grid(N, st, None, dx, dy, rg, R, AH.PHYSICAL).reshape(R * R, 2 * N)
            tol = 6 * EPS * (np.abs(AH.base_point(N, st)) + (abs(rg[0]) + abs(rg[1])) * np.abs(dx) + (abs(rg[2]) + abs(rg[3])) * np.abs(dy))
            assert np.all(np.abs(v_ext - want) <= tol), (R, k, float((np.abs(v_ext - want) / tol).max()))
            assert np.ptp(v_ext, axis=0).min() > 0                    # every control moves
            pv, pt = SH.point_front(N, par, v_ext)
            assert PH.same(vpp, pv) and PH.same(tc, pt), (R, k)


# ------------------------------------------------------------------ the axis resolver
def test_scan_axis_vector():
    from qadapt_hip.vec_env import scan_axis_vector as vec, scan_axis_vectors as vecs, scan_control_index
    N = 4
    r2 = 1.0 / np.sqrt(2.0)
    assert vec("e1_2", N).tolist() == [1, -1, 0, 0, 0, 0, 0, 0]
    assert vec("e4_1", N).tolist() == [-1, 0, 0, 1, 0, 0, 0, 0]
    assert vec("U1_3", N).tolist() == [r2, 0, r2, 0, 0, 0, 0, 0] and vec("U3_1", N).tolist() == vec("U1_3", N).tolist()
    assert vec("e1_2", N, "physical").tolist() == vec("e1_2", N).tolist()
    assert vec("vP2", N).tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and vec("P2", N, "physical").tolist() == vec("vP2", N).tolist()
    assert vec("S", N).tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and vec("B3", N).tolist() == [0] * 7 + [1]
    assert vec(5, N).tolist() == [0, 0, 0, 0, 0, 1, 0, 0] and vec(np.int64(0), N)[0] == 1.0
    assert vec({"vP1": 1.0, "B1": -0.25, 4: 0.5}, N).tolist() == [1, 0, 0, 0, 0.5, -0.25, 0, 0]
    assert vec({"vP1": 1.0, 0: 0.5}, N)[0] == 1.5
    v = np.arange(8.0)
    assert vec(v, N).tolist() == v.tolist() and vec(list(v), N).dtype == np.float64 and vec(v, N) is not v
    assert vec(np.zeros(8), N).tolist() == [0.0] * 8                        # the zero vector is legal
    with pytest.raises(ValueError, match="physical frame"):
        vec("P1", N, "virtual")
    with pytest.raises(ValueError, match="virtual frame"):
        vec({"vP1": 1.0}, N, "physical")
    for bad in ("e1_1", "U3_3"):
        with pytest.raises(ValueError, match="two different dots"):
            vec(bad, N)
    for bad in ("e0_1", "e1_5", "U5_1", "U1_0"):
        with pytest.raises(ValueError, match="1..4"):
            vec(bad, N)
    for bad in ("e1", "e1_2_3", "u1_2", "E1_2", "Q1", "vP9", "", "e1_-2"):
        with pytest.raises(ValueError):
            vec(bad, N)
    for bad in (np.zeros(7), np.zeros((2, 8)), [1.0, 2.0]):
        with pytest.raises(ValueError):
            vec(bad, N)
    with pytest.raises(TypeError):
        vec({1.5: 1.0}, N)
    # scan_control_index still refuses the combination names (scan2d is unchanged)
    with pytest.raises(ValueError):
        scan_control_index("e1_2", N)
    # per query
    assert vecs("e1_2", N, "virtual", 3).shape == (3, 8) and np.all(vecs("e1_2", N, "virtual", 3) == vec("e1_2", N))
    per = vecs(["e1_2", {"B1": 2.0}, v], N, "virtual", 3)
    assert per[0].tolist() == vec("e1_2", N).tolist() and per[1, N + 1] == 2.0 and per[2].tolist() == v.tolist()
    assert vecs(v, N, "virtual", 2).tolist() == [v.tolist()] * 2
    m = np.arange(16.0).reshape(2, 8)
    assert vecs(m, N, "virtual", 2).tolist() == m.tolist()
    with pytest.raises(ValueError):
        vecs(["e1_2", "U1_2"], N, "virtual", 3)
    with pytest.raises(ValueError):
        vecs(m, N, "virtual", 3)


# ------------------------------------------------------------------ C ABI without a GPU
def _built_lib():
    from qadapt_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is missing: run __graft_entry__.build() before the tests (no test compiles it)")
    return _lib, _lib.lib()


def test_scan_affine_symbol_and_prototype():
    _lib, L = _built_lib()
    assert "qd_scan_affine" in _lib.EXPORTS and hasattr(L, "qd_scan_affine")
    at = L.qd_scan_affine.argtypes
    assert len(at) == 13 and at[2] is ctypes.c_int and L.qd_scan_affine.restype is ctypes.c_int
    assert at[11]._type_ is _lib.QdScanAffineOpts and ctypes.sizeof(_lib.QdScanAffineOpts) == 56
    hdr = open(os.path.join(ROOT, "include", "qdsim.h")).read()
    assert "int qd_scan_affine(qd_handle* h, const int32_t* env_of_query_dev, int nq, const double* dir_dev, const double* range_dev," in hdr
    assert "} qd_scan_affine_opts;" in hdr
    # qd_scan2d and its options are untouched
    assert ctypes.sizeof(_lib.QdScanOpts) == 56 and "int qd_scan2d(qd_handle* h, const int32_t* env_of_query_dev, int nq, const int32_t* axes_dev," in hdr
    assert L.qd_scan_affine(None, None, 1, None, None, None, None, None, None, None, None, None, None) == _lib.QD_ERR_ARG   # no crash


def _handle(L, N, R, B, flags=0, qconfig=None):
    from qadapt_hip.vec_env import make_qd_config
    cfg = make_qd_config(DM.load_yaml(None, "env_config.yaml"), qconfig or DM.load_yaml(None, "qarray_config.yaml"), N, R, B,
                         flags=flags)
    h = ctypes.c_void_p()
    L.qd_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    if not h:
        pytest.fail("qd_create handed out no handle")
    return h


def test_scan_affine_argument_checks_need_no_device():
    """Without a GPU qd_create fails with QD_ERR_HIP and still hands out the partial handle (qdsim.h), which is all these
    checks need: each returns before anything touches the device."""
    _lib, L = _built_lib()
    B = 3
    h = _handle(L, 4, 8, B)
    one = ctypes.c_void_p(64)                      # a device pointer that is never dereferenced

    def opts(**kw):
        o = _lib.QdScanAffineOpts(struct_size=ctypes.sizeof(_lib.QdScanAffineOpts))
        for k, v in kw.items():
            setattr(o, k, v)
        return ctypes.byref(o)

    def call(hh=h, env=one, nq=1, dirs=one, rng=one, gv=one, bv=one, o=None):
        return L.qd_scan_affine(hh, env, nq, dirs, rng, gv, bv, None, one, None, None, o, None)

    try:
        assert call(env=None) == _lib.QD_ERR_ARG and b"env_of_query_dev" in L.qd_last_error(h)
        assert call(dirs=None) == _lib.QD_ERR_ARG and b"dir_dev" in L.qd_last_error(h)
        assert call(rng=None) == _lib.QD_ERR_ARG and b"range_dev" in L.qd_last_error(h)
        assert call(gv=None) == _lib.QD_ERR_ARG and b"gate_v_dev" in L.qd_last_error(h)
        assert call(bv=None) == _lib.QD_ERR_ARG and b"barrier_v_dev" in L.qd_last_error(h)
        assert call(nq=-1) == _lib.QD_ERR_ARG and b"nq < 0" in L.qd_last_error(h)
        assert call(o=opts(struct_size=8)) == _lib.QD_ERR_ARG and b"struct_size" in L.qd_last_error(h)
        assert call(o=opts(frame=2)) == _lib.QD_ERR_ARG and b"frame" in L.qd_last_error(h)
        assert call(o=opts(frame=-1)) == _lib.QD_ERR_ARG
        assert call(o=opts(frame=_lib.QD_SCAN_PHYSICAL, vgm_dev=64)) == _lib.QD_ERR_ARG and b"vgm_dev" in L.qd_last_error(h)
        assert call(o=opts(noise_flags=_lib.QD_NOISE_RADIAL)) == _lib.QD_ERR_ARG and b"radial" in L.qd_last_error(h)
        assert call(o=opts(noise_flags=_lib.QD_NOISE_SENSOR | _lib.QD_NOISE_RADIAL)) == _lib.QD_ERR_ARG
        assert call(o=opts(noise_flags=8)) == _lib.QD_ERR_ARG
        assert b"qd_scan_affine" in L.qd_last_error(h)
        assert call(nq=0) == 0 and call(nq=0, o=opts(noise_flags=_lib.QD_NOISE_SENSOR | _lib.QD_NOISE_LATCH)) == 0
    finally:
        L.qd_destroy(h)
    hv = _handle(L, 4, 8, B, flags=_lib.QD_FLAG_VALIDATE)
    try:
        assert call(hh=hv) == _lib.QD_ERR_STATE and b"QD_FLAG_VALIDATE" in L.qd_last_error(hv)
        assert call(hh=hv, dirs=None) == _lib.QD_ERR_ARG                 # the argument checks come first
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


# ------------------------------------------------------------------ the array facade on a stub backend
class StubBackend:
    """Shape-faithful stand-in for VecQuantumDeviceEnv with B = 1 that records its scan_affine calls."""

    def __init__(self, N, R):
        self.N, self.R = N, R
        self.calls = []

    def _obs(self):
        N, R = self.N, self.R
        return {"image": np.zeros((1, R, R, N - 1), np.float32), "obs_gate_voltages": np.zeros((1, N), np.float32),
                "obs_barrier_voltages": np.zeros((1, N - 1), np.float32)}

    def reset(self, seed=None, **kw):
        return self._obs()

    def device_state(self):
        N = self.N
        return {"gate_ground_truth": np.ones((1, N), np.float32), "barrier_ground_truth": np.zeros((1, N - 1), np.float32),
                "sensor_ground_truth": np.array([0.5]), "current_gate_voltages": np.full((1, N), 2.0),
                "current_barrier_voltages": np.full((1, N - 1), 3.0),
                "virtual_gate_matrix": -np.eye(N + 1)[None], "virtual_gate_origin": np.zeros((1, N + 1))}

    def scan_affine(self, env_ids, x, y, x_range, y_range, gate_voltages, barrier_voltages, sensor_voltage=None, **kw):
        self.calls.append(dict(env_ids=list(env_ids), x=x, y=y, x_range=tuple(x_range), y_range=tuple(y_range),
                               gv=np.array(gate_voltages), bv=np.array(barrier_voltages), sv=sensor_voltage, kw=kw))
        R = self.R
        out = {"raw": np.arange(R * R, dtype=np.float64).reshape(1, R, R)}
        if kw.get("normalised"):
            out["image"] = np.zeros((1, R, R), np.float32); out["plohi"] = np.array([[0.0, 1.0]])
        if kw.get("occupations"):
            out["occupations"] = np.zeros((1, R, R, self.N))
        return out


def test_array_scan_affine_mirror(tmp_path):
    N, R = 4, 6
    cfg = DM.load_yaml(None, "env_config.yaml")
    cfg["capacitance_model"]["update_method"] = None
    cfg["simulator"].update(num_dots=N, resolution=R)
    p = tmp_path / "env.yaml"
    p.write_text(yaml.safe_dump(cfg))
    env = QuantumDeviceEnv(config_path=str(p), backend=StubBackend(N, R))
    gv, bv = np.array([1.0, -2.0, 3.0, 4.5]), np.array([0.1, 0.2, 0.3])
    out = env.array.scan_affine("e1_2", "U1_2", (-1, 1), (2, 0), gv, bv, occupations=True, frame="virtual")
    assert out["raw"].shape == (R, R) and out["raw"].dtype == np.float64 and out["occupations"].shape == (R, R, N)
    c = env._b.calls[-1]
    assert (c["x"], c["y"], c["env_ids"], c["sv"]) == ("e1_2", "U1_2", [0], None)
    assert c["x_range"] == (-1, 1) and c["y_range"] == (2, 0) and c["kw"] == {"occupations": True, "frame": "virtual"}
    assert c["gv"].shape == (1, N) and c["bv"].shape == (1, N - 1) and np.array_equal(c["gv"][0], gv) and np.array_equal(c["bv"][0], bv)
    d = {"vP1": 1.0, "B1": -0.3}
    out = env.array.scan_affine(d, np.arange(8.0), (0, 1), (0, 1), gv, bv, 0.25, normalised=True)
    c = env._b.calls[-1]
    assert c["x"] is d and c["sv"] == 0.25 and np.array_equal(c["y"], np.arange(8.0))
    assert set(out) == {"raw", "image", "plohi"} and out["image"].shape == (R, R) and out["plohi"].shape == (2,)
    assert env.current_step == 0
