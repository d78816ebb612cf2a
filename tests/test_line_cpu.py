"""Dense 1-D sweeps (qd_scan1d), CPU tier: the line front end (csrc/qd_line.h: qd_line_voltages, compiled for the host in
tests/hosttest_line) against the affine front end bit for bit, against the reference composer's do1d lines
(tests/golden/line_grids.npz) and against NumPy in the physical frame; the slot arithmetic and the inert tail records; the
argument checks, prototype and export of qd_scan1d; the axis resolver per query; the `env.array.scan1d` mirror and the
`env.array.model.do1d_open` facade on a stub backend.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import yaml

import affine_helpers as AH
import helpers as H
import line_helpers as LH
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


def _directions(N, rng):
    """a plunger, the sensor, a barrier, an e axis and a dense direction"""
    from qadapt_hip.vec_env import scan_axis_vector as vec
    return [("plunger", vec(N - 1, N)), ("sensor", vec("S", N)), ("barrier", vec("B1", N)), ("e", vec(f"e1_{N}", N)),
            ("dense", rng.normal(0, 1, 2 * N))]


# ------------------------------------------------------------------ the affine front end with dy = 0
@pytest.mark.parametrize("N", [2, 4, 8])
def test_line_voltages_equal_row_0_of_the_affine_front_end(N):
    """qd_line_voltages(d, [lo, hi], n) has the bits of qd_affine_voltages(dx = d, dy = 0, R = n) in row 0, in v_ext, vpp and tc:
    both frames, a plunger, the sensor, a barrier, an e axis and a dense direction, a forward and a reversed range, n in
    {1, 5, 8}.  (The y range of the affine scan is finite and arbitrary: fma(sy, 0, w) = w for every w but -0.)"""
    par, st, rng = _scene(N, 900 + N)
    for frame in (LH.VIRTUAL, LH.PHYSICAL):
        for n in (1, 5, 8):
            for name, d in _directions(N, rng):
                for rg in ((-3.25, 7.5), (6.5, -2.75)):
                    rg = np.array(rg) + rng.uniform(-1, 1, 2)
                    got = LH.line_voltages(N, par, st, d, rg, n, frame)
                    ref = AH.affine_voltages(N, par, st, d, np.zeros(2 * N), [rg[0], rg[1], 11.0, -2.0], n, frame)
                    for what, a, b in zip(("v_ext", "vpp", "tc"), got, ref):
                        assert np.isfinite(a).all()
                        assert PH.same(a, b[:n]), (what, frame, n, name, tuple(rg))
                    if n > 1 and name != "sensor":
                        assert np.ptp(got[1], axis=0).max() > 0, (name, n)           # the line moves
                    if n == 1:
                        # one point: s = lo
                        one = AH.affine_voltages(N, par, st, d, np.zeros(2 * N), [rg[0], rg[0], 0.0, 0.0], 2, frame)
                        assert PH.same(got[0][0], one[0][0])


# ------------------------------------------------------------------ the reference composer's lines
def test_golden_line_grids():
    """GateVoltageComposer.do1d(gate, min, max, n) of the reference on P, vP, e and U gates (adjacent, non-adjacent and reversed
    dot pairs, asymmetric and reversed ranges, N in {2, 4, 8}, n in {5, 8}).  The composer holds the other gates at 0, renders
    "P" without matrix or origin and adds its origin once per "vP" sweep, sqrt(2) times per "U" sweep and never per "e" sweep;
    the front end adds it once in the virtual frame, so the surplus (multiplicity - 1) origin is taken off the reference.  Gate
    part of v_ext within (G+1) eps (|VGM| |W| + |origin|) per element (the bound of test_golden_affine_grids; in the physical
    frame the matrix is the identity and the origin 0)."""
    from qadapt_hip.vec_env import scan_axis_vector
    z = np.load(os.path.join(ROOT, "tests", "golden", "line_grids.npz"))
    ncases = int(z["n_cases"])
    assert ncases >= 12
    seen_N, seen_n, kinds = set(), set(), set()
    for c in range(ncases):
        g = lambda k: z[f"c{c}_{k}"]     # noqa: E731
        N, n, gate = int(g("n_dot")), int(g("n")), str(g("gate"))
        L = layout(N); G = N + 1
        seen_N.add(N); seen_n.add(n)
        rg = g("ranges")
        kind = "vP" if gate[0] == "v" else gate[0]
        kinds.add(kind)
        if kind in "eU":
            i, j = (int(t) for t in gate[1:].split("_"))
            kinds |= {"nonadjacent"} if abs(i - j) > 1 else {"adjacent"}
            kinds |= {"reversed_pair"} if i > j else set()
        kinds |= {"reversed_range"} if rg[0] > rg[1] else set()
        kinds |= {"asymmetric"} if abs(rg[0] + rg[1]) > 1e-9 else set()
        mult = float(g("origin_multiplicity"))
        assert mult == {"P": 0.0, "e": 0.0, "U": np.sqrt(2.0), "vP": 1.0}[kind]
        physical = kind == "P"
        par = np.zeros(L.size); st = np.zeros(L.s_size)
        par[L.origin:L.origin + G] = g("origin")
        st = SH.query_state(N, st, np.zeros(N), np.zeros(N - 1), 0.0, g("vgm"))
        # "P{g}" is the composer's physical gate g, 1-indexed, g = N+1 the sensor gate: control index g - 1
        d = scan_axis_vector(int(gate[1:]) - 1, N, "physical") if physical else scan_axis_vector(gate, N)
        v_ext, _, _ = LH.line_voltages(N, par, st, d, rg, n, LH.PHYSICAL if physical else LH.VIRTUAL)
        got = v_ext[:, :G]
        W = LH.numpy_w(np.zeros(2 * N), d, rg, n)[:, :G]
        if physical:
            ref = g("vg")
            bound = (G + 1) * EPS * np.abs(W)
        else:
            ref = g("vg") - (mult - 1.0) * g("origin")
            bound = (G + 1) * EPS * (np.abs(W) @ np.abs(g("vgm")).T + np.abs(g("origin")))
        worst = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
        print(f"[golden lines] case {c} N={N} n={n} {gate}: worst |diff| / bound {worst:.3f}")
        assert np.all(np.abs(got - ref) <= bound), (c, worst)
        assert np.ptp(got, axis=0).max() > 0
        # direction of the sweep: the reversed line is NOT within the bound
        assert not np.all(np.abs(got[::-1] - ref) <= bound), c
        assert PH.same(v_ext[:, G:], np.zeros((n, N - 1)))
    assert seen_N == {2, 4, 8} and seen_n == {5, 8}
    assert kinds == {"P", "vP", "e", "U", "adjacent", "nonadjacent", "reversed_pair", "reversed_range", "asymmetric"}


# ------------------------------------------------------------------ dense directions against NumPy
@pytest.mark.parametrize("N", [2, 4, 8])
def test_physical_frame_dense_direction_matches_numpy(N):
    """v_ext = W in the physical frame, W[i] = fma(s, d[i], W0[i]) against NumPy's W0 + s d.  The front end rounds once, NumPy
    twice, each by at most eps / 2 of a partial sum bounded by |W0| + |s d|; s itself is start + i * step on both sides with the
    same three roundings, at most 3 eps (|lo| + |hi|) apart: 4 eps (|W0| + (|lo| + |hi|) |d|) per element bounds both.  vpp and
    tc have the bits of qd_point_front at that v_ext."""
    par, st, rng = _scene(N, 940 + N)
    for n in (5, 8, 37):
        for k in range(3):
            d = rng.normal(0, 1, 2 * N)
            rg = np.array([-3.25, 7.5]) + rng.uniform(-1, 1, 2)
            v_ext, vpp, tc = LH.line_voltages(N, par, st, d, rg, n, LH.PHYSICAL)
            want = LH.numpy_line(N, st, None, d, rg, n, LH.PHYSICAL)
            tol = 4 * EPS * (np.abs(AH.base_point(N, st)) + (abs(rg[0]) + abs(rg[1])) * np.abs(d))
            assert np.all(np.abs(v_ext - want) <= tol), (n, k, float((np.abs(v_ext - want) / tol).max()))
            pv, pt = SH.point_front(N, par, v_ext)
            assert PH.same(vpp, pv) and PH.same(tc, pt), (n, k)


# ------------------------------------------------------------------ slot arithmetic
def test_slot_arithmetic_and_inert_tail():
    """Rl = ceil(sqrt(n)), the tail Rl^2 - n and the batches ceil(Rl^2 / 256) for n in {1, 2, 63, 64, 65, 100, P} (P = 64^2 and
    the odd 37^2), and for every n up to 5000 against integer arithmetic; every tail record of a slot is the inert all-zero
    record, every point's record is not, and a point's vpp and tc are those of the front end."""
    import math
    for P in (64 * 64, 37 * 37):
        for n in (1, 2, 63, 64, 65, 100, P):
            side, tail, nb = LH.slot(n)
            assert side == math.isqrt(n - 1) + 1 and (side - 1) ** 2 < n <= side * side, n
            assert tail == side * side - n and 0 <= tail < 2 * side - 1
            assert nb == -(-side * side // 256)
            assert side <= math.isqrt(P) and nb <= -(-P // 256)              # a slot never exceeds one channel image of the handle
    assert LH.slot(1) == (1, 0, 1) and LH.slot(2) == (2, 2, 1) and LH.slot(63) == (8, 1, 1) and LH.slot(64) == (8, 0, 1)
    assert LH.slot(65) == (9, 16, 1) and LH.slot(100) == (10, 0, 1) and LH.slot(4096) == (64, 0, 16) and LH.slot(257) == (17, 32, 2)
    for n in range(1, 5001):
        side = LH.slot(n)[0]
        assert (side - 1) ** 2 < n <= side * side, n
    assert LH.slot(2 ** 30)[0] == 2 ** 15 and LH.slot(2 ** 30 + 1)[0] == 2 ** 15 + 1
    N = 4
    par, st, rng = _scene(N, 960)
    d = rng.normal(0, 1, 2 * N)
    off_vpp = 2 * 32 + 4 * 8 + 8                       # QdPixelRec: idx[32] uint16, fl[8] int32, nvalid, pad, then vpp[9], tc[7], E[32]
    for n in (1, 2, 63, 64, 65, 100):
        side, tail, _ = LH.slot(n)
        recs, live = LH.line_records(N, par, st, d, (-2.0, 3.0), n)
        assert recs.shape == (side * side, off_vpp + 8 * (9 + 7 + 32))
        assert live[:n].all() and not live[n:].any() and int((~live).sum()) == tail
        assert not recs[n:].any(), n                                           # the tail: all zero, written over the 0xA5 fill
        _, vpp, tc = LH.line_voltages(N, par, st, d, (-2.0, 3.0), n)
        got = np.ascontiguousarray(recs[:n, off_vpp:off_vpp + 8 * 16]).view(np.float64).reshape(n, 16)
        assert PH.same(got[:, :N + 1], vpp) and PH.same(got[:, 9:9 + N - 1], tc)


# ------------------------------------------------------------------ the axis resolver, per query
def test_scan1d_axis_resolver():
    from qadapt_hip.vec_env import scan_axis_vector as vec, scan_axis_vectors as vecs
    N = 4
    assert vecs("U1_3", N, "virtual", 2).shape == (2, 8)
    per = vecs(["vP2", {"vP1": 1.0, "B2": -0.5}, "e4_1", 4], N, "virtual", 4)
    assert per[0].tolist() == vec("vP2", N).tolist() and per[1].tolist() == [1, 0, 0, 0, 0, 0, -0.5, 0]
    assert per[2].tolist() == [-1, 0, 0, 1, 0, 0, 0, 0] and per[3].tolist() == vec("S", N).tolist()
    assert vecs("P3", N, "physical", 1).tolist() == [[0, 0, 1, 0, 0, 0, 0, 0]]
    with pytest.raises(ValueError, match="physical frame"):
        vecs("P3", N, "virtual", 1)


# ------------------------------------------------------------------ C ABI without a GPU
def _built_lib():
    from qadapt_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is missing: run __graft_entry__.build() before the tests (no test compiles it)")
    return _lib, _lib.lib()


def test_scan1d_symbol_and_prototype():
    _lib, L = _built_lib()
    assert "qd_scan1d" in _lib.EXPORTS_WITH_DIGITS and hasattr(L, "qd_scan1d")
    at = L.qd_scan1d.argtypes
    assert len(at) == 14 and at[2] is ctypes.c_int and at[3] is ctypes.c_int and L.qd_scan1d.restype is ctypes.c_int
    assert at[12]._type_ is _lib.QdScan1dOpts and ctypes.sizeof(_lib.QdScan1dOpts) == 56
    hdr = open(os.path.join(ROOT, "include", "qdsim.h")).read()
    assert "int qd_scan1d(qd_handle* h, const int32_t* env_of_query_dev, int nq, int n_points, const double* dir_dev," in hdr
    assert "} qd_scan1d_opts;" in hdr and f"#define QD_LINE_SLOTS {_lib.QD_LINE_SLOTS}" in hdr
    # the siblings and their options are untouched
    assert ctypes.sizeof(_lib.QdScanOpts) == 56 and ctypes.sizeof(_lib.QdScanAffineOpts) == 56
    assert L.qd_scan1d(None, None, 1, 1, None, None, None, None, None, None, None, None, None, None) == _lib.QD_ERR_ARG   # no crash


def _handle(L, N, R, B, flags=0, qconfig=None):
    from qadapt_hip.vec_env import make_qd_config
    cfg = make_qd_config(DM.load_yaml(None, "env_config.yaml"), qconfig or DM.load_yaml(None, "qarray_config.yaml"), N, R, B,
                         flags=flags)
    h = ctypes.c_void_p()
    L.qd_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    if not h:
        pytest.fail("qd_create handed out no handle")
    return h


def test_scan1d_argument_checks_need_no_device():
    """Without a GPU qd_create fails with QD_ERR_HIP and still hands out the partial handle (qdsim.h), which is all these
    checks need: each returns before anything touches the device."""
    _lib, L = _built_lib()
    B, R = 3, 8
    h = _handle(L, 4, R, B)
    one = ctypes.c_void_p(64)                      # a device pointer that is never dereferenced

    def opts(**kw):
        o = _lib.QdScan1dOpts(struct_size=ctypes.sizeof(_lib.QdScan1dOpts))
        for k, v in kw.items():
            setattr(o, k, v)
        return ctypes.byref(o)

    def call(hh=h, env=one, nq=1, n=5, dirs=one, rng=one, gv=one, bv=one, o=None):
        return L.qd_scan1d(hh, env, nq, n, dirs, rng, gv, bv, None, one, None, None, o, None)

    try:
        assert call(env=None) == _lib.QD_ERR_ARG and b"env_of_query_dev" in L.qd_last_error(h)
        assert call(dirs=None) == _lib.QD_ERR_ARG and b"dir_dev" in L.qd_last_error(h)
        assert call(rng=None) == _lib.QD_ERR_ARG and b"range_dev" in L.qd_last_error(h)
        assert call(gv=None) == _lib.QD_ERR_ARG and b"gate_v_dev" in L.qd_last_error(h)
        assert call(bv=None) == _lib.QD_ERR_ARG and b"barrier_v_dev" in L.qd_last_error(h)
        assert call(nq=-1) == _lib.QD_ERR_ARG and b"nq < 0" in L.qd_last_error(h)
        for bad in (0, -3, R * R + 1):
            assert call(n=bad) == _lib.QD_ERR_ARG and b"n_points" in L.qd_last_error(h)
            assert call(n=bad, nq=0) == _lib.QD_ERR_ARG                       # the argument checks come before "nothing to do"
        assert call(o=opts(struct_size=8)) == _lib.QD_ERR_ARG and b"struct_size" in L.qd_last_error(h)
        assert call(o=opts(frame=2)) == _lib.QD_ERR_ARG and b"frame" in L.qd_last_error(h)
        assert call(o=opts(frame=-1)) == _lib.QD_ERR_ARG
        assert call(o=opts(frame=_lib.QD_SCAN_PHYSICAL, vgm_dev=64)) == _lib.QD_ERR_ARG and b"vgm_dev" in L.qd_last_error(h)
        assert call(o=opts(noise_flags=_lib.QD_NOISE_RADIAL)) == _lib.QD_ERR_ARG and b"radial" in L.qd_last_error(h)
        assert call(o=opts(noise_flags=_lib.QD_NOISE_SENSOR | _lib.QD_NOISE_RADIAL)) == _lib.QD_ERR_ARG
        assert call(o=opts(noise_flags=8)) == _lib.QD_ERR_ARG
        assert b"qd_scan1d" in L.qd_last_error(h)
        assert call(nq=0) == 0 and call(nq=0, n=1) == 0 and call(nq=0, n=R * R) == 0
        assert call(nq=0, o=opts(noise_flags=_lib.QD_NOISE_SENSOR | _lib.QD_NOISE_LATCH)) == 0
    finally:
        L.qd_destroy(h)
    hv = _handle(L, 4, R, B, flags=_lib.QD_FLAG_VALIDATE)
    try:
        assert call(hh=hv) == _lib.QD_ERR_STATE and b"QD_FLAG_VALIDATE" in L.qd_last_error(hv)
        assert call(hh=hv, dirs=None) == _lib.QD_ERR_ARG                 # the argument checks come first
        assert call(hh=hv, n=0) == _lib.QD_ERR_ARG
    finally:
        L.qd_destroy(hv)
    from qadapt_hip.vec_env import override_charge_states
    q = override_charge_states(DM.load_yaml(None, "qarray_config.yaml"), "all")
    q["simulator"]["model"]["max_charge_carriers"] = 2
    hf = _handle(L, 3, R, B, qconfig=q)
    try:
        assert call(hh=hf) == _lib.QD_ERR_STATE and b"full charge-state space" in L.qd_last_error(hf)
    finally:
        L.qd_destroy(hf)


# ------------------------------------------------------------------ the facades on a stub backend
class StubBackend:
    """Shape-faithful stand-in for VecQuantumDeviceEnv with B = 1 that records its scan1d calls."""

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

    def scan1d(self, env_ids, axis, s_range, n_points, gate_voltages, barrier_voltages, sensor_voltage=None, **kw):
        self.calls.append(dict(env_ids=list(env_ids), axis=axis, s_range=tuple(s_range), n=n_points, gv=np.array(gate_voltages),
                               bv=np.array(barrier_voltages), sv=sensor_voltage, kw=kw))
        n = int(n_points)
        out = {"raw": np.arange(n, dtype=np.float64).reshape(1, n), "image": np.zeros((1, n), np.float32),
               "plohi": np.array([[0.0, 1.0]])}
        if kw.get("occupations"):
            out["occupations"] = np.arange(n * self.N, dtype=np.float64).reshape(1, n, self.N)
        return out


def _stub_env(tmp_path, N, R):
    cfg = DM.load_yaml(None, "env_config.yaml")
    cfg["capacitance_model"]["update_method"] = None
    cfg["simulator"].update(num_dots=N, resolution=R)
    p = tmp_path / "env.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return QuantumDeviceEnv(config_path=str(p), backend=StubBackend(N, R))


def test_array_scan1d_mirror(tmp_path):
    N, R = 4, 6
    env = _stub_env(tmp_path, N, R)
    gv, bv = np.array([1.0, -2.0, 3.0, 4.5]), np.array([0.1, 0.2, 0.3])
    out = env.array.scan1d("e1_2", (-1, 1), 17, gv, bv, occupations=True, frame="virtual")
    assert out["raw"].shape == (17,) and out["raw"].dtype == np.float64 and out["occupations"].shape == (17, N)
    assert out["image"].shape == (17,) and out["plohi"].shape == (2,)
    c = env._b.calls[-1]
    assert (c["axis"], c["env_ids"], c["sv"], c["n"]) == ("e1_2", [0], None, 17)
    assert c["s_range"] == (-1, 1) and c["kw"] == {"occupations": True, "frame": "virtual"}
    assert c["gv"].shape == (1, N) and c["bv"].shape == (1, N - 1) and np.array_equal(c["gv"][0], gv) and np.array_equal(c["bv"][0], bv)
    d = {"vP1": 1.0, "B1": -0.3}
    out = env.array.scan1d(d, (2, 0), 5, gv, bv, 0.25, noise=("sensor", "latch"))
    c = env._b.calls[-1]
    assert c["axis"] is d and c["sv"] == 0.25 and c["s_range"] == (2, 0) and c["kw"] == {"noise": ("sensor", "latch")}
    assert set(out) == {"raw", "image", "plohi"}
    assert env.current_step == 0


def test_model_do1d_open_facade(tmp_path):
    """The reference's gate grammar: an int and "P{g}" sweep physical gate g (control g - 1, g = N + 1 the sensor gate) in the
    physical frame, "vP", "e" and "U" go through as names in the virtual frame; the base point is zero, the sweep noise-free,
    the peak width the model's, and the result (signal (points, 1), n_open (points, N))."""
    N, R = 4, 6
    env = _stub_env(tmp_path, N, R)
    m = env.array.model
    m.coulomb_peak_width = 0.125
    for gate, axis, frame in ((2, 1, "physical"), ("P3", 2, "physical"), (N + 1, N, "physical"), (f"P{N + 1}", N, "physical"),
                              (np.int64(1), 0, "physical"), ("vP2", "vP2", "virtual"), ("e1_3", "e1_3", "virtual"),
                              ("U4_2", "U4_2", "virtual")):
        sig, occ = m.do1d_open(gate, -1.5, 2.5, 9)
        c = env._b.calls[-1]
        assert c["axis"] == axis and c["kw"] == {"frame": frame, "gamma": 0.125, "occupations": True}, gate
        assert c["s_range"] == (-1.5, 2.5) and c["n"] == 9 and c["env_ids"] == [0] and c["sv"] == 0.0
        assert c["gv"].shape == (1, N) and not c["gv"].any() and c["bv"].shape == (1, N - 1) and not c["bv"].any()
        assert sig.shape == (9, 1) and sig.dtype == np.float64 and np.array_equal(sig[:, 0], np.arange(9.0))
        assert occ.shape == (9, N) and np.array_equal(occ, np.arange(9.0 * N).reshape(9, N))
    m.coulomb_peak_width = None
    m.do1d_open("vP1", 0, 1, 3)
    assert env._b.calls[-1]["kw"]["gamma"] is None
    for bad in (0, N + 2, "P0", f"P{N + 2}", "B1", "S", "x", "", 1.5, None, True):
        with pytest.raises(ValueError):
            m.do1d_open(bad, 0, 1, 3)
    doc = type(m).do1d_open.__doc__
    assert "sqrt(2)" in doc and "origin" in doc and "ONCE" in doc
    assert env.current_step == 0
