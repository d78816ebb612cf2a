"""The closed regime's interface without a GPU: the ctypes prototypes against include/qdsim.h, the argument checks of the two
C calls on a handle that never reached a device, the Python layer's n_charge checks and the model facade on a stub backend."""
import ctypes
import os
import re

import numpy as np
import pytest
import yaml

import helpers as H
from qadapt_hip import device_model as DM
from qadapt_hip.env import QuantumDeviceEnv


def _built_lib():
    from qadapt_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is missing: run __graft_entry__.build() before the tests (no test compiles it)")
    return _lib, _lib.lib()


def _c_args(hdr, name):
    """the parameter list of `int name(...)` in the header, one string per parameter"""
    m = re.search(r"\bint " + name + r"\((.*?)\);", hdr, re.S)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _kind(decl):
    """what a ctypes prototype must say about a C parameter"""
    if "*" not in decl:
        return ctypes.c_int
    if decl.startswith("const int32_t*") and decl.endswith("_host"):
        return ctypes.POINTER(ctypes.c_int32)
    if decl.startswith("const int64_t*"):
        return ctypes.POINTER(ctypes.c_int64)
    if decl.startswith("const double*") and decl.endswith("_host"):
        return ctypes.POINTER(ctypes.c_double)
    if decl.startswith("const qd_scan_grid_opts*"):
        return "opts"
    return ctypes.c_void_p


@pytest.mark.parametrize("name,open_name,extra", [("qd_eval_points_closed", "qd_eval_points", ["n_charge_host", "states_dst"]),
                                                  ("qd_scan_grid_closed", "qd_scan_grid", ["n_charge_dev"])])
def test_prototypes_match_the_header(name, open_name, extra):
    _lib, L = _built_lib()
    hdr = open(os.path.join(H.ROOT, "include", "qdsim.h")).read()
    assert name in _lib.EXPORTS and hasattr(L, name)
    decl = _c_args(hdr, name)
    fn = getattr(L, name)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(decl)
    for a, d in zip(fn.argtypes, decl):
        k = _kind(d)
        if k == "opts":
            assert a._type_ is _lib.QdScanGridOpts, d
        elif k is ctypes.c_int or k is ctypes.c_void_p:
            assert a is k, d
        else:
            assert a._type_ is k._type_, d
    # the arguments of the open sibling in its order, plus the new ones
    names = [d.split()[-1].lstrip("*") for d in decl]
    open_names = [d.split()[-1].lstrip("*") for d in _c_args(hdr, open_name)]
    assert [n for n in names if n not in extra] == open_names and all(e in names for e in extra)


def _handle(L, N, R, B, flags=0, qconfig=None):
    from qadapt_hip.vec_env import make_qd_config
    cfg = make_qd_config(DM.load_yaml(None, "env_config.yaml"), qconfig or DM.load_yaml(None, "qarray_config.yaml"), N, R, B,
                         flags=flags)
    h = ctypes.c_void_p()
    L.qd_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    if not h:
        pytest.fail("qd_create handed out no handle")
    return h


def _full_space_config():
    from qadapt_hip.vec_env import override_charge_states
    q = override_charge_states(DM.load_yaml(None, "qarray_config.yaml"), "all")
    q["simulator"]["model"]["max_charge_carriers"] = 2
    return q


def test_argument_checks_need_no_device():
    """Every refusal that is found before the device is touched (qd_create without a GPU hands out the partial handle)."""
    _lib, L = _built_lib()
    B = 3
    one = ctypes.c_void_p(64)                          # a device pointer that is never dereferenced
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)     # noqa: E731
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)     # noqa: E731
    pts = lambda h, q, env=i32(0), start=i64(0, 1), ng=1: L.qd_eval_points_closed(h, env, start, ng, one, one, None, q, one, one, None, None)  # noqa: E731
    opts = _lib.QdScanGridOpts(struct_size=ctypes.sizeof(_lib.QdScanGridOpts))
    grid = lambda h, q, o=None: L.qd_scan_grid_closed(h, one, 1, 4, 2, one, one, one, one, None, q, one, None, None, o, None)   # noqa: E731
    assert pts(None, i32(1)) == _lib.QD_ERR_ARG and grid(None, one) == _lib.QD_ERR_ARG
    h = _handle(L, 4, 8, B)
    try:
        assert pts(h, None) == _lib.QD_ERR_ARG and b"n_charge_host" in L.qd_last_error(h)
        for bad in (-1, 32768, 1 << 20):
            assert pts(h, i32(bad)) == _lib.QD_ERR_ARG and b"0..32767" in L.qd_last_error(h), bad
        assert pts(h, i32(2, -3), env=i32(0, 1), start=i64(0, 1, 2), ng=2) == _lib.QD_ERR_ARG
        assert pts(h, i32(2), env=i32(B)) == _lib.QD_ERR_ARG and b"qd_eval_points_closed: env id" in L.qd_last_error(h)
        assert pts(h, i32(2), start=i64(3, 3)) == 0                                    # a group without a point
        assert grid(h, None) == _lib.QD_ERR_ARG and b"n_charge_dev" in L.qd_last_error(h)
        for flags in (_lib.QD_NOISE_SENSOR, _lib.QD_NOISE_LATCH, _lib.QD_NOISE_SENSOR | _lib.QD_NOISE_LATCH):
            opts.noise_flags = flags
            assert grid(h, one, ctypes.byref(opts)) == _lib.QD_ERR_ARG and b"no noise stages" in L.qd_last_error(h), flags
        opts.noise_flags = _lib.QD_NOISE_RADIAL
        assert grid(h, one, ctypes.byref(opts)) == _lib.QD_ERR_ARG
        opts.noise_flags = 0
        assert L.qd_scan_grid_closed(h, one, 1, 9, 9, one, one, one, one, None, one, one, None, None, None, None) == _lib.QD_ERR_ARG
        assert b"qd_scan_grid_closed: nx and ny" in L.qd_last_error(h)
        assert L.qd_scan_grid_closed(h, one, 0, 4, 2, one, one, one, one, None, one, one, None, None, None, None) == 0   # no query
    finally:
        L.qd_destroy(h)
    for kw, word in ((dict(flags=_lib.QD_FLAG_VALIDATE), b"QD_FLAG_VALIDATE"), (dict(qconfig=_full_space_config()), b"full charge-state space")):
        hs = _handle(L, 3, 8, B, **kw)
        try:
            assert pts(hs, i32(2)) == _lib.QD_ERR_STATE and word in L.qd_last_error(hs)
            assert grid(hs, one) == _lib.QD_ERR_STATE and word in L.qd_last_error(hs)
            assert pts(hs, i32(-2)) == _lib.QD_ERR_ARG                                 # arguments first
        finally:
            L.qd_destroy(hs)


def test_n_charge_of_the_python_layer():
    from qadapt_hip.vec_env import closed_charges
    assert closed_charges(3, 4, "query").tolist() == [3, 3, 3, 3] and closed_charges(3, 4, "query").dtype == np.int32
    assert closed_charges([0, 32767], 2, "query").tolist() == [0, 32767]
    assert closed_charges(np.array([2.0, 5.0]), 2, "query").tolist() == [2, 5]
    for bad in (-1, 32768, [1, -1], 2.5, True, "3", [[1, 2]], [1, 2, 3]):
        with pytest.raises(ValueError):
            closed_charges(bad, 2, "query")


# ------------------------------------------------------------------ the model facade on a stub backend
class StubBackend:
    """Shape-faithful stand-in for VecQuantumDeviceEnv with B = 1 that records its eval_points and scan_grid calls."""

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

    def eval_points(self, env_ids, vg, vb, gamma=None, outputs=("signal", "occupations"), n_charge=None, states=False):
        vg = np.array(vg)
        self.calls.append(dict(fn="eval_points", n_charge=n_charge, outputs=tuple(outputs), gamma=gamma))
        m = vg.shape[1]
        out = {"signal": vg[..., 0], "occupations": np.broadcast_to(vg[..., :self.N], (1, m, self.N))}
        return {k: out[k] for k in outputs}

    def scan_grid(self, env_ids, x, y, x_range, y_range, nx, ny, gv, bv, sv=None, **kw):
        self.calls.append(dict(fn="scan_grid", x=x, y=y, x_range=x_range, y_range=y_range, nx=nx, ny=ny, **kw))
        return {"raw": np.zeros((1, ny, nx)), "occupations": np.ones((1, ny, nx, self.N))}

    def scan_grid_closed(self, env_ids, x, y, x_range, y_range, nx, ny, gv, bv, n_charge, sv=None, **kw):
        self.calls.append(dict(fn="scan_grid_closed", x=x, y=y, x_range=x_range, y_range=y_range, nx=nx, ny=ny, n_charge=n_charge, **kw))
        return {"raw": np.zeros((1, ny, nx)), "occupations": np.ones((1, ny, nx, self.N))}


def _env(tmp_path, N=4, R=6):
    cfg = DM.load_yaml(None, "env_config.yaml")
    cfg["capacitance_model"]["update_method"] = None
    cfg["simulator"].update(num_dots=N, resolution=R)
    p = tmp_path / "env.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return QuantumDeviceEnv(config_path=str(p), backend=StubBackend(N, R))


def test_model_facade_closed_functions(tmp_path):
    N = 4
    env = _env(tmp_path, N, 6)
    model = env.array.model
    rng = np.random.default_rng(2)
    for lead in ((), (5,), (3, 7)):
        vg, vb = rng.normal(size=lead + (N + 1,)), rng.normal(size=lead + (N - 1,))
        signal, n = model.charge_sensor_closed(vg, 3, vb)
        assert signal.shape == lead + (1,) and n.shape == lead + (N,) and signal.dtype == n.dtype == np.float64
        assert env._b.calls[-1] == dict(fn="eval_points", n_charge=3, outputs=("signal", "occupations"), gamma=None)
        assert model.ground_state_closed(vg, 2, vb=vb).shape == lead + (N,)
        assert env._b.calls[-1]["n_charge"] == 2 and env._b.calls[-1]["outputs"] == ("occupations",)
    with pytest.raises(NotImplementedError, match="model.tc"):                         # the vb is None rule of the open functions
        model.charge_sensor_closed(np.zeros(N + 1), 2)
    with pytest.raises(NotImplementedError):
        model.ground_state_closed(np.zeros(N + 1), 2, None)
    # do1d_closed is a one-row grid with a zero second axis; shapes of the open functions
    model.coulomb_peak_width = 0.3
    signal, n = model.do1d_closed("e1_2", -1.0, 2.0, 17, 3)
    assert signal.shape == (17, 1) and n.shape == (17, N)
    c = env._b.calls[-1]
    assert (c["fn"], c["nx"], c["ny"], c["n_charge"], c["frame"], c["gamma"]) == ("scan_grid_closed", 17, 1, 3, "virtual", 0.3)
    assert c["x"] == "e1_2" and np.array_equal(c["y"], np.zeros(2 * N)) and c["x_range"] == (-1.0, 2.0)
    signal, n = model.do1d_closed(2, 0.0, 1.0, 5, 1)
    assert signal.shape == (5, 1) and env._b.calls[-1]["frame"] == "physical" and env._b.calls[-1]["x"] == 1
    signal, n = model.do2d_closed("P1", -1.0, 1.0, 9, "P2", 0.0, 2.0, 4, 2)
    assert signal.shape == (4, 9, 1) and n.shape == (4, 9, N)
    c = env._b.calls[-1]
    assert (c["nx"], c["ny"], c["n_charge"], c["frame"]) == (9, 4, 2, "physical")
    model.do2d_open("P1", -1.0, 1.0, 9, "P2", 0.0, 2.0, 4)
    assert env._b.calls[-1]["fn"] == "scan_grid" and "n_charge" not in env._b.calls[-1]                                          # the open call is as it was
    with pytest.raises(NotImplementedError):
        model.do2d_closed("P1", -1.0, 1.0, 9, "vP2", 0.0, 2.0, 4, 2)
    with pytest.raises(ValueError):
        model.do1d_closed("Q7", 0.0, 1.0, 5, 1)
