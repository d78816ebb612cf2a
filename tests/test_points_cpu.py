"""Point evaluation, CPU tier: the point front end (csrc/qd_points.h: qd_point_front, compiled for the host in
tests/hosttest_points) against the scan front end at the scan's own voltages, bit for bit; the inert padding record in the
host build of the structure kernel's pair test; the argument checks, prototype and export of qd_eval_points; and the
`env.array.model` facade on a stub backend.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import yaml

import helpers as H
import points_helpers as PH
import test_gs_hop_cpu as HOP
from qadapt_hip import device_model as DM
from qadapt_hip.env import QuantumDeviceEnv
from qadapt_hip.layout import layout

ROOT = H.ROOT


# ------------------------------------------------------------------ the front end
@pytest.mark.parametrize("N,linear", [(2, False), (4, False), (8, False), (4, True)])
def test_point_front_reproduces_the_scan_front_end_bit_for_bit(N, linear):
    """Every pixel of an 8 x 8 scan of every channel, two devices, near and far from the ground truth: the v_ext that
    qd_pixel_voltages synthesises, fed to qd_point_front, gives the vpp, tc and (scaled) v' of helpers.host_front."""
    R, L = 8, layout(N)
    eb = PH.blocks(N, [300 + N, 301 + N], linear=linear)
    rng = np.random.default_rng(17 + N)
    scaled = 0
    for e, mode in enumerate(("near", "far")):
        par = eb.params[e]
        assert (par[L.scal + 4] != 0.0) == linear
        st = H.place(N, eb.state[e], mode, rng)
        for ch in range(N - 1):
            v_ext, vpp, tc = PH.scan_voltages(N, par, st, ch, R)
            ref = H.host_front(N, par, st, ch, R)
            assert PH.same(vpp, ref["vpp"]) and PH.same(tc, ref["tc"])          # the harness is the scan front end
            out = PH.point_front(N, par, v_ext)
            assert PH.same(out["vpp"], ref["vpp"]), (mode, ch)
            assert PH.same(out["tc"], ref["tc"]), (mode, ch)
            assert PH.same(out["vd"], ref["vd"]), (mode, ch)
            assert np.all(out["ncont"] >= 0.0) and np.all(np.isfinite(out["isa"]))
            # the search sees floor(n_cont): the same kept states as the scan's
            assert np.array_equal(np.floor(out["ncont"]).astype(np.int32), ref["floors"]), (mode, ch)
            scaled += int(np.any(out["vd"] != out["vpp"][:, :N]))
            assert np.all(out["isa"] == 1.0) or linear
    assert (scaled > 0) == linear                                            # the linear model really rescaled v'


# ------------------------------------------------------------------ the padding record
def test_inert_padding_record_emits_no_task():
    """The padding record of qd_k_points_front is all zero: nvalid = 0, codes 0, tc 0.  In the structure kernel
    (qd_ground_structure) lane m's code is 0 (m >= nvalid), the coupling mask tcq is 0 (every tc == 0), and the verdict of
    the pair test on equal codes is 0 whatever the mask; `valid` is false for every lane, so every neighbour mask is empty,
    every component has one state, and `solve = active && ssz > 1` is false: no task.  nvalid = 0 is not QD_T_REDO (-1), so
    the redo pass returns at once."""
    zero = np.zeros(32, np.uint32)
    for n in range(2, 9):
        for tcq in HOP.masks_of(n):                                   # any coupling mask, not only the record's 0
            assert not HOP.hop(zero, zero, tcq).any()
    # the kernel's 16 exchange rounds on the 32 zero codes: no verdict, so nbrmask = 0 for every lane
    ecode, tcq, acc = zero, np.uint32(0), np.zeros(32, np.uint32)
    for j in range(1, 17):
        acc |= HOP.hop(ecode, np.roll(ecode, -j), tcq) << np.uint32(j)
    assert not acc.any()
    seg = np.uint32(1) << np.arange(32, dtype=np.uint32)              # seg = (1 << m) | nbrmask
    assert all(bin(int(s)).count("1") == 1 for s in seg)              # ssz = 1 everywhere -> solve is false
    hdr = open(os.path.join(H.CSRC, "qd_tile.h")).read()
    assert "#define QD_T_REDO (-1)" in hdr
    src = open(os.path.join(H.CSRC, "qd_groundstate.h")).read()
    assert "const bool solve = active && ssz > 1;" in src and "const bool valid = m < nvalid;" in src


# ------------------------------------------------------------------ C ABI without a GPU
def _built_lib():
    from qadapt_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is missing: run __graft_entry__.build() before the tests (no test compiles it)")
    return _lib, _lib.lib()


def test_eval_points_symbol_and_prototype():
    _lib, L = _built_lib()
    assert "qd_eval_points" in _lib.EXPORTS and hasattr(L, "qd_eval_points")
    at = L.qd_eval_points.argtypes
    assert len(at) == 10 and at[3] is ctypes.c_int and L.qd_eval_points.restype is ctypes.c_int
    assert at[1]._type_ is ctypes.c_int32 and at[2]._type_ is ctypes.c_int64 and at[6]._type_ is ctypes.c_double
    hdr = open(os.path.join(ROOT, "include", "qdsim.h")).read()
    assert "int qd_eval_points(qd_handle* h, const int32_t* group_env_host, const int64_t* group_start_host, int ng," in hdr
    assert f"#define QD_POINTS_SLOTS {_lib.QD_POINTS_SLOTS}" in hdr
    assert L.qd_eval_points(None, None, None, 1, None, None, None, None, None, None) == _lib.QD_ERR_ARG   # no crash


def _handle(L, N, R, B, flags=0, qconfig=None):
    from qadapt_hip.vec_env import make_qd_config
    cfg = make_qd_config(DM.load_yaml(None, "env_config.yaml"), qconfig or DM.load_yaml(None, "qarray_config.yaml"), N, R, B,
                         flags=flags)
    h = ctypes.c_void_p()
    L.qd_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    if not h:
        pytest.fail("qd_create handed out no handle")
    return h


def test_eval_points_argument_checks_need_no_device():
    """Without a GPU qd_create fails with QD_ERR_HIP and still hands out the partial handle (qdsim.h), which is all these
    checks need: each returns before anything touches the device."""
    _lib, L = _built_lib()
    B = 3
    h = _handle(L, 4, 8, B)
    one = ctypes.c_void_p(64)                      # a device pointer that is never dereferenced
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)     # noqa: E731
    i64 = lambda *v: (ctypes.c_int64 * len(v))(*v)     # noqa: E731
    call = lambda env, start, ng, vg=one, vb=one: L.qd_eval_points(h, env, start, ng, vg, vb, None, one, one, None)  # noqa: E731
    try:
        assert call(None, i64(0, 1), 1) == _lib.QD_ERR_ARG and b"group_env_host" in L.qd_last_error(h)
        assert call(i32(0), None, 1) == _lib.QD_ERR_ARG
        assert call(i32(0), i64(0, 1), 1, vg=None) == _lib.QD_ERR_ARG and b"vg_dev" in L.qd_last_error(h)
        assert call(i32(0), i64(0, 1), 1, vb=None) == _lib.QD_ERR_ARG
        assert call(i32(0), i64(0, 1), -1) == _lib.QD_ERR_ARG and b"ng < 0" in L.qd_last_error(h)
        assert call(i32(0, 1), i64(0, 5, 4), 2) == _lib.QD_ERR_ARG and b"non-decreasing" in L.qd_last_error(h)
        assert call(i32(0), i64(-1, 4), 1) == _lib.QD_ERR_ARG
        assert call(i32(0, B), i64(0, 1, 2), 2) == _lib.QD_ERR_ARG and b"env id" in L.qd_last_error(h)
        assert call(i32(-1), i64(0, 1), 1) == _lib.QD_ERR_ARG
        assert call(i32(0), i64(0), 0) == 0                                  # no group
        assert call(i32(0, 2), i64(7, 7, 7), 2) == 0                         # groups without a point
    finally:
        L.qd_destroy(h)
    # refusals by handle kind come after the argument checks and before the device as well
    hv = _handle(L, 4, 8, B, flags=_lib.QD_FLAG_VALIDATE)
    try:
        assert L.qd_eval_points(hv, i32(0), i64(0, 1), 1, one, one, None, one, one, None) == _lib.QD_ERR_STATE
        assert b"QD_FLAG_VALIDATE" in L.qd_last_error(hv)
        assert L.qd_eval_points(hv, i32(B), i64(0, 1), 1, one, one, None, one, one, None) == _lib.QD_ERR_ARG
    finally:
        L.qd_destroy(hv)
    from qadapt_hip.vec_env import override_charge_states
    q = override_charge_states(DM.load_yaml(None, "qarray_config.yaml"), "all")
    q["simulator"]["model"]["max_charge_carriers"] = 2
    hf = _handle(L, 3, 8, B, qconfig=q)
    try:
        assert L.qd_eval_points(hf, i32(0), i64(0, 1), 1, one, one, None, one, one, None) == _lib.QD_ERR_STATE
        assert b"full charge-state space" in L.qd_last_error(hf)
    finally:
        L.qd_destroy(hf)


# ------------------------------------------------------------------ the model facade on a stub backend
class StubBackend:
    """Shape-faithful stand-in for VecQuantumDeviceEnv with B = 1 that records its eval_points calls."""

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

    def eval_points(self, env_ids, vg, vb, gamma=None, outputs=("signal", "occupations")):
        vg, vb = np.array(vg), np.array(vb)
        self.calls.append(dict(env_ids=list(env_ids), vg=vg, vb=vb, gamma=gamma, outputs=tuple(outputs)))
        m = vg.shape[1]
        out = {"signal": vg[..., 0] + vb[..., 0], "occupations": np.broadcast_to(vg[..., :self.N] * 2.0, (1, m, self.N))}
        return {k: out[k] for k in outputs}


def _env(tmp_path, N=4, R=6):
    cfg = DM.load_yaml(None, "env_config.yaml")
    cfg["capacitance_model"]["update_method"] = None
    cfg["simulator"].update(num_dots=N, resolution=R)
    p = tmp_path / "env.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return QuantumDeviceEnv(config_path=str(p), backend=StubBackend(N, R))


def test_model_facade_shapes_and_peak_width(tmp_path):
    N = 4
    env = _env(tmp_path, N, 6)
    model = env.array.model
    assert hasattr(model, "cgd_full") and hasattr(model, "coulomb_peak_width")
    rng = np.random.default_rng(1)
    for lead in ((), (5,), (3, 7)):
        vg, vb = rng.normal(size=lead + (N + 1,)), rng.normal(size=lead + (N - 1,))
        signal, n_open = model.charge_sensor_open(vg, vb)
        assert signal.shape == lead + (1,) and n_open.shape == lead + (N,)
        assert signal.dtype == np.float64 and n_open.dtype == np.float64
        assert isinstance(signal, np.ndarray) and isinstance(n_open, np.ndarray)
        assert np.array_equal(signal[..., 0], vg[..., 0] + vb[..., 0])           # point by point, in order
        assert np.array_equal(n_open, vg[..., :N] * 2.0)
        call = env._b.calls[-1]
        assert call["env_ids"] == [0] and call["vg"].shape == (1, int(np.prod(lead, dtype=int)), N + 1)
        assert call["vb"].shape == (1, int(np.prod(lead, dtype=int)), N - 1)
        assert call["outputs"] == ("signal", "occupations")
        assert np.array_equal(model.ground_state_open(vg, vb), n_open)
        assert env._b.calls[-1]["outputs"] == ("occupations",)              # no second solve for a signal nobody reads
    # the peak width is read at call time, as the reference's _get_obs assigns it (qarray_base_class.py:196)
    model.coulomb_peak_width = 0.37
    model.charge_sensor_open(np.zeros(N + 1), np.zeros(N - 1))
    assert env._b.calls[-1]["gamma"] == 0.37
    model.coulomb_peak_width = 0.21
    model.ground_state_open(np.zeros((2, N + 1)), np.zeros((2, N - 1)))
    assert env._b.calls[-1]["gamma"] == 0.21
    assert env.current_step == 0                                               # no step was counted


def test_model_facade_refusals(tmp_path):
    N = 4
    env = _env(tmp_path, N, 6)
    model = env.array.model
    with pytest.raises(NotImplementedError, match="model.tc"):
        model.charge_sensor_open(np.zeros(N + 1))
    with pytest.raises(NotImplementedError, match="2N columns"):
        model.ground_state_open(np.zeros(N + 1), None)
    with pytest.raises(ValueError):
        model.charge_sensor_open(np.zeros(N), np.zeros(N - 1))
    with pytest.raises(ValueError):
        model.charge_sensor_open(np.zeros((3, N + 1)), np.zeros((2, N - 1)))
    assert env._b.calls == []
