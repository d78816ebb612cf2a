"""The host-side request path of the stateless queries without a GPU: (a) every refusal of the fourteen C entry points that is found
before the device is touched -- return code and the WHOLE qd_last_error text -- on handles that never reached a device, as
test_host_closed_api.py::test_argument_checks_need_no_device does it; (b) the pure helpers of vec_env.py that the scans and
eval_points share.  The texts below are those of the library before its entry points were moved onto one request value; the
table passes against that library and against the present one (QDSIM_LIB selects the library).

Out of reach here, and covered by the GPU suites: the refusals that read the device (n_charge_dev, kT_dev, the capacitance
model on grids).  qd_probe_ex has no refusal of the full charge-state space."""
import ctypes
import os

import numpy as np
import pytest
import torch

from qadapt_hip import _lib
from qadapt_hip import device_model as DM
from qadapt_hip import vec_env as VE

ARG, STATE = _lib.QD_ERR_ARG, _lib.QD_ERR_STATE
ONE = ctypes.c_void_p(64)                              # a device pointer that is never dereferenced
N, R, B = 4, 8, 3


def i32(*v):
    return (ctypes.c_int32 * len(v))(*v)


def i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def f64(*v):
    return (ctypes.c_double * len(v))(*v)


class O:
    """An option struct of a row, built when the row runs: its class by name, struct_size right unless the row sets it."""

    def __init__(self, cls, **fields):
        self.cls, self.fields = cls, fields

    def build(self):
        cls = getattr(_lib, self.cls)
        return cls(**{"struct_size": ctypes.sizeof(cls), **self.fields})


# the arguments of every entry point between the handle and the stream, and a call that passes every check made without a device
SCAN = ["env", "nq", "second", "range", "gate", "barrier", "sensor", "raw", "image", "plohi", "opts"]
GRID = ["env", "nq", "nx", "ny", "second", "range", "gate", "barrier", "sensor"]
POINTS = ["genv", "gstart", "ng", "vg", "vb"]
ARGS = {
    "qd_probe_ex": ["env", "nq", "gate", "barrier", "sensor", "window", "raw", "image", "plohi", "opts"],
    "qd_scan2d": SCAN,
    "qd_scan_affine": SCAN,
    "qd_scan1d": ["env", "nq", "n_points", "second", "range", "gate", "barrier", "sensor", "raw", "image", "plohi", "opts"],
    "qd_scan_grid": GRID + ["raw", "image", "plohi", "opts"],
    "qd_scan_grid_closed": GRID + ["n_charge", "raw", "image", "plohi", "opts"],
    "qd_scan_grid_thermal": GRID + ["kT", "raw", "image", "plohi", "opts", "own"],
    "qd_scan_grid_response": GRID + ["kT", "raw", "image", "plohi", "opts", "own"],
    "qd_scan_grid_levels": GRID + ["raw", "image", "plohi", "opts", "own"],
    "qd_eval_points": POINTS + ["gamma", "signal", "occ"],
    "qd_eval_points_closed": POINTS + ["gamma", "n_charge", "signal", "occ", "states"],
    "qd_eval_points_ex": POINTS + ["signal", "occ", "opts"],
    "qd_eval_points_thermal": POINTS + ["kT", "signal", "occ", "opts"],
    "qd_eval_points_response": POINTS + ["kT", "signal", "occ", "opts"],
}
GOOD_SCAN = dict(env=ONE, nq=1, n_points=4, nx=4, ny=2, second=ONE, range=ONE, gate=ONE, barrier=ONE, sensor=None, window=None,
                 n_charge=ONE, kT=ONE, raw=ONE, image=None, plohi=None, opts=None, own=None)
GOOD_POINTS = dict(genv=i32(0), gstart=i64(0, 1), ng=1, vg=ONE, vb=ONE, gamma=None, n_charge=i32(1), kT=f64(0.01), signal=ONE, occ=ONE,
                   states=None, opts=None)
LEVELS = O("QdGridLevelsOpts", n_levels=2, levels_dst=64)
GOOD = {name: dict(GOOD_POINTS if name.startswith("qd_eval") else GOOD_SCAN) for name in ARGS}
GOOD["qd_scan_grid_levels"]["own"] = LEVELS

# entry point -> (its second array, the class of its options, their C name, what it renders)
SCANS = {
    "qd_scan2d": ("axes_dev", "QdScanOpts", "qd_scan_opts", "scan"),
    "qd_scan_affine": ("dir_dev", "QdScanAffineOpts", "qd_scan_affine_opts", "scan"),
    "qd_scan1d": ("dir_dev", "QdScan1dOpts", "qd_scan1d_opts", "line"),
    "qd_scan_grid": ("dir_dev", "QdScanGridOpts", "qd_scan_grid_opts", "grid"),
    "qd_scan_grid_closed": ("dir_dev", "QdScanGridOpts", "qd_scan_grid_opts", "grid"),
    "qd_scan_grid_thermal": ("dir_dev", "QdScanGridOpts", "qd_scan_grid_opts", "grid"),
    "qd_scan_grid_response": ("dir_dev", "QdScanGridOpts", "qd_scan_grid_opts", "grid"),
    "qd_scan_grid_levels": ("dir_dev", "QdScanGridOpts", "qd_scan_grid_opts", "grid"),
}
# the options of its own that carry a grid call's total charges: (class, fields of a good one)
OWN = {"qd_scan_grid_thermal": ("QdGridThermalOpts", {}), "qd_scan_grid_response": ("QdGridResponseOpts", {}),
       "qd_scan_grid_levels": ("QdGridLevelsOpts", LEVELS.fields)}
POINT_CALLS = ["qd_eval_points", "qd_eval_points_closed", "qd_eval_points_ex", "qd_eval_points_thermal", "qd_eval_points_response"]
# how each points call is given the total charges of its groups
POINTS_CHARGE = {"qd_eval_points_closed": lambda q: dict(n_charge=q),
                 "qd_eval_points_ex": lambda q: dict(opts=O("QdPointsOpts", n_charge_host=q)),
                 "qd_eval_points_thermal": lambda q: dict(opts=O("QdThermalOpts", n_charge_host=q)),
                 "qd_eval_points_response": lambda q: dict(opts=O("QdResponseOpts", n_charge_host=q))}

ROWS = []                                              # (entry point, handle, arguments that differ from the good call, code, text)


def row(name, code, text, handle="plain", **over):
    ROWS.append((name, handle, over, code, text))


# ---- qd_probe_ex (its texts say qd_probe for what qd_probe refuses too)
row("qd_probe_ex", ARG, "null handle", handle="null")
row("qd_probe_ex", ARG, "qd_probe: nq < 0", nq=-1)
row("qd_probe_ex", ARG, "qd_probe: env_of_query_dev is NULL", env=None)
row("qd_probe_ex", ARG, "qd_probe: gate_v_dev or barrier_v_dev is NULL", gate=None)
row("qd_probe_ex", ARG, "qd_probe: gate_v_dev or barrier_v_dev is NULL", barrier=None)
row("qd_probe_ex", ARG, "qd_probe_ex: opts->struct_size is not sizeof(qd_probe_opts)", opts=O("QdProbeOpts", struct_size=24))
row("qd_probe_ex", ARG, "qd_probe_ex: opts->noise_flags has a bit that is no QD_NOISE_* stage", opts=O("QdProbeOpts", noise_flags=8))
row("qd_probe_ex", STATE, "qd_probe: a QD_FLAG_VALIDATE handle keeps records, occupations and eigenvalues of its B envs' last observe "
    "and renders no probes; use a handle without the flag", handle="validate")
row("qd_probe_ex", ARG, "qd_probe: nq < 0", handle="validate", nq=-1)
row("qd_probe_ex", 0, None, nq=0)
row("qd_probe_ex", 0, None, nq=0, opts=O("QdProbeOpts", noise_flags=_lib.QD_NOISE_SENSOR | _lib.QD_NOISE_RADIAL | _lib.QD_NOISE_LATCH))

# ---- the scans: qd_scan2d, qd_scan_affine, qd_scan1d and the five grids
for who, (second, cls, ctype, what) in SCANS.items():
    grid, thermal = who.startswith("qd_scan_grid"), who in ("qd_scan_grid_thermal", "qd_scan_grid_response")
    row(who, ARG, "null handle", handle="null")
    row(who, ARG, f"{who}: nq < 0", nq=-1)
    for null in ("env", "second", "range"):
        row(who, ARG, f"{who}: env_of_query_dev, {second} or range_dev is NULL", **{null: None})
    for null in ("gate", "barrier"):
        row(who, ARG, f"{who}: gate_v_dev or barrier_v_dev is NULL", **{null: None})
    if who == "qd_scan1d":
        for n in (0, -3, R * R + 1):
            row(who, ARG, "qd_scan1d: n_points must be in 1..P (P = resolution^2 of the handle)", n_points=n)
    if grid:
        for nx, ny in ((0, 2), (4, 0), (-1, -1), (9, 8), (R * R + 1, 1)):
            row(who, ARG, f"{who}: nx and ny must be >= 1 with nx*ny <= P (P = resolution^2 of the handle)", nx=nx, ny=ny)
    row(who, ARG, f"{who}: opts->struct_size is not sizeof({ctype})", opts=O(cls, struct_size=48))
    for frame in (2, -1):
        row(who, ARG, f"{who}: opts->frame is neither QD_SCAN_VIRTUAL nor QD_SCAN_PHYSICAL", opts=O(cls, frame=frame))
    row(who, ARG, f"{who}: vgm_dev has no meaning in the physical frame", opts=O(cls, frame=_lib.QD_SCAN_PHYSICAL, vgm_dev=64))
    for bits in (_lib.QD_NOISE_RADIAL, 8, _lib.QD_NOISE_SENSOR | _lib.QD_NOISE_RADIAL):
        row(who, ARG, f"{who}: noise_flags takes QD_NOISE_SENSOR and QD_NOISE_LATCH only (the radial stage is centred on the env's "
            "own adjacent-pair observation)", opts=O(cls, noise_flags=bits))
    if thermal:
        for bits in (_lib.QD_NOISE_LATCH, _lib.QD_NOISE_LATCH | _lib.QD_NOISE_SENSOR):
            row(who, ARG, f"{who}: QD_NOISE_LATCH has no thermal form: the latching model holds an integer configuration, a thermal "
                "mean has none", opts=O(cls, noise_flags=bits))
    if who != "qd_scan_grid" and grid:                 # noise in the closed regime, however the call is given its charges
        charges = dict(n_charge=ONE) if who == "qd_scan_grid_closed" else dict(own=O(OWN[who][0], n_charge_dev=64, **OWN[who][1]))
        row(who, ARG, f"{who}: the closed regime has no noise stages: noise_flags must be 0",
            opts=O(cls, noise_flags=_lib.QD_NOISE_SENSOR), **charges)
    row(who, STATE, f"{who}: a QD_FLAG_VALIDATE handle keeps records, occupations and eigenvalues of its B envs' last observe and "
        f"renders no {what}s; use a handle without the flag", handle="validate")
    row(who, STATE, f"{who}: the full charge-state space synthesises its own voltages (qd_k_full_structure); a {what} front end for "
        "it is not built", handle="full")
    row(who, ARG, f"{who}: nq < 0", handle="validate", nq=-1)                          # arguments before the handle's state
    row(who, ARG, f"{who}: opts->struct_size is not sizeof({ctype})", handle="full", opts=O(cls, struct_size=0))
    row(who, 0, None, nq=0)
row("qd_scan_grid_closed", ARG, "qd_scan_grid_closed: n_charge_dev is NULL", n_charge=None)
row("qd_scan_grid_closed", ARG, "qd_scan_grid_closed: n_charge_dev is NULL", n_charge=None, nq=-1)     # (its first check)
row("qd_scan_grid_thermal", ARG, "qd_scan_grid_thermal: kT_dev is NULL", kT=None)
row("qd_scan_grid_thermal", ARG, "qd_scan_grid_thermal: topts->struct_size is not sizeof(qd_grid_thermal_opts)",
    own=O("QdGridThermalOpts", struct_size=40))
row("qd_scan_grid_response", ARG, "qd_scan_grid_response: kT_dev is NULL", kT=None)
row("qd_scan_grid_response", ARG, "qd_scan_grid_response: ropts->struct_size is not sizeof(qd_grid_response_opts)",
    own=O("QdGridResponseOpts", struct_size=32))
row("qd_scan_grid_levels", ARG, "qd_scan_grid_levels: lopts is NULL", own=None)
row("qd_scan_grid_levels", ARG, "qd_scan_grid_levels: lopts->struct_size is not sizeof(qd_grid_levels_opts)",
    own=O("QdGridLevelsOpts", struct_size=24, **LEVELS.fields))
for levels in (0, -1, 9):
    row("qd_scan_grid_levels", ARG, "qd_scan_grid_levels: n_levels must be in 1..QD_LEVELS_MAX (8)",
        own=O("QdGridLevelsOpts", n_levels=levels, levels_dst=64))
row("qd_scan_grid_levels", ARG, "qd_scan_grid_levels: levels_dst is NULL", own=O("QdGridLevelsOpts", n_levels=2))
row("qd_scan_grid_levels", ARG, "qd_scan_grid_levels: levels_dst is NULL", handle="validate", own=O("QdGridLevelsOpts", n_levels=2))

# ---- the points
for who in POINT_CALLS:
    row(who, ARG, "null handle", handle="null")
    row(who, ARG, f"{who}: ng < 0", ng=-1)
    for null in ("genv", "gstart"):
        row(who, ARG, f"{who}: group_env_host or group_start_host is NULL", **{null: None})
    for null in ("vg", "vb"):
        row(who, ARG, f"{who}: vg_dev or vb_dev is NULL", **{null: None})
    row(who, ARG, f"{who}: group_start is negative", gstart=i64(-1, 1))
    row(who, ARG, f"{who}: group_start is not non-decreasing", gstart=i64(2, 1))
    two = dict(genv=i32(0, 1), ng=2, **(dict(kT=f64(0.01, 0.01)) if "kT" in ARGS[who] else {}))    # (one temperature per group)
    row(who, ARG, f"{who}: group_start is not non-decreasing", gstart=i64(0, 3, 2), **two)
    for env in (B, -1):
        row(who, ARG, f"{who}: env id out of range", genv=i32(env))
    if who in POINTS_CHARGE:
        for q in (-1, 32768):
            row(who, ARG, f"{who}: n_charge must be in 0..32767", **POINTS_CHARGE[who](i32(q)))
        row(who, ARG, f"{who}: n_charge must be in 0..32767", gstart=i64(0, 1, 2), **two, **POINTS_CHARGE[who](i32(2, -3)))
    row(who, STATE, f"{who}: a QD_FLAG_VALIDATE handle keeps records, occupations and eigenvalues of its B envs' last observe and "
        "evaluates no points; use a handle without the flag", handle="validate")
    row(who, STATE, f"{who}: the full charge-state space synthesises its own voltages (qd_k_full_structure); a point front end for "
        "it is not built yet", handle="full")
    row(who, ARG, f"{who}: env id out of range", handle="validate", genv=i32(B))        # arguments before the handle's state
    row(who, ARG, f"{who}: ng < 0", handle="full", ng=-1)
    row(who, 0, None, ng=0)
    row(who, 0, None, gstart=i64(3, 3))                                                # a group without a point
row("qd_eval_points_closed", ARG, "qd_eval_points_closed: n_charge_host is NULL", n_charge=None)
row("qd_eval_points_ex", ARG, "qd_eval_points_ex: opts->struct_size is not sizeof(qd_points_opts)", opts=O("QdPointsOpts", struct_size=40))
for levels in (-1, 9):
    row("qd_eval_points_ex", ARG, "qd_eval_points_ex: opts->n_levels must be in 0..QD_LEVELS_MAX (8)",
        opts=O("QdPointsOpts", n_levels=levels, levels_dst=64))
row("qd_eval_points_ex", ARG, "qd_eval_points_ex: opts->n_levels > 0 needs opts->levels_dst", opts=O("QdPointsOpts", n_levels=2))
row("qd_eval_points_ex", ARG, "qd_eval_points_ex: opts->states_dst is an output of the closed regime and needs opts->n_charge_host",
    opts=O("QdPointsOpts", states_dst=64))
row("qd_eval_points_ex", ARG, "qd_eval_points_ex: opts->n_levels > 0 needs opts->levels_dst", handle="validate",
    opts=O("QdPointsOpts", n_levels=2))
for who, cls, ctype in (("qd_eval_points_thermal", "QdThermalOpts", "qd_thermal_opts"),
                        ("qd_eval_points_response", "QdResponseOpts", "qd_response_opts")):
    row(who, ARG, f"{who}: kT_host is NULL", kT=None)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        row(who, ARG, f"{who}: kT must be finite and > 0", kT=f64(bad))
    row(who, ARG, f"{who}: kT must be finite and > 0", genv=i32(0, 1), gstart=i64(0, 1, 2), ng=2, kT=f64(0.01, 0.0))
    row(who, ARG, f"{who}: kT must be finite and > 0", handle="validate", kT=f64(0.0))
    row(who, ARG, f"{who}: kT must be finite and > 0", vg=None, kT=f64(-2.0))           # (the temperatures before the arrays)
    row(who, ARG, f"{who}: opts->struct_size is not sizeof({ctype})", opts=O(cls, struct_size=8))


def _handle(L, n_dot, flags=0, qconfig=None):
    cfg = VE.make_qd_config(DM.load_yaml(None, "env_config.yaml"), qconfig or DM.load_yaml(None, "qarray_config.yaml"), n_dot, R, B,
                            flags=flags)
    h = ctypes.c_void_p()
    L.qd_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    if not h:
        pytest.fail("qd_create handed out no handle")
    return h


@pytest.fixture(scope="module")
def handles():
    """the library and the three handles of test_host_closed_api.py: N = 4, and N = 3 with QD_FLAG_VALIDATE and in the full space"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is missing: run __graft_entry__.build() before the tests (no test compiles it)")
    L = _lib.lib()
    full = VE.override_charge_states(DM.load_yaml(None, "qarray_config.yaml"), "all")
    full["simulator"]["model"]["max_charge_carriers"] = 2
    hs = {"null": None, "plain": _handle(L, N), "validate": _handle(L, 3, flags=_lib.QD_FLAG_VALIDATE), "full": _handle(L, 3, qconfig=full)}
    yield L, hs
    for h in hs.values():
        if h:
            L.qd_destroy(h)


def test_the_table_covers_every_entry_point():
    assert {r[0] for r in ROWS} == set(ARGS) and len(ARGS) == 14
    for name in ARGS:
        kinds = {r[1] for r in ROWS if r[0] == name}
        assert kinds == ({"null", "plain", "validate"} if name == "qd_probe_ex" else {"null", "plain", "validate", "full"}), name
        assert any(r[1] == "validate" and r[3] == ARG for r in ROWS if r[0] == name), name           # the order of the checks
        assert any(r[3] == 0 for r in ROWS if r[0] == name), name
    sizes = {r[4] for r in ROWS if r[4] and "struct_size" in r[4]}
    assert len(sizes) == 1 + len(SCANS) + 3 + 3                                        # eight checks in the C file, fifteen texts


@pytest.mark.parametrize("name,handle,over,code,text", ROWS, ids=[f"{i}-{r[0]}-{r[1]}" for i, r in enumerate(ROWS)])
def test_refusals_need_no_device(handles, name, handle, over, code, text):
    L, hs = handles
    h = hs[handle]
    assert not set(over) - set(ARGS[name]), (name, over)                               # a row names arguments its call has
    args = {**GOOD[name], **over}
    keep = {k: v.build() for k, v in args.items() if isinstance(v, O)}                  # (alive over the call)
    values = [ctypes.byref(keep[k]) if k in keep else args[k] for k in ARGS[name]]
    if h and code:                                                                     # (so that the text below is this row's)
        assert L.qd_load_episodes(h, None, 0, None, None, 0, None) == ARG and L.qd_last_error(h) == b"qd_load_episodes: bad argument"
    rc = getattr(L, name)(h, *values, None)
    assert rc == code, (rc, L.qd_last_error(h))
    if text is not None:
        assert L.qd_last_error(h).decode() == text


# ------------------------------------------------------------------ the helpers of vec_env.py
SENSOR, RADIAL, LATCH = _lib.QD_NOISE_SENSOR, _lib.QD_NOISE_RADIAL, _lib.QD_NOISE_LATCH


def test_scan_noise_flags():
    assert (SENSOR, RADIAL, LATCH) == (1, 2, 4)
    for env_flags in range(8):                                                         # an env created with each subset of stages
        for none in (None, False, (), []):
            assert VE.scan_noise_flags(none, env_flags, "grids") == 0
        assert VE.scan_noise_flags(True, env_flags, "lines") == env_flags & ~RADIAL
        for names, flags in (((), 0), (("sensor",), SENSOR), (("latch",), LATCH), (("sensor", "latch"), SENSOR | LATCH),
                             (["latch", "sensor"], SENSOR | LATCH), ({"sensor"}, SENSOR)):
            assert VE.scan_noise_flags(names, env_flags, "axis scans") == flags
    for family in ("axis scans", "lines", "grids"):
        for names in (("radial",), ("sensor", "radial"), ["radial", "latch"], ("sensor", "radial", "latch")):
            with pytest.raises(ValueError) as ei:
                VE.scan_noise_flags(names, SENSOR | RADIAL | LATCH, family)
            assert str(ei.value) == f"radial noise is centred on the env's own adjacent-pair observation: not defined for {family}"
    with pytest.raises(KeyError):
        VE.scan_noise_flags(("telegraph",), 0, "grids")


def test_check_scan_frame():
    for frame, vgm in (("virtual", None), ("physical", None), ("virtual", np.eye(5)[None])):
        VE.check_scan_frame(frame, vgm)
    with pytest.raises(ValueError) as ei:
        VE.check_scan_frame("other", None)
    assert str(ei.value) == "frame must be 'virtual' or 'physical', got 'other'"
    with pytest.raises(ValueError) as ei:
        VE.check_scan_frame("physical", np.eye(5)[None])
    assert str(ei.value) == "vgm has no meaning in the physical frame"


def test_scan_ranges():
    r = VE.scan_ranges((0.0, 1.0), (3, 2), 3)
    assert r.shape == (3, 4) and r.dtype == np.float64 and np.array_equal(r, [[0, 1, 3, 2]] * 3)
    x, y = np.arange(6.0).reshape(3, 2), -np.arange(6.0).reshape(3, 2)
    assert np.array_equal(VE.scan_ranges(x, y, 3), np.concatenate([x, y], axis=1))
    assert np.array_equal(VE.scan_ranges(x, (7, 8), 3)[:, 2:], [[7, 8]] * 3)
    for bad in (np.zeros((2, 2)), (0.0, 1.0, 2.0), np.zeros((3, 3))):
        with pytest.raises(ValueError):
            VE.scan_ranges(bad, (0, 1), 3)
        with pytest.raises(ValueError):
            VE.scan_ranges((0, 1), bad, 3)


def test_host_vector():
    for x in (0.5, np.float32(0.5), [0.5, 0.5, 0.5], np.full(3, 0.5), torch.full((3,), 0.5), torch.tensor(0.5, dtype=torch.float32),
              np.full(6, 0.5)[::2]):
        v = VE.host_vector(x, 3)
        assert isinstance(v, np.ndarray) and v.shape == (3,) and v.dtype == np.float64 and v.flags["C_CONTIGUOUS"]
        assert np.array_equal(v, [0.5] * 3)
    assert VE.host_vector(torch.arange(4), 4).tolist() == [0.0, 1.0, 2.0, 3.0]
    assert VE.host_vector(2.0, 0).shape == (0,)
    for bad in ([1.0, 2.0], np.zeros(4), torch.zeros(2), np.zeros((3, 1))):
        with pytest.raises(ValueError):
            VE.host_vector(bad, 3)


def test_host_kT():
    assert VE.host_kT(0.02, 2).tolist() == [0.02, 0.02] and VE.host_kT(torch.tensor([0.01, 0.03], dtype=torch.float64), 2).tolist() == [0.01, 0.03]
    for bad, got in ((0, "0"), (0.0, "0.0"), (-1.0, "-1.0"), (float("inf"), "inf"), (float("nan"), "nan"), ([0.01, 0.0], "[0.01, 0.0]"),
                     ([np.inf, 0.01], "[inf, 0.01]")):
        with pytest.raises(ValueError) as ei:
            VE.host_kT(bad, 2)
        assert str(ei.value) == f"kT must be finite and > 0, got {got}"
    with pytest.raises(ValueError):
        VE.host_kT([0.01, 0.02, 0.03], 2)
