"""
VecQuantumDeviceEnv -- B quantum-dot tuning environments stepped as one batch on
one MI355X.  Host side of the C-ABI in include/qdsim.h; observation / action
buffers are PyTorch-ROCm tensors, the computation is the HIP library.

Semantics per env are those of the reference's QuantumDeviceEnv
(src/qadapt/environment/env.py:135-315): reset() builds a new random device,
identity VGM, ground truth, voltage ranges, random start, first observation and
a Kalman/VGM update; step() rescales the action, pays the reward against the
PREVIOUS ground truth, renders the N-1 CSD channels, normalises them, updates
Kalman/VGM and then the ground truth.  The capacitance CNN (env.py:568-581) is
an input provider here: pass `capacitance_model=callable`, or
`update_method: null` in the env config, or per-step `cnn_outputs`.
"""
from __future__ import annotations

import ctypes
import re

import numpy as np
import torch

from . import _lib
from .device_model import DeviceSampler, check_solver_options, load_yaml, max_charge_carriers
from .layout import layout


class SyntheticCapacitanceModel:
    """Stand-in for the capacitance CNN used by benchmarks and tests
    (values ~ N(0, 0.1^2), log_vars ~ U(-6, -2)); deterministic
    per (seed, call index)."""

    def __init__(self, seed=99, outputs=3):
        self.seed = seed
        self.calls = 0
        self.outputs = outputs

    def __call__(self, images):
        n = images.shape[0]
        g = torch.Generator(device="cpu").manual_seed(self.seed + self.calls)
        self.calls += 1
        values = torch.randn((n, self.outputs), generator=g, dtype=torch.float32) * 0.1
        log_vars = torch.rand((n, self.outputs), generator=g, dtype=torch.float32) * 4.0 - 6.0
        return values.to(images.device), log_vars.to(images.device)


def device_state_from_rows(L, st, params, steps):
    """The reference's info["current_device_state"] (env.py:214-222) for host rows of state blocks `st` (n, L.s_size),
    parameter blocks `params` (n, L.size) and step counters `steps` (n,): ground truths float32, voltages float64."""
    N, G = L.N, L.N + 1
    return {"gate_ground_truth": st[:, L.s_gate_gt:L.s_gate_gt + N].astype(np.float32),
            "barrier_ground_truth": st[:, L.s_barrier_gt:L.s_barrier_gt + N - 1].astype(np.float32),
            "sensor_ground_truth": st[:, L.s_sensor_gt].copy(),
            "current_gate_voltages": st[:, L.s_gate_v:L.s_gate_v + N].copy(),
            "current_barrier_voltages": st[:, L.s_barrier_v:L.s_barrier_v + N - 1].copy(),
            "virtual_gate_matrix": st[:, L.s_vgm:L.s_vgm + G * G].reshape(-1, G, G).copy(),
            "virtual_gate_origin": params[:, L.origin:L.origin + G].copy(),
            "kalman_means": st[:, L.s_kmean:L.s_kmean + N * N].reshape(-1, N, N).copy(),
            "kalman_variances": st[:, L.s_kvar:L.s_kvar + N * N].reshape(-1, N, N).copy(),
            "steps": steps}


def cgd_full_from_params(L, params):
    """(n, N+1, 2N) float64: the devices' cgd_full (the reference's array.model.cgd_full) from parameter block rows."""
    return params[:, L.cgd:L.cgd + L.G * L.V].reshape(-1, L.G, L.V).copy()


def override_charge_states(qconfig, num_charge_states):
    """The num_charge_states= constructor override applied to a loaded qarray config: None keeps the file's value, "all"
    writes an explicit null (the full charge-state space), anything else is written as given (checked later)."""
    if num_charge_states is not None:
        qconfig["simulator"].setdefault("latched_model", {})["num_charge_states"] = \
            None if num_charge_states == "all" else num_charge_states
    return qconfig


def make_qd_config(config, qconfig, num_dots, resolution, batch, *, env_chunk=0, flags=0, noise_flags=0, seed=0,
                   env_id_offset=0):
    """The qd_config (include/qdsim.h) of a handle for the env config `config` and the qarray config `qconfig` (both as
    loaded by load_yaml); builds no handle and needs no GPU.  The kept-state count K comes from
    `qconfig.simulator.latched_model.num_charge_states` (check_solver_options); an explicit null there selects the full
    charge-state space, encoded as -max_charge_carriers (QD_ALL_CHARGE_STATES in qdsim.h)."""
    sim, rew, cm = config["simulator"], config["reward"], config["capacitance_model"]
    nearest = bool(cm.get("nearest_neighbour"))
    k = check_solver_options(qconfig, n_dot=num_dots)
    ncs = k if k is not None else -max_charge_carriers(qconfig)
    return _lib.QdConfig(struct_size=ctypes.sizeof(_lib.QdConfig), n_dot=int(num_dots), resolution=int(resolution),
                         batch=int(batch), max_steps=int(sim["max_steps"]), env_chunk=int(env_chunk), flags=int(flags),
                         noise_flags=int(noise_flags),
                         gate_ramp_start=float(rew["gate_ramp_start"]),
                         gate_quadratic_start=float(rew["gate_quadratic_start"]),
                         barrier_ramp_start=float(rew["barrier_ramp_start"]),
                         kalman_prior_mean=0.3, kalman_prior_variance=0.5, kalman_prior_mean_nnn=0.15,
                         kalman_variance_threshold=float(cm.get("variance_threshold", 0.05)),
                         kalman_process_noise=float(cm.get("process_noise", 0.0)),
                         rng_seed=int(seed) & 0xFFFFFFFFFFFFFFFF, env_id_offset=int(env_id_offset),
                         use_deltas=1 if sim.get("use_deltas") else 0,
                         sparse_reward=1 if rew.get("sparse_reward") else 0,
                         gate_curve_type=_lib.QD_CURVES[rew.get("gate_curve_type", "constant")],
                         update_method=_lib.QD_UPDATE_DIRECT if cm["update_method"] == "direct" else _lib.QD_UPDATE_KALMAN,
                         cnn_outputs=2 if nearest else 3, num_charge_states=ncs,
                         delta_max=float(sim.get("delta_max", 0.0)),
                         gate_curve_exponent=float(rew.get("gate_curve_exponent", 2.0)),
                         plunger_radius=float(rew.get("plunger_radius", 0.0)),
                         outer_plunger_radius=float(rew.get("outer_plunger_radius", 0.0)),
                         outer_plunger_reward_max=float(rew.get("outer_plunger_reward_max", 0.0)),
                         barrier_radius=float(rew.get("barrier_radius", 0.0)))


def scan_control_index(name, N, frame="virtual"):
    """Index of one swept control of scan2d in the order of the model's voltage vector: 0..N-1 the plungers, N the sensor
    gate, N+1..2N-1 the barriers.  `name` is such an index, or a name, 1-indexed as the reference's GateVoltageComposer
    names its gates: "vP1".."vPN" in the virtual frame ("P1".."PN" in the physical frame), "S", "B1".."B{N-1}"."""
    if isinstance(name, (int, np.integer)):
        i = int(name)
        if not 0 <= i < 2 * N:
            raise ValueError(f"control index {i} outside [0, {2 * N})")
        return i
    if not isinstance(name, str):
        raise TypeError(f"a control is an index or a name, got {type(name).__name__}")
    if name == "S":
        return N
    plunger = "vP" if frame == "virtual" else "P"
    other = "P" if frame == "virtual" else "vP"
    for prefix, base, count in ((plunger, 0, N), ("B", N + 1, N - 1)):
        if name.startswith(prefix) and name[len(prefix):].isdigit():
            k = int(name[len(prefix):])
            if not 1 <= k <= count:
                raise ValueError(f"{name!r}: {prefix}1..{prefix}{count} exist for {N} dots")
            return base + k - 1
    if name.startswith(other) and name[len(other):].isdigit():
        raise ValueError(f"{name!r} is a plunger of the {'physical' if frame == 'virtual' else 'virtual'} frame; "
                         f"the {frame} frame names its plungers {plunger}1..{plunger}{N}")
    raise ValueError(f"unknown control {name!r}: expected {plunger}1..{plunger}{N}, S or B1..B{N - 1}")


def scan_control_indices(x, N, frame, nq):
    """(nq,) int32 control indices from one index / name for all queries or a sequence of nq of them."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(x, (str, int, np.integer)):
        return np.full(nq, scan_control_index(x, N, frame), np.int32)
    idx = np.array([scan_control_index(v, N, frame) for v in list(x)], np.int32)
    if idx.shape != (nq,):
        raise ValueError(f"{len(idx)} controls for {nq} queries")
    return idx


_COMBINATION_AXIS = re.compile(r"^([eU])(\d+)_(\d+)$")


def scan_axis_vector(axis, N, frame="virtual"):
    """(2N,) float64 direction of one axis of scan_affine over the controls in the order of the model's voltage vector
    (0..N-1 the plungers, N the sensor gate, N+1..2N-1 the barriers).  `axis` is
      a control index or name, as scan_control_index takes them: the unit vector of that control;
      "e{i}_{j}": detuning, +1 on plunger i and -1 on plunger j; "U{i}_{j}": the on-site axis, 1/sqrt(2) on both plungers --
          1-indexed and unnormalised exactly as the reference's GateVoltageComposer builds them (v_i - v_j and
          (v_i + v_j) / sqrt(2), GateVoltageComposer.py:66-82); the plungers are virtual or physical by `frame`;
      a {control: coefficient} dict, its controls indices or names (coefficients of a control named twice add up);
      a (2N,) sequence of numbers: the vector itself."""
    if isinstance(axis, str):
        m = _COMBINATION_AXIS.match(axis)
        if m:
            i, j = int(m.group(2)), int(m.group(3))
            if not (1 <= i <= N and 1 <= j <= N):
                raise ValueError(f"{axis!r}: the dots of a combination axis are 1..{N} for {N} dots")
            if i == j:
                raise ValueError(f"{axis!r}: a combination axis needs two different dots")
            v = np.zeros(2 * N)
            if m.group(1) == "e":
                v[i - 1], v[j - 1] = 1.0, -1.0
            else:
                v[i - 1] = v[j - 1] = 1.0 / np.sqrt(2.0)
            return v
    if isinstance(axis, (str, int, np.integer)):
        v = np.zeros(2 * N)
        v[scan_control_index(axis, N, frame)] = 1.0
        return v
    if isinstance(axis, dict):
        v = np.zeros(2 * N)
        for name, c in axis.items():
            v[scan_control_index(name, N, frame)] += float(c)
        return v
    if isinstance(axis, torch.Tensor):
        axis = axis.detach().cpu().numpy()
    v = np.asarray(axis, np.float64)
    if v.shape != (2 * N,):
        raise ValueError(f"an axis vector has one coefficient per control, shape ({2 * N},); got {v.shape}")
    return v.copy()


def scan_axis_vectors(axis, N, frame, nq):
    """(nq, 2N) float64 directions: one axis for all queries (anything scan_axis_vector takes), an (nq, 2N) array, or a
    list of nq axes that are not all plain numbers (names, dicts, vectors)."""
    if isinstance(axis, torch.Tensor):
        axis = axis.detach().cpu().numpy()
    if isinstance(axis, (list, tuple)) and not all(isinstance(a, (int, float, np.integer, np.floating)) for a in axis):
        rows = [scan_axis_vector(a, N, frame) for a in axis]
        if len(rows) != nq:
            raise ValueError(f"{len(rows)} axes for {nq} queries")
        return np.stack(rows)
    if isinstance(axis, np.ndarray) and axis.ndim == 2:
        if axis.shape != (nq, 2 * N):
            raise ValueError(f"per-query axis vectors have shape ({nq}, {2 * N}); got {axis.shape}")
        return np.ascontiguousarray(axis, np.float64)
    return np.tile(scan_axis_vector(axis, N, frame), (nq, 1))


QD_CLOSED_QMAX = 32767


def closed_charges(n_charge, n, what):
    """n_charge of a closed query -- a scalar or one value per `what` -- as (n,) int32 on the host; integers in 0..32767"""
    a = np.asarray(n_charge.detach().cpu().numpy() if isinstance(n_charge, torch.Tensor) else n_charge)
    if a.dtype == bool or not (np.issubdtype(a.dtype, np.integer) or (np.issubdtype(a.dtype, np.floating) and np.all(a == np.rint(a)))):
        raise ValueError(f"n_charge must hold integers, got {n_charge!r}")
    if a.ndim > 1 or (a.ndim == 1 and a.size != n):
        raise ValueError(f"n_charge must be a scalar or one value per {what} ({n}), got shape {a.shape}")
    a = np.broadcast_to(a.astype(np.int64), (n,))
    if a.size and (a.min() < 0 or a.max() > QD_CLOSED_QMAX):
        raise ValueError(f"n_charge must be in 0..{QD_CLOSED_QMAX}, got {int(a.min())}..{int(a.max())}")
    return np.ascontiguousarray(a, np.int32)


def _ptr(t):
    """A device tensor's address as a pointer argument; None stays NULL."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _addr(t):
    """A device tensor's address as a pointer field of an option struct; None stays NULL."""
    return None if t is None else t.data_ptr()


def _opts(cls, **fields):
    """An option struct of _lib with its struct_size set."""
    return cls(struct_size=ctypes.sizeof(cls), **fields)


NOISE_STAGES = {"sensor": _lib.QD_NOISE_SENSOR, "radial": _lib.QD_NOISE_RADIAL, "latch": _lib.QD_NOISE_LATCH}


def check_scan_frame(frame, vgm):
    """A scan's frame is "virtual" or "physical", and only the virtual one takes a virtual gate matrix."""
    if frame not in ("virtual", "physical"):
        raise ValueError(f"frame must be 'virtual' or 'physical', got {frame!r}")
    if vgm is not None and frame == "physical":
        raise ValueError("vgm has no meaning in the physical frame")


def scan_noise_flags(noise, env_flags, family):
    """The QD_NOISE_* stages of a scan.  noise None / False / (): none.  True: those of `env_flags`, the stages the env was
    created with, without the radial one.  Or an iterable of {"sensor", "latch"}; "radial" raises, with the family's word
    ("axis scans", "lines", "grids")."""
    if noise is True:
        return env_flags & ~_lib.QD_NOISE_RADIAL
    names = tuple(noise) if noise else ()
    if "radial" in names:
        raise ValueError(f"radial noise is centred on the env's own adjacent-pair observation: not defined for {family}")
    flags = 0
    for k in names:
        flags |= NOISE_STAGES[k]
    return flags


def scan_ranges(x_range, y_range, nq):
    """(nq, 4) float64 rows (x lo, x hi, y lo, y hi) from one (lo, hi) pair for all queries or (nq, 2) per axis."""
    return np.concatenate([np.broadcast_to(np.asarray(x_range, np.float64), (nq, 2)),
                           np.broadcast_to(np.asarray(y_range, np.float64), (nq, 2))], axis=1)


def host_vector(x, n):
    """A scalar or (n,) values, numpy or torch, as a contiguous (n,) float64 array on the host."""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(
        x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, np.float64), (n,)))


def host_kT(kT, n):
    """kT of a thermal query -- a scalar or (n,) values -- as host_vector gives it; finite and > 0"""
    kth = host_vector(kT, n)
    if not (np.isfinite(kth).all() and (kth > 0).all()):
        raise ValueError(f"kT must be finite and > 0, got {kT!r}")
    return kth


class VecQuantumDeviceEnv:
    def __init__(self, num_envs, num_dots=None, config_path=None, qarray_config_path=None,
                 resolution=None, device=None, seed=None, env_id_offset=0, capacitance_model=None,
                 validate=False, env_chunk=0, reset_kalman_on_reset=False, noise=None,
                 vary_peak_width=False, peak_width_alpha=0.01, voltage_capacitance_model=None, pixel_search=False,
                 num_charge_states=None, gs_gershgorin_zero=False):
        """pixel_search: a9 by the per-pixel search only (A/B switch; the default runs one search per 8x8 tile).
        gs_gershgorin_zero: the ground-state stage prunes hop components against the bound 0 alone (A/B switch,
        QD_FLAG_GS_GERSHGORIN_ZERO; the default prunes against the pixel's lowest pair bound: fewer tasks, same results).
        seed: base seed of the per-env device streams (PCG64(seed + global env id)) and the Philox key of
        the stochastic stages; None draws fresh OS entropy, as the reference's unseeded generators do
        (qarray_base_class.py:773-774, env.py:161).
        vary_peak_width / peak_width_alpha: QarrayBaseClass ctor arguments (qarray_base_class.py:42-43).
        voltage_capacitance_model: overrides `simulator.voltage_capacitance_model.type` of the qarray
        config (None keeps the file's value; "linear" or "none").
        num_charge_states: overrides `simulator.latched_model.num_charge_states` of the qarray config (None keeps the
        file's value): K, the charge states kept per pixel (1..32; the K x K Hamiltonian is solved exactly), or "all":
        every charge state with 0..max_charge_carriers carriers per dot (the YAML's explicit `num_charge_states: null`,
        the reference model's default).  One mode per handle; `self.num_charge_states` is K, or None for the full space,
        whose carrier cap is `self.max_charge_carriers` (None otherwise)."""
        if seed is None:
            seed = int(np.random.SeedSequence().entropy) & 0x7FFFFFFFFFFF      # 47 bits: seed + env id stays exact
        self.seed = int(seed)
        self.env_id_offset = int(env_id_offset)
        self.config = load_yaml(config_path, "env_config.yaml")
        self.qconfig = load_yaml(qarray_config_path, "qarray_config.yaml")
        override_charge_states(self.qconfig, num_charge_states)
        if voltage_capacitance_model is not None:
            self.qconfig["simulator"]["voltage_capacitance_model"]["type"] = \
                None if voltage_capacitance_model in ("none", "null") else voltage_capacitance_model
        sim = self.config["simulator"]
        self.num_envs = int(num_envs)
        self.num_dots = int(num_dots if num_dots is not None else sim["num_dots"])
        self.num_charge_states = check_solver_options(self.qconfig, n_dot=self.num_dots)
        self.max_charge_carriers = max_charge_carriers(self.qconfig) if self.num_charge_states is None else None
        self.use_barriers = bool(sim["use_barriers"])
        if not self.use_barriers:
            raise NotImplementedError("env.py only supports barrier mode for now")      # env.py:61-62
        rew = self.config["reward"]
        if rew.get("gate_curve_type", "constant") not in _lib.QD_CURVES:
            raise ValueError(f"Unknown curve type: {rew.get('gate_curve_type')}")            # env.py:441
        self.resolution = int(resolution if resolution is not None else sim["resolution"])
        self.max_steps = int(sim["max_steps"])
        self.update_method = self.config["capacitance_model"]["update_method"]
        if self.update_method in ("bayesian", "kriging", "ema"):                             # env.py:766-771
            raise NotImplementedError(f"update_method={self.update_method!r} requires an updater module the "
                                      "reference removed; use 'kalman' or 'direct'")
        if self.update_method == "fake":
            # env.py:555-559 hands fake_capacitance_model the (N, N+1) dot-only matrix, and
            # qarray_base_class.py:917-923 then stacks rows of N+nb+2 and N+nb+1 columns: the reference's own
            # barrier-mode path raises there, so there is no behaviour to reproduce.
            raise ValueError("update_method 'fake' fails in the reference's barrier mode (shape mismatch in "
                             "QarrayBaseClass._update_virtual_gate_matrix); not built")
        if self.update_method not in (None, "kalman", "direct", "perfect"):
            raise ValueError(f"Unknown update method: {self.update_method}")                 # env.py:788
        self.nearest_neighbour = bool(self.config["capacitance_model"].get("nearest_neighbour"))
        self.cnn_outputs = 2 if self.nearest_neighbour else 3
        if self.update_method in (None, "perfect"):
            capacitance_model = None                           # env.py:683-689: no CNN, no Kalman
        self.capacitance_model = capacitance_model
        if self.update_method in ("kalman", "direct") and capacitance_model is None:
            # same exception type as env.py:801-802
            raise RuntimeError("Error initialising capacitance model: update_method 'kalman' needs a "
                               "capacitance_model callable (images -> values, log_vars)")
        if not torch.cuda.is_available():
            raise RuntimeError("VecQuantumDeviceEnv needs a ROCm GPU (no CPU fallback)")
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.index is None:                                  # "cuda" means the CURRENT device
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.reset_kalman_on_reset = bool(reset_kalman_on_reset)
        N = self.num_dots; R = self.resolution; B = self.num_envs
        self.N, self.R, self.B, self.C = N, R, B, N - 1
        self.L = layout(N)
        self.sampler = DeviceSampler(N, self.qconfig, self.config, vary_peak_width=vary_peak_width,
                                     peak_width_alpha=peak_width_alpha,
                                     perfect_vgm=self.update_method == "perfect")
        self._rngs = [np.random.Generator(np.random.PCG64(self.seed + self.env_id_offset + e)) for e in range(B)]
        # ---- library handle ---------------------------------------------------
        self._lib = _lib.lib()
        self.noise_flags = self._noise_flags(noise)   # the stages this env's steps run (probe(noise=True) runs the same)
        self._probe_serials = 0                       # noisy probes so far: the default serial of the next one
        cfg = make_qd_config(self.config, self.qconfig, N, R, B, env_chunk=env_chunk,
                             flags=(_lib.QD_FLAG_VALIDATE if validate else 0) | (_lib.QD_FLAG_PIXEL_SEARCH if pixel_search else 0)
                             | (_lib.QD_FLAG_GS_GERSHGORIN_ZERO if gs_gershgorin_zero else 0),
                             noise_flags=self.noise_flags, seed=self.seed, env_id_offset=self.env_id_offset)
        self._h = ctypes.c_void_p()
        rc = self._lib.qd_create(ctypes.byref(cfg), self.device.index, ctypes.byref(self._h))
        if rc != 0:                          # a partially built handle carries the error text and must be released
            msg = self._lib.qd_last_error(self._h).decode() if self._h else "no handle"
            if self._h:
                self._lib.qd_destroy(self._h)
                self._h = None
            raise _lib.QdError(f"qd_create failed (code {rc}): {msg}")
        self.validate = bool(validate)
        # ---- caller-owned output tensors ---------------------------------------
        dev = self.device
        self.global_image = torch.zeros((B, R, R, self.C), dtype=torch.float32, device=dev)
        self.plunger_images = torch.zeros((B, N, R, R, 2), dtype=torch.float32, device=dev)
        self.barrier_images = torch.zeros((B, self.C, R, R, 1), dtype=torch.float32, device=dev)
        self.voltages = torch.zeros((B, 2 * N - 1), dtype=torch.float32, device=dev)
        self.rewards = torch.zeros((B, 2 * N - 1), dtype=torch.float64, device=dev)
        self.truncated = torch.zeros((B,), dtype=torch.uint8, device=dev)
        _lib.check(self._h, self._lib.qd_bind_outputs(self._h, self.global_image.data_ptr(),
                                                      self.plunger_images.data_ptr(),
                                                      self.barrier_images.data_ptr(),
                                                      self.voltages.data_ptr()), "qd_bind_outputs")
        self._params_host = np.zeros((B, self.L.size))
        self._T_host = np.full(B, np.nan)             # each device's sampled temperature (extras["T"]); NaN: loaded from raw blocks
        self._steps_host = np.zeros(B, np.int64)      # host mirror of the device step counters (truncation is
        self._needs_reset = True                      # deterministic, so auto-reset needs no device read-back)
        self.obs_count = 0
        self.final = None                             # step(keep_final=True): the truncating envs' last step (_snapshot)

    # ------------------------------------------------------------------ helpers
    def _noise_flags(self, noise):
        """noise=None/False: deterministic parity mode.  noise=True: what the configs enable
        (sensor white + telegraph noise always, radial noise if simulator.radial_noise.enabled).
        Or an iterable of {"sensor", "radial", "latch"}."""
        if not noise:
            return 0
        if noise is True:
            rn = self.config["simulator"].get("radial_noise") or {}
            lt = self.qconfig["simulator"]["model"].get("latching_model_parameters") or {}
            return (_lib.QD_NOISE_SENSOR | (_lib.QD_NOISE_RADIAL if rn.get("enabled") else 0)
                    | (_lib.QD_NOISE_LATCH if lt.get("Exists") else 0))
        f = 0
        for k in noise:
            f |= NOISE_STAGES[k]
        return f

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.qd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _obs(self):
        N = self.N
        return {"image": self.global_image, "obs_gate_voltages": self.voltages[:, :N],
                "obs_barrier_voltages": self.voltages[:, N:], "plunger_images": self.plunger_images,
                "barrier_images": self.barrier_images}

    def _cnn(self, env_ids=None):
        """Run the capacitance model on the current images of `env_ids` (all if None);
        returns full-batch (B,C,3) tensors as qd_update_capacitance expects."""
        if self.capacitance_model is None:
            return None, None
        img = self.barrier_images if env_ids is None else self.barrier_images[env_ids]
        n = img.shape[0]
        batch = img.reshape(n * self.C, 1, self.R, self.R)          # (C,1,R,R) per env, env.py:568-574
        values, log_vars = self.capacitance_model(batch)
        K = self.cnn_outputs
        values = values.to(torch.float32).reshape(n, self.C, K)
        log_vars = log_vars.to(torch.float32).reshape(n, self.C, K)
        if env_ids is None:
            return values.contiguous(), log_vars.contiguous()
        fv = torch.zeros((self.B, self.C, K), dtype=torch.float32, device=self.device)
        fl = torch.zeros_like(fv)
        fv[env_ids] = values; fl[env_ids] = log_vars
        return fv, fl

    # ------------------------------------------------------------------ probe scans
    def _to_dev(self, x, dtype, shape):
        """numpy / torch / scalar -> contiguous device tensor of `dtype`, broadcast to `shape`; host data goes through
        pinned memory so that the upload does not wait for the stream."""
        if isinstance(x, torch.Tensor):
            t = x.to(device=self.device, dtype=dtype)
        else:
            a = np.ascontiguousarray(np.asarray(x), dtype={torch.float64: np.float64, torch.int32: np.int32}[dtype])
            t = torch.from_numpy(a.reshape(-1)).pin_memory().to(self.device, non_blocking=True).reshape(a.shape)
        return t.broadcast_to(shape).contiguous()

    def _query_inputs(self, env_ids, gate_voltages, barrier_voltages, sensor_voltage):
        """What probe() and scan2d() take per query, on the device: (nq, env ids, gate, barrier, sensor voltages or None)."""
        def arr(x, dtype):
            return x if isinstance(x, torch.Tensor) else np.asarray(x, dtype)
        N, C = self.N, self.C
        gv = arr(gate_voltages, np.float64).reshape(-1, N)
        nq = int(gv.shape[0])
        return (nq, self._to_dev(arr(env_ids, np.int32).reshape(-1), torch.int32, (nq,)), self._to_dev(gv, torch.float64, (nq, N)),
                self._to_dev(arr(barrier_voltages, np.float64).reshape(-1, C), torch.float64, (nq, C)),
                None if sensor_voltage is None else self._to_dev(sensor_voltage, torch.float64, (nq,)))

    def _query_outputs(self, nq, channels, normalised, occupations, shape=None):
        """The result tensors of nq queries of `channels` = (C,) or () channel images each; `shape`: what one image is, (R, R)
        unless given ((n,) for the lines of scan1d)."""
        f64 = {"dtype": torch.float64, "device": self.device}
        shape = (self.R, self.R) if shape is None else tuple(shape)
        out = {"raw": torch.empty((nq, *channels, *shape), **f64)}
        if normalised:
            out["image"] = torch.empty((nq, *shape, *channels), dtype=torch.float32, device=self.device)
            out["plohi"] = torch.empty((nq, 2), **f64)
        if occupations:
            out["occupations"] = torch.empty((nq, *channels, *shape, self.N), **f64)
        return out

    def _query_serial(self, serial, flags):
        """The serial word of a probe or scan: the caller's, or (1 << 63) | k, k counting this object's noisy queries."""
        if serial is None:
            serial = (1 << 63) | self._probe_serials
            if flags:
                self._probe_serials += 1
        return int(serial) & 0xFFFFFFFFFFFFFFFF

    def _scan_request(self, opts_type, flags, frame, vgm, gamma, serial, stream_base, nq, occupations):
        """The options of a scan of nq queries as the family's struct `opts_type` (QdScanOpts, QdScanAffineOpts, QdScan1dOpts,
        QdScanGridOpts: one layout), with vgm and gamma uploaded.  Returns (opts, keep): keep holds the tensors that opts points
        to and the caller has not, to be kept until the call has been queued."""
        vm = None if vgm is None else self._to_dev(vgm, torch.float64, (nq, self.N + 1, self.N + 1))
        gm = None if gamma is None else self._to_dev(gamma, torch.float64, (nq,))
        opts = _opts(opts_type, frame=_lib.QD_SCAN_PHYSICAL if frame == "physical" else _lib.QD_SCAN_VIRTUAL, noise_flags=int(flags),
                     reserved=0, serial=self._query_serial(serial, flags),
                     stream_base=int(self.env_id_offset if stream_base is None else stream_base),
                     vgm_dev=_addr(vm), gamma_dev=_addr(gm), occ_dst=_addr(occupations))
        return opts, (vm, gm)

    def probe(self, env_ids, gate_voltages, barrier_voltages, sensor_voltage=None, window=None, normalised=False,
              noise=None, serial=None, stream_base=None, occupations=False):
        """Stateless scans (qd_probe / qd_probe_ex): the reference's `array._get_obs(gate_voltages, barrier_voltages,
        sensor_voltage)` for nq queries in one call, each on the device of env `env_ids[q]` with that env's current
        virtual gate matrix.  Nothing of the episodes changes (state, step counters, Kalman filters, last observation,
        noise streams), nq may exceed the batch and one env may serve many queries.
          env_ids           (nq,) ints, or one id for all queries
          gate_voltages     (nq, N) virtual gate voltages; barrier_voltages (nq, N-1)
          sensor_voltage    None (0.0, as the reference's default), a scalar or (nq,)
          window            None (each env's own half-width), a scalar or (nq,) half-widths
          noise             None / False: a deterministic probe, no noise stage runs.  True: the stages this env was
                            created with (those of its steps).  Or an iterable of {"sensor", "radial", "latch"}, as the
                            constructor takes it, whatever the env was created with
          serial            the observation-number word of the noise streams; None: (1 << 63) | k, where k counts this
                            object's noisy probes, so every call draws fresh noise and none shares a stream with a step
          stream_base       query q draws from the streams of global env id stream_base + q; None: env_id_offset
          occupations       True adds the occupations the signal was formed from (after latching, if it ran)
        numpy or torch inputs.  Returns device tensors {"raw": (nq, C, R, R) float64 unnormalised}, plus, with
        normalised=True, {"image": (nq, R, R, C) float32 normalised per query, "plohi": (nq, 2) its percentiles}, plus,
        with occupations=True, {"occupations": (nq, C, R, R, N) float64; NaN in a channel the radial stage replaced by
        white noise}."""
        nq, ids, gv, bv, sv = self._query_inputs(env_ids, gate_voltages, barrier_voltages, sensor_voltage)
        wd = None if window is None else self._to_dev(window, torch.float64, (nq,))
        out = self._query_outputs(nq, (self.C,), normalised, occupations)
        if noise is None and serial is None and stream_base is None and not occupations:
            rc = self._lib.qd_probe(self._h, _ptr(ids), nq, _ptr(gv), _ptr(bv), _ptr(sv), _ptr(wd), _ptr(out["raw"]),
                                    _ptr(out.get("image")), _ptr(out.get("plohi")), self._stream())
            _lib.check(self._h, rc, "qd_probe")
            return out
        flags = self.noise_flags if noise is True else self._noise_flags(noise)
        opts = _opts(_lib.QdProbeOpts, noise_flags=int(flags), serial=self._query_serial(serial, flags),
                     stream_base=int(self.env_id_offset if stream_base is None else stream_base), occ_dst=_addr(out.get("occupations")))
        rc = self._lib.qd_probe_ex(self._h, _ptr(ids), nq, _ptr(gv), _ptr(bv), _ptr(sv), _ptr(wd), _ptr(out["raw"]),
                                   _ptr(out.get("image")), _ptr(out.get("plohi")), ctypes.byref(opts), self._stream())
        _lib.check(self._h, rc, "qd_probe_ex")
        return out

    def compose(self, raw, nx, ny, channel=0, mode="global"):
        """One channel of nx*ny probe signals `raw` (nx*ny, C, R, R; scan (i, j) at index i*ny + j) stitched into one
        (ny*R, nx*R) float32 device image (qd_probe_compose).  mode "global": one exact 0.5 / 99.5 percentile pair over
        the whole composite, scan (i, j) at row block j; "per_scan": every scan normalised by itself, row blocks flipped.
        Returns (composite, plohi): plohi (2,) or (nx*ny, 2) float64."""
        per = {"global": _lib.QD_MAP_GLOBAL, "per_scan": _lib.QD_MAP_PER_SCAN}[mode]
        nq, R = int(nx) * int(ny), self.R
        raw = raw.to(device=self.device, dtype=torch.float64).contiguous()
        if raw.numel() != nq * self.C * R * R:
            raise ValueError(f"raw holds {raw.numel()} values, {nx} x {ny} scans need {nq * self.C * R * R}")
        comp = torch.empty((int(ny) * R, int(nx) * R), dtype=torch.float32, device=self.device)
        plohi = torch.empty((nq, 2) if per else (2,), dtype=torch.float64, device=self.device)
        rc = self._lib.qd_probe_compose(self._h, raw.data_ptr(), int(nx), int(ny), int(channel), per, comp.data_ptr(),
                                        plohi.data_ptr(), self._stream())
        _lib.check(self._h, rc, "qd_probe_compose")
        return comp, plohi

    # ------------------------------------------------------------------ axis scans
    def scan2d(self, env_ids, x, y, x_range, y_range, gate_voltages, barrier_voltages, sensor_voltage=None,
               frame="virtual", vgm=None, gamma=None, normalised=False, occupations=False, noise=None, serial=None,
               stream_base=None):
        """Stateless 2-D scans over any two controls (qd_scan2d): the reference model layer's `do2d_open(x_gate, x_min,
        x_max, ..., y_gate, ...)` / `GateVoltageComposer.do2d(..., gate_voltages, add_full_crosstalk=True)` for nq queries in
        one call, each on the device of env `env_ids[q]`.  Nothing of the episodes changes.
          env_ids           (nq,) ints, or one id for all queries
          x, y              the swept controls, one for all queries or (nq,): indices in the order of the model's voltage
                            vector (0..N-1 plungers, N the sensor gate, N+1..2N-1 barriers) or names, 1-indexed as the
                            composer's: "vP1".."vPN" ("P1".."PN" in the physical frame), "S", "B1".."B{N-1}".  x runs along
                            columns, y along rows
          x_range, y_range  (lo, hi) for all queries or (nq, 2); lo > hi sweeps downwards, lo == hi repeats a 1-D sweep
          gate_voltages     (nq, N), barrier_voltages (nq, N-1), sensor_voltage None (0.0) / scalar / (nq,): the controls
                            that are not swept
          frame             "virtual": the gates go through the virtual gate matrix (the env's current one, or `vgm`
                            (nq, N+1, N+1)) and origin; "physical": voltages as the model takes them, as eval_points
          gamma             None, a scalar or (nq,) peak widths.  None: with two virtual plungers as axes the rule of a
                            step (vary_peak_width) on those plungers' base voltages, else the env's constant
          noise             None / False: deterministic.  True: the sensor and latching stages this env was created with.
                            Or an iterable of {"sensor", "latch"}; the radial stage is not defined for axis scans
          serial, stream_base   as in probe()
        Returns device tensors {"raw": (nq, R, R) float64}, plus, with normalised=True, {"image": (nq, R, R) float32
        normalised per query, "plohi": (nq, 2)}, plus, with occupations=True, {"occupations": (nq, R, R, N) float64}."""
        N = self.N
        check_scan_frame(frame, vgm)
        nq, ids, gv, bv, sv = self._query_inputs(env_ids, gate_voltages, barrier_voltages, sensor_voltage)
        axes = np.stack([scan_control_indices(x, N, frame, nq), scan_control_indices(y, N, frame, nq)], axis=1)
        if np.any(axes[:, 0] == axes[:, 1]):
            raise ValueError("x and y must be two different controls")
        rng = scan_ranges(x_range, y_range, nq)
        flags = scan_noise_flags(noise, self.noise_flags, "axis scans")
        ax = self._to_dev(axes.astype(np.int32), torch.int32, (nq, 2))
        rg = self._to_dev(rng, torch.float64, (nq, 4))
        out = self._query_outputs(nq, (), normalised, occupations)
        opts, _keep = self._scan_request(_lib.QdScanOpts, flags, frame, vgm, gamma, serial, stream_base, nq, out.get("occupations"))
        rc = self._lib.qd_scan2d(self._h, _ptr(ids), nq, _ptr(ax), _ptr(rg), _ptr(gv), _ptr(bv), _ptr(sv), _ptr(out["raw"]),
                                 _ptr(out.get("image")), _ptr(out.get("plohi")), ctypes.byref(opts), self._stream())
        _lib.check(self._h, rc, "qd_scan2d")
        return out

    def scan_affine(self, env_ids, x, y, x_range, y_range, gate_voltages, barrier_voltages, sensor_voltage=None,
                    frame="virtual", vgm=None, gamma=None, normalised=False, occupations=False, noise=None, serial=None,
                    stream_base=None):
        """Stateless 2-D scans along two direction vectors over the controls (qd_scan_affine): detuning against the on-site
        axis, a plunger with a compensating barrier, any mixed-control axis, for nq queries in one call, each on the device
        of env `env_ids[q]`.  With W0 = [gate_voltages, sensor_voltage, barrier_voltages] of the query, pixel (row r, column
        c) sits at W0 + linspace(*x_range, R)[c] * dx + linspace(*y_range, R)[r] * dy.  Nothing of the episodes changes.
          x, y              the two axes, one for all queries or one per query (scan_axis_vector, scan_axis_vectors): a control
                            index or name as scan2d takes them; "e{i}_{j}" (detuning: +1 on plunger i, -1 on plunger j) or
                            "U{i}_{j}" (on-site: 1/sqrt(2) on both), 1-indexed and unnormalised exactly as the reference's
                            GateVoltageComposer builds them, plungers virtual or physical by `frame`; a {control: coefficient}
                            dict; a (2N,) vector, or (nq, 2N) for one per query.  A zero vector repeats a 1-D sweep.
                            Coefficients are not checked for NaN or infinity
          x_range, y_range  (lo, hi) of the scalar that multiplies the axis, for all queries or (nq, 2)
          gate_voltages, barrier_voltages, sensor_voltage   the BASE POINT of the scan.  Unlike the composer's crosstalk-free
                            `do2d(x_gate, ..., y_gate, ...)`, which holds every control that is not swept at 0 and adds its
                            origin once per "vP" axis, sqrt(2) times per "U" axis and never per "e" axis, the controls that
                            are not swept keep these voltages (a swept one starts from its own) and the origin is added once
          frame, vgm, normalised, occupations, noise, serial, stream_base   as in scan2d
          gamma             None (each env's constant coulomb_peak_width), a scalar or (nq,) peak widths.  The vary_peak_width
                            rule of a step is a function of the swept plunger pair and is not applied: an axis has no pair
        With unit vectors for x and y and 0 at those two controls of the base point this is scan2d (bit for bit, given the
        same gamma).  Returns what scan2d returns."""
        N = self.N
        check_scan_frame(frame, vgm)
        nq, ids, gv, bv, sv = self._query_inputs(env_ids, gate_voltages, barrier_voltages, sensor_voltage)
        dirs = np.stack([scan_axis_vectors(x, N, frame, nq), scan_axis_vectors(y, N, frame, nq)], axis=1)
        rng = scan_ranges(x_range, y_range, nq)
        flags = scan_noise_flags(noise, self.noise_flags, "axis scans")
        dr = self._to_dev(dirs, torch.float64, (nq, 2, 2 * N))
        rg = self._to_dev(rng, torch.float64, (nq, 4))
        out = self._query_outputs(nq, (), normalised, occupations)
        opts, _keep = self._scan_request(_lib.QdScanAffineOpts, flags, frame, vgm, gamma, serial, stream_base, nq, out.get("occupations"))
        rc = self._lib.qd_scan_affine(self._h, _ptr(ids), nq, _ptr(dr), _ptr(rg), _ptr(gv), _ptr(bv), _ptr(sv), _ptr(out["raw"]),
                                      _ptr(out.get("image")), _ptr(out.get("plohi")), ctypes.byref(opts), self._stream())
        _lib.check(self._h, rc, "qd_scan_affine")
        return out

    def scan1d(self, env_ids, axis, s_range, n_points, gate_voltages, barrier_voltages, sensor_voltage=None, *,
               frame="virtual", vgm=None, gamma=None, noise=(), serial=None, stream_base=None, occupations=False):
        """Stateless dense 1-D sweeps along one control or direction vector (qd_scan1d): the reference model layer's
        `do1d_open(gate, min, max, points)` over `GateVoltageComposer.do1d`, for nq queries in one call, each on the device of
        env `env_ids[q]`.  With W0 = [gate_voltages, sensor_voltage, barrier_voltages] of the query, point t sits at
        W0 + linspace(*s_range, n_points)[t] * d.  A line runs in a slot of its own size (ceil(sqrt(n))^2 records), not in one
        of an image.  Nothing of the episodes changes.
          axis              the direction d, one for all queries or one per query (scan_axis_vector, scan_axis_vectors): a
                            control index or name, "e{i}_{j}", "U{i}_{j}", a {control: coefficient} dict, a (2N,) vector, or
                            (nq, 2N).  The zero vector repeats the base point.  Coefficients are not checked for NaN or infinity
          s_range           (lo, hi) of the scalar that multiplies d, for all queries or (nq, 2); lo > hi sweeps downwards,
                            lo == hi repeats a point
          n_points          points per line, 1 .. R*R of this env, the same for all queries of a call
          gate_voltages, barrier_voltages, sensor_voltage   the BASE POINT, as in scan_affine
          frame, vgm, serial, stream_base   as in scan2d
          gamma             None (each env's constant coulomb_peak_width), a scalar or (nq,) peak widths
          noise             () / None / False: deterministic.  True: the sensor and latching stages this env was created with.
                            Or an iterable of {"sensor", "latch"}.  Latching walks the line as ONE row: the held state starts
                            at point 0 and is never reset; the telegraph chain starts at point 0
          occupations       True adds the occupations the signal was formed from (after latching, if it ran)
        Returns device tensors {"raw": (nq, n) float64, "image": (nq, n) float32 normalised per line with its own 0.5 / 99.5
        percentiles, "plohi": (nq, 2)}, plus, with occupations=True, {"occupations": (nq, n, N) float64}."""
        N = self.N
        check_scan_frame(frame, vgm)
        n = int(n_points)
        if not 1 <= n <= self.R * self.R:
            raise ValueError(f"n_points must be in 1..{self.R * self.R} (R*R of this env), got {n_points}")
        nq, ids, gv, bv, sv = self._query_inputs(env_ids, gate_voltages, barrier_voltages, sensor_voltage)
        dirs = scan_axis_vectors(axis, N, frame, nq)
        rng = np.array(np.broadcast_to(np.asarray(s_range, np.float64), (nq, 2)))
        flags = scan_noise_flags(noise, self.noise_flags, "lines")
        dr = self._to_dev(dirs, torch.float64, (nq, 2 * N))
        rg = self._to_dev(rng, torch.float64, (nq, 2))
        out = self._query_outputs(nq, (), True, occupations, shape=(n,))
        opts, _keep = self._scan_request(_lib.QdScan1dOpts, flags, frame, vgm, gamma, serial, stream_base, nq, out.get("occupations"))
        rc = self._lib.qd_scan1d(self._h, _ptr(ids), nq, n, _ptr(dr), _ptr(rg), _ptr(gv), _ptr(bv), _ptr(sv), _ptr(out["raw"]),
                                 _ptr(out["image"]), _ptr(out["plohi"]), ctypes.byref(opts), self._stream())
        _lib.check(self._h, rc, "qd_scan1d")
        return out

    def scan_grid(self, env_ids, x, y, x_range, y_range, nx, ny, gate_voltages, barrier_voltages, sensor_voltage=None, *,
                  frame="virtual", vgm=None, gamma=None, noise=(), serial=None, stream_base=None, occupations=False):
        """Stateless 2-D scans on any nx x ny grid of points along two direction vectors over the controls (qd_scan_grid): the
        reference model layer's `do2d_open(x_gate, x_min, x_max, x_points, y_gate, y_min, y_max, y_points)` over
        `GateVoltageComposer.do2d`, for nq queries in one call, each on the device of env `env_ids[q]`.  With W0 =
        [gate_voltages, sensor_voltage, barrier_voltages] of the query, point (row r, column c) sits at
        W0 + linspace(*x_range, nx)[c] * dx + linspace(*y_range, ny)[r] * dy.  A grid runs in a slot of its own size
        (ceil(sqrt(nx*ny))^2 records), not in one of an image, and costs what its point count costs.  Nothing of the episodes
        changes.
          x, y              the two axes, resolved as scan_affine resolves them (scan_axis_vectors)
          x_range, y_range  (lo, hi) of the scalar that multiplies the axis, for all queries or (nq, 2); lo > hi sweeps
                            downwards, lo == hi repeats a point
          nx, ny            columns and rows, both >= 1 with nx*ny <= R*R of this env, the same for all queries of a call
          gate_voltages, barrier_voltages, sensor_voltage   the BASE POINT, as in scan_affine
          frame, vgm, serial, stream_base   as in scan2d
          gamma             None (each env's constant coulomb_peak_width), a scalar or (nq,) peak widths
          noise             () / None / False: deterministic.  True: the sensor and latching stages this env was created with.
                            Or an iterable of {"sensor", "latch"}.  Latching walks every row of nx points by itself: the held
                            state is reset at every row start; the telegraph chain starts at point 0 and runs row after row
          occupations       True adds the occupations the signal was formed from (after latching, if it ran)
        With nx = ny = R this is scan_affine on a pixel_search env, with ny = 1 and a zero y it is scan1d (both bit for bit,
        noise included).  Returns device tensors {"raw": (nq, ny, nx) float64, "image": (nq, ny, nx) float32 normalised per
        grid with its own 0.5 / 99.5 percentiles, "plohi": (nq, 2)}, plus, with occupations=True, {"occupations":
        (nq, ny, nx, N) float64}.  scan_grid_closed is the same grid at a fixed total charge, scan_grid_thermal the same grid
        at a temperature, scan_grid_levels the same grid with the energy levels of every point."""
        return self._scan_grid(env_ids, x, y, x_range, y_range, nx, ny, gate_voltages, barrier_voltages, sensor_voltage, frame, vgm,
                               gamma, noise, serial, stream_base, occupations, None)

    def scan_grid_closed(self, env_ids, x, y, x_range, y_range, nx, ny, gate_voltages, barrier_voltages, n_charge,
                         sensor_voltage=None, *, frame="virtual", vgm=None, gamma=None, occupations=False):
        """scan_grid in the CLOSED regime (qd_scan_grid_closed; the reference's `do2d_closed`, and `do1d_closed` as a one-row
        grid): the array is isolated from its reservoirs and holds exactly `n_charge` carriers -- a scalar or (nq,) integers in
        0..32767 -- so the occupations of every point sum to n_charge.  Arguments, frames and results are scan_grid's; there
        are no noise stages.  In the physical frame the results equal eval_points(..., n_charge=) at the grid's voltages bit for
        bit."""
        if n_charge is None:
            raise ValueError("scan_grid_closed needs n_charge; scan_grid is the open regime")
        return self._scan_grid(env_ids, x, y, x_range, y_range, nx, ny, gate_voltages, barrier_voltages, sensor_voltage, frame, vgm,
                               gamma, (), None, None, occupations, n_charge)

    def scan_grid_thermal(self, env_ids, x, y, x_range, y_range, nx, ny, gate_voltages, barrier_voltages, kT, sensor_voltage=None, *,
                          n_charge=None, frame="virtual", vgm=None, gamma=None, noise=(), serial=None, stream_base=None,
                          occupations=False, variance=False, ztail=False):
        """scan_grid (n_charge None) or scan_grid_closed at a TEMPERATURE (qd_scan_grid_thermal): every point of the grid is in the
        thermal state rho = exp(-H / kT) / Z of eval_points(kT=), and "raw", "image", "plohi" and "occupations" are those of that
        state -- the thermally broadened charge-stability diagram.  scan_grid and scan_grid_closed themselves are the T = 0 calls
        they were, with the signatures they had.  Arguments, frames and results are scan_grid's, and
          kT                a scalar or (nq,) values, finite and > 0, one per query, in the energy units of `levels` of eval_points
          n_charge          None: the open regime.  A scalar or (nq,) integers in 0..32767: the closed regime of scan_grid_closed
          noise             "sensor" is allowed in the open regime (the sensor stage reads the thermal sensor constant alone);
                            "latch" raises ValueError (the latching model holds an integer configuration, a thermal mean has
                            none), also when noise=True would bring it along; no noise stage with n_charge
          variance, ztail   True adds "variance" (nq, ny, nx, N), sum_m P_m (s_m[d] - <n_d>)^2, and "ztail" (nq, ny, nx), the
                            normalised Boltzmann weight of the highest kept level (the check on the truncation to K states at
                            this kT)
        In the open regime the kernel solves each hop component of a point by itself; it agrees with eval_points(kT=) at the same
        voltages within the sum of both tolerances, not bit for bit.  A closed list is one hop component, so the whole-block
        solver of eval_points(kT=) runs, and in the physical frame the results equal eval_points(..., n_charge=, kT=) at the
        grid's voltages bit for bit."""
        if kT is None:
            raise ValueError("scan_grid_thermal needs kT; scan_grid and scan_grid_closed are the T = 0 calls")
        return self._scan_grid(env_ids, x, y, x_range, y_range, nx, ny, gate_voltages, barrier_voltages, sensor_voltage, frame, vgm,
                               gamma, noise, serial, stream_base, occupations, n_charge, kT, variance, ztail)

    RESPONSE_OUTPUTS = ("chi", "jacobian", "dsignal", "docc_axes", "dsignal_axes")

    def scan_grid_response(self, env_ids, x, y, x_range, y_range, nx, ny, gate_voltages, barrier_voltages, kT, sensor_voltage=None, *,
                           n_charge=None, frame="virtual", vgm=None, gamma=None, noise=(), serial=None, stream_base=None,
                           occupations=False, variance=False, ztail=False, response=("dsignal_axes", "docc_axes")):
        """scan_grid_thermal plus the CHARGE RESPONSE of the thermal state at every point of the grid (qd_scan_grid_response): the
        derivatives of eval_points(kT=, response=True), and the two a grid is plotted with -- the lock-in charge-stability diagram
        dS/dV along a sweep axis, and the slopes of the occupations along a transition line.  Arguments, frames and results are
        scan_grid_thermal's, and
          response   any non-empty subset of
                       "chi"           (nq, ny, nx, N, 2N-1)  d<n_i>/d(eps_k) and d<n_i>/d(ln tc_d), as eval_points defines them
                       "jacobian"      (nq, ny, nx, N, 2N)    d<n_i>/dv_j over the PHYSICAL voltages v = (vg, vb), in either frame
                       "dsignal"       (nq, ny, nx, 2N)       dS/dv_j, the slope of the sensor expression at the thermal c0
                       "docc_axes"     (nq, ny, nx, N, 2)     d<n_i>/d(sx), d<n_i>/d(sy) = jacobian . (u_x, u_y)
                       "dsignal_axes"  (nq, ny, nx, 2)        dS/d(sx), dS/d(sy) = dsignal . (u_x, u_y)
                     per unit of the axis scalars (the units of x_range / y_range), not per pixel.  u = dv/ds is the physical
                     direction of one step of the scalar: the axis vector itself in the physical frame; in the virtual frame
                     u[:N+1] = vgm @ axis[:N+1] with the query's `vgm` if given, else the env's matrix, and the barriers pass
                     through
        The kept list is held FIXED, Ns = rint(v''_s) is not differentiated and gamma is taken as constant, as in eval_points.
        "raw", "image", "plohi", "occupations", "variance" and "ztail" equal scan_grid_thermal bit for bit under the same
        arguments; the response is that of the noiseless sensor expression and does not depend on `noise`.  Open regime: the
        epilogue runs inside the hop components of a point and agrees with eval_points(kT=, response=True) at the same voltages
        within the sum of both tolerances.  With n_charge (closed): in the physical frame "chi", "jacobian" and "dsignal" equal
        that call bit for bit.  Envs with the voltage-dependent capacitance model are refused."""
        if kT is None:
            raise ValueError("scan_grid_response needs kT: the response is that of the thermal state")
        names = (response,) if isinstance(response, str) else tuple(response)
        if not names or any(r not in self.RESPONSE_OUTPUTS for r in names):
            raise ValueError(f"response must name a non-empty subset of {self.RESPONSE_OUTPUTS}, got {response!r}")
        return self._scan_grid(env_ids, x, y, x_range, y_range, nx, ny, gate_voltages, barrier_voltages, sensor_voltage, frame, vgm,
                               gamma, noise, serial, stream_base, occupations, n_charge, kT, variance, ztail, response=names)

    def scan_grid_levels(self, env_ids, x, y, x_range, y_range, nx, ny, gate_voltages, barrier_voltages, sensor_voltage=None, *,
                         levels=2, n_charge=None, frame="virtual", vgm=None, gamma=None, noise=(), serial=None, stream_base=None,
                         occupations=False):
        """scan_grid (n_charge None) or scan_grid_closed that also hands out the ENERGY LEVELS of every point
        (qd_scan_grid_levels): the `levels` lowest eigenvalues and ||H||_inf of the point's truncated Hamiltonian, as
        eval_points(levels=) defines them -- the gap map levels[1] - levels[0] over, say, detuning x barrier, from which a tunnel
        coupling is read off the anticrossing sqrt(eps^2 + 4 t^2), and rel_gap, the validity mask of the T = 0 diagram (below
        about 1e-9 float64 does not resolve the ground vector, and the point's occupations are round-off).  Arguments, frames
        and results are scan_grid's, and
          levels            1..8, the number of levels per point
          n_charge          None: the open regime.  A scalar or (nq,) integers in 0..32767: the closed regime of scan_grid_closed
          noise             as in scan_grid, open regime only; the levels do not depend on it
        Returns scan_grid's dict -- "raw", "image", "plohi" and "occupations" equal scan_grid / scan_grid_closed bit for bit under
        the same arguments -- plus {"levels": (nq, ny, nx, levels) float64, +inf from the point's number of valid kept states
        on, "hnorm": (nq, ny, nx)} and, for levels >= 2, {"gap": levels[..., 1] - levels[..., 0] (+inf where levels[..., 1]
        is), "rel_gap": gap / hnorm}.
        In the open regime the kernel tridiagonalises each hop component of a point by itself; it agrees with
        eval_points(levels=) at the same voltages within 2e-12 hnorm, not bit for bit.  A closed list is one hop component, so
        the whole-block solver of eval_points runs, and in the physical frame the levels equal
        eval_points(..., n_charge=, levels=) at the grid's voltages bit for bit."""
        L = int(levels)
        if L != levels or L < 1 or L > _lib.QD_LEVELS_MAX:
            raise ValueError(f"levels must be an integer in 1..{_lib.QD_LEVELS_MAX}, got {levels!r}")
        return self._scan_grid(env_ids, x, y, x_range, y_range, nx, ny, gate_voltages, barrier_voltages, sensor_voltage, frame, vgm,
                               gamma, noise, serial, stream_base, occupations, n_charge, levels=L)

    def _scan_grid(self, env_ids, x, y, x_range, y_range, nx, ny, gate_voltages, barrier_voltages, sensor_voltage, frame, vgm, gamma,
                   noise, serial, stream_base, occupations, n_charge, kT=None, variance=False, ztail=False, levels=0, response=()):
        """scan_grid (n_charge None) and scan_grid_closed; with kT, scan_grid_thermal in either regime, and with `response`
        scan_grid_response; with levels, scan_grid_levels in either regime"""
        N = self.N
        check_scan_frame(frame, vgm)
        cx, cy = int(nx), int(ny)
        if cx < 1 or cy < 1 or cx * cy > self.R * self.R:
            raise ValueError(f"nx and ny must be >= 1 with nx*ny <= {self.R * self.R} (R*R of this env), got {nx} x {ny}")
        nq, ids, gv, bv, sv = self._query_inputs(env_ids, gate_voltages, barrier_voltages, sensor_voltage)
        dirs = np.stack([scan_axis_vectors(x, N, frame, nq), scan_axis_vectors(y, N, frame, nq)], axis=1)
        rng = scan_ranges(x_range, y_range, nq)
        flags = scan_noise_flags(noise, self.noise_flags, "grids")
        kth = None
        if kT is not None:
            if flags & _lib.QD_NOISE_LATCH:
                raise ValueError("latching has no thermal form (the latching model holds an integer configuration, a thermal "
                                 "mean has none): a thermal grid's noise may name 'sensor' only")
            kth = host_kT(kT, nq)
        qd = None
        if n_charge is not None:
            if flags:
                raise ValueError("the closed regime has no noise stages: noise must be empty with n_charge")
            qd = self._to_dev(closed_charges(n_charge, nq, "query"), torch.int32, (nq,))
        dr = self._to_dev(dirs, torch.float64, (nq, 2, 2 * N))
        rg = self._to_dev(rng, torch.float64, (nq, 4))
        out = self._query_outputs(nq, (), True, occupations, shape=(cy, cx))
        opts, _keep = self._scan_request(_lib.QdScanGridOpts, flags, frame, vgm, gamma, serial, stream_base, nq, out.get("occupations"))
        # every entry point takes `lead`, then its own inputs, `dst`, its own options and the stream
        lead = (self._h, _ptr(ids), nq, cx, cy, _ptr(dr), _ptr(rg), _ptr(gv), _ptr(bv), _ptr(sv))
        dst = (_ptr(out["raw"]), _ptr(out["image"]), _ptr(out["plohi"]), ctypes.byref(opts))
        f64 = {"dtype": torch.float64, "device": self.device}
        if kth is not None:
            kd = self._to_dev(kth, torch.float64, (nq,))
            if variance:
                out["variance"] = torch.zeros((nq, cy, cx, N), **f64)
            if ztail:
                out["ztail"] = torch.zeros((nq, cy, cx), **f64)
            shapes = {"chi": (N, 2 * N - 1), "jacobian": (N, 2 * N), "dsignal": (2 * N,), "docc_axes": (N, 2), "dsignal_axes": (2,)}
            for r in response:
                out[r] = torch.zeros((nq, cy, cx) + shapes[r], **f64)
            thermal = dict(reserved=0, n_charge_dev=_addr(qd), var_dst=_addr(out.get("variance")), ztail_dst=_addr(out.get("ztail")))
            if response:
                name, own = "qd_scan_grid_response", _opts(
                    _lib.QdGridResponseOpts, **thermal, chi_dst=_addr(out.get("chi")), jac_dst=_addr(out.get("jacobian")),
                    dsignal_dst=_addr(out.get("dsignal")), docc_axes_dst=_addr(out.get("docc_axes")),
                    dsignal_axes_dst=_addr(out.get("dsignal_axes")))
            else:
                name, own = "qd_scan_grid_thermal", _opts(_lib.QdGridThermalOpts, **thermal)
            args = (*lead, _ptr(kd), *dst, ctypes.byref(own))
        elif levels:
            out["levels"] = torch.zeros((nq, cy, cx, levels), **f64)
            out["hnorm"] = torch.zeros((nq, cy, cx), **f64)
            own = _opts(_lib.QdGridLevelsOpts, n_levels=int(levels), n_charge_dev=_addr(qd), levels_dst=_addr(out["levels"]),
                        hnorm_dst=_addr(out["hnorm"]))
            name, args = "qd_scan_grid_levels", (*lead, *dst, ctypes.byref(own))
        elif qd is not None:
            name, args = "qd_scan_grid_closed", (*lead, _ptr(qd), *dst)
        else:
            name, args = "qd_scan_grid", (*lead, *dst)
        _lib.check(self._h, getattr(self._lib, name)(*args, self._stream()), name)
        if levels >= 2:
            # (+inf wherever the second level is: a point with one valid state, and one with none, where inf - inf would be nan
            # and hnorm is 0)
            l0, l1 = out["levels"][..., 0], out["levels"][..., 1]
            out["gap"] = torch.where(torch.isinf(l1), l1, l1 - l0)
            out["rel_gap"] = out["gap"] / out["hnorm"]
        return out

    # ------------------------------------------------------------------ point evaluation
    def eval_points(self, env_ids, vg, vb, gamma=None, outputs=("signal", "occupations"), n_charge=None, states=False, *, kT=None,
                    response=False, levels=0):
        """The reference model's point function (qd_eval_points): `charge_sensor_open(vg, vb)` and `ground_state_open(vg, vb)`
        (TunnelCoupledChargeSensed.py:312-380) at arbitrary PHYSICAL voltages, on the devices of the listed envs.  Nothing of
        the episodes changes and no noise stage runs; an env may be named many times.
          env_ids   (n,) ints
          vg        (n, m, N+1) physical gate voltages, sensor gate last (no virtual gate matrix is applied); vb (n, m, N-1);
                    numpy or device tensors -- or lists of n arrays (m_i, N+1) / (m_i, N-1) of different lengths
          gamma     None (each env's own coulomb_peak_width), a scalar or (n,) peak widths
          outputs   which of "signal" and "occupations" to compute.  The signal is solved from the kept states in the order
                    qd_observe and qd_probe solve them (their bits), the occupations from the reference order a validate
                    handle keeps (the bits of `occupations()`); with num_charge_states 8, 16 or 32 those orders differ and
                    asking for both runs the ground-state stage twice
          n_charge  None: the open regime.  A scalar or (n,) integers in 0..32767, one per env id: the CLOSED regime
                    (qd_eval_points_closed; the reference's `charge_sensor_closed` / `ground_state_closed`), the array isolated
                    from its reservoirs with exactly that many carriers.  The kept states are the K lowest of that total-charge
                    sector around the constrained continuous minimiser, the occupations of a point sum to n_charge, and signal
                    and occupations come from one solve
          states    True (closed regime only) adds "states": the kept charge states in list order, int32, zeros behind the
                    candidates found
          levels    L in 1..8 adds "levels" and "hnorm" (qd_eval_points_ex, open or closed): per point the L lowest eigenvalues,
                    increasing and counted with multiplicity, of H = diag(E) + H_t over the nv valid kept states -- the
                    reference's truncated K-state Hamiltonian with the |0..0> padding copies left out, not the spectrum of
                    the infinite system; +inf from level nv on -- and hnorm = ||H||_inf.  rel_gap = (levels[..., 1] -
                    levels[..., 0]) / hnorm is the project's measure of whether float64 resolves the ground vector.  With
                    levels > 0, outputs may be empty: then no ground-state kernel runs
          kT        None: the T = 0 ground state, as above.  A scalar or (n,) values, finite and > 0, one per env id, in the energy
                    units of `levels` (qd_eval_points_thermal): "signal" and "occupations" are those of the THERMAL state
                    rho = exp(-H / kT) / Z of the same truncated Hamiltonian -- P_m = sum_k w_k V[m,k]^2 over the whole
                    eigendecomposition, <n_d> = sum_m P_m s_m[d], the sensor signal evaluated at <n>; both from one solve --
                    and outputs may also name "variance" (sum_m P_m (s_m[d] - <n_d>)^2) and "ztail", the normalised
                    Boltzmann weight of the HIGHEST kept level: where that is not negligible the K kept states are too few for
                    this kT.  Defined at exact degeneracies (the equal mixture): no point needs the rel_gap exemption.  With
                    n_charge: the closed list.  Not together with levels or states=True: ask for those in a second call.
                    (keyword only, as `levels` is from here on)
          response  True (with kT; qd_eval_points_response) adds the derivatives of that thermal state at the point:
                    "chi" (n, m, N, 2N-1): columns 0..N-1 d<n_i>/d(eps_k) for H + eps_k n_k (symmetric, negative
                    semidefinite, -cov / kT when every tc is zero), columns N..2N-2 d<n_i>/d(ln tc_d);  "jacobian"
                    (n, m, N, 2N): d<n_i>/dv_j over v = (vg, vb);  "dsignal" (n, m, 2N): dS/dv_j.  The kept list is held
                    FIXED: this is the derivative of the truncated K-state model at the point (see `levels`), exact on
                    the transition lines, where it is the finite peak a measurement shows.  Ns = rint(v''_s) is piecewise
                    constant and its jumps are not differentiated; gamma is taken as constant.  The other outputs keep
                    the bits of the call without it.  Envs with the voltage-dependent capacitance model are refused
        Returns device tensors {"signal": (n, m) float64, "occupations": (n, m, N) float64[, "states": (n, m, K, N) int32]
        [, "levels": (n, m, L) float64, "hnorm": (n, m) float64][, "variance": (n, m, N), "ztail": (n, m) float64]
        [, "chi", "jacobian", "dsignal"]}; for list input, lists of n tensors (m_i,), (m_i, N), (m_i, K, N), (m_i, L), (m_i,),
        (m_i, N), (m_i,), (m_i, N, 2N-1), (m_i, N, 2N) and (m_i, 2N)."""
        outputs = tuple(outputs)
        if response and kT is None:
            raise ValueError("response=True needs kT: the response is that of the thermal state (at T = 0 it is round-off on the "
                             "transition lines and zero elsewhere); pass the temperature the derivative is wanted at")
        levels = int(levels)
        if not 0 <= levels <= _lib.QD_LEVELS_MAX:
            raise ValueError(f"levels must be in 0..{_lib.QD_LEVELS_MAX}, got {levels}")
        if kT is not None:
            if levels or states:
                raise ValueError("kT together with levels or states=True: ask for those in a second call")
            if not outputs or any(o not in ("signal", "occupations", "variance", "ztail") for o in outputs):
                raise ValueError(f"outputs must name 'signal', 'occupations', 'variance' and / or 'ztail', got {outputs!r}")
        elif (not outputs and levels == 0) or any(o not in ("signal", "occupations") for o in outputs):
            raise ValueError(f"outputs must name 'signal' and / or 'occupations', got {outputs!r}")
        N, C = self.N, self.C
        ids = np.asarray(env_ids.detach().cpu().numpy() if isinstance(env_ids, torch.Tensor) else env_ids, np.int32).reshape(-1)
        n = int(ids.size)
        if states and n_charge is None:
            raise ValueError("states=True needs n_charge: the kept states are an output of the closed regime")
        qh = None if n_charge is None else closed_charges(n_charge, n, "env id")
        kth = None if kT is None else host_kT(kT, n)
        if states and self.num_charge_states is None:
            raise _lib.QdError(f"qd_eval_points_closed refused (code {_lib.QD_ERR_STATE}): the full charge-state space has no "
                               "kept list of K states")
        ragged = isinstance(vg, (list, tuple))
        if ragged != isinstance(vb, (list, tuple)):
            raise ValueError("vg and vb must both be arrays or both be lists of per-env arrays")

        def rows(x, width):
            if isinstance(x, torch.Tensor):
                return x.to(device=self.device, dtype=torch.float64).reshape(-1, width)
            a = np.asarray(x, np.float64).reshape(-1, width)
            return self._to_dev(a, torch.float64, a.shape)

        if ragged:
            if len(vg) != n or len(vb) != n:
                raise ValueError(f"{n} env ids, {len(vg)} vg arrays and {len(vb)} vb arrays")
            gs, bs = [rows(x, N + 1) for x in vg], [rows(x, C) for x in vb]
            counts = [int(g.shape[0]) for g in gs]
            if counts != [int(b.shape[0]) for b in bs]:
                raise ValueError("vg and vb hold different numbers of points")
            g_all = torch.cat(gs) if gs else torch.empty((0, N + 1), dtype=torch.float64, device=self.device)
            b_all = torch.cat(bs) if bs else torch.empty((0, C), dtype=torch.float64, device=self.device)
        else:
            lead = tuple(vg.shape[:-1])
            if len(lead) != 2 or lead[0] != n or vg.shape[-1] != N + 1 or tuple(vb.shape) != lead + (C,):
                raise ValueError(f"vg must be ({n}, m, {N + 1}) and vb ({n}, m, {C}); got {tuple(vg.shape)} and {tuple(vb.shape)}")
            counts = [int(lead[1])] * n
            g_all, b_all = rows(vg, N + 1), rows(vb, C)
        g_all, b_all = g_all.contiguous(), b_all.contiguous()
        start = np.zeros(n + 1, np.int64)
        start[1:] = np.cumsum(counts)
        total = int(start[-1])
        gam = None if gamma is None else host_vector(gamma, n)
        K = self.num_charge_states
        # every output: name, dtype, shape of one point, whether the call has it -- in the order of the returned dict
        f64 = torch.float64
        table = (("states", torch.int32, (K, N), states), ("signal", f64, (), "signal" in outputs),
                 ("occupations", f64, (N,), "occupations" in outputs), ("levels", f64, (levels,), levels), ("hnorm", f64, (), levels),
                 ("variance", f64, (N,), "variance" in outputs), ("ztail", f64, (), "ztail" in outputs),
                 ("chi", f64, (N, 2 * N - 1), response), ("jacobian", f64, (N, 2 * N), response), ("dsignal", f64, (2 * N,), response))
        t = {name: torch.empty((total, *shape), dtype=dtype, device=self.device) for name, dtype, shape, wanted in table if wanted}
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        gp, qp = None if gam is None else gam.ctypes.data_as(dp), None if qh is None else qh.ctypes.data_as(ip)

        def opts_of(cls, **own):
            """the option struct of a branch with the fields they share: peak widths and total charges, variance and tail rows"""
            thermal = {} if cls is _lib.QdPointsOpts else dict(var_dst=_addr(t.get("variance")), ztail_dst=_addr(t.get("ztail")))
            return _opts(cls, gamma_host=gp, n_charge_host=qp, **thermal, **own)

        # every entry point takes `head`, then its own inputs, `dst` and its own outputs or options, and the stream
        head = (self._h, ids.ctypes.data_as(ip), start.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n, _ptr(g_all), _ptr(b_all))
        dst = (_ptr(t.get("signal")), _ptr(t.get("occupations")))
        if kth is not None:
            if response:
                name, opts = "qd_eval_points_response", opts_of(_lib.QdResponseOpts, chi_dst=_addr(t["chi"]), jac_dst=_addr(t["jacobian"]),
                                                                dsignal_dst=_addr(t["dsignal"]))
            else:
                name, opts = "qd_eval_points_thermal", opts_of(_lib.QdThermalOpts)
            args = (*head, kth.ctypes.data_as(dp), *dst, ctypes.byref(opts))
        elif levels:
            opts = opts_of(_lib.QdPointsOpts, n_levels=levels, states_dst=_addr(t.get("states")), levels_dst=_addr(t["levels"]),
                           hnorm_dst=_addr(t["hnorm"]))
            name, args = "qd_eval_points_ex", (*head, *dst, ctypes.byref(opts))
        elif qh is not None:
            name, args = "qd_eval_points_closed", (*head, gp, qp, *dst, _ptr(t.get("states")))
        else:
            name, args = "qd_eval_points", (*head, gp, *dst)
        if total:                                                        # (an empty tensor has no address to hand over)
            _lib.check(self._h, getattr(self._lib, name)(*args, self._stream()), name)
        if ragged:
            return {k: [v[start[i]:start[i + 1]] for i in range(n)] for k, v in t.items()}
        m = counts[0] if n else 0
        return {k: v.reshape(n, m, *v.shape[1:]) for k, v in t.items()}

    # ------------------------------------------------------------------ reset
    def load_new_devices(self, env_ids=None, seed=None):
        """Sample new random devices for the listed envs and upload their parameter / initial
        state blocks (the device-construction half of reset(); no observation is rendered)."""
        ids = np.arange(self.B, dtype=np.int32) if env_ids is None else np.asarray(env_ids, dtype=np.int32).reshape(-1)
        if seed is not None:                 # keyed by GLOBAL env id, like the constructor's streams
            for e in ids:
                self._rngs[e] = np.random.Generator(np.random.PCG64(int(seed) + self.env_id_offset + int(e)))
        u = np.stack([self._rngs[e].random(self.sampler.n_draws) for e in ids])
        eb = self.sampler.build(u)
        self._params_host[ids] = eb.params
        self._T_host[ids] = eb.extras["T"]
        self.last_episode = eb
        ip = ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        rc = self._lib.qd_load_episodes(self._h, ip, int(ids.size), eb.params.ctypes.data, eb.state.ctypes.data,
                                        1 if self.reset_kalman_on_reset else 0, self._stream())
        _lib.check(self._h, rc, "qd_load_episodes")
        self._steps_host[ids] = 0
        self._needs_reset = False
        return eb

    def observe(self, env_ids_dev=None, n=0):
        """Render the observation of the current state (qd_observe) without stepping."""
        idp = None if env_ids_dev is None else ctypes.c_void_p(env_ids_dev.data_ptr())
        _lib.check(self._h, self._lib.qd_observe(self._h, idp, int(n), self._stream()), "qd_observe")
        return self._obs()

    def reset(self, env_ids=None, seed=None, options=None, cnn_outputs=None):
        """Reset the listed envs (all if None).  Returns the observation dict of
        the whole batch (device tensors, valid until the next call)."""
        ids = np.arange(self.B, dtype=np.int32) if env_ids is None else np.asarray(env_ids, dtype=np.int32).reshape(-1)
        if ids.size == 0:
            return self._obs()
        self.load_new_devices(ids, seed=seed)
        all_envs = ids.size == self.B and np.array_equal(ids, np.arange(self.B))
        # (pinned + non_blocking: a pageable upload would make the host wait for everything queued on the stream before it)
        ids_dev = None if all_envs else torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).pin_memory().to(self.device, non_blocking=True)
        idp = None if all_envs else ctypes.c_void_p(ids_dev.data_ptr())
        _lib.check(self._h, self._lib.qd_observe(self._h, idp, int(ids.size), self._stream()), "qd_observe")
        if cnn_outputs is not None:
            values, log_vars = cnn_outputs
        else:
            values, log_vars = self._cnn(None if all_envs else ids_dev.long())
        if values is not None:
            values = values.contiguous(); log_vars = log_vars.contiguous()
            rc = self._lib.qd_update_capacitance(self._h, idp, int(ids.size), values.data_ptr(), log_vars.data_ptr(),
                                                 0, self._stream())             # reset does not refresh the ground truth (env.py:233)
            _lib.check(self._h, rc, "qd_update_capacitance")
            self._keep = (values, log_vars, ids_dev)
        self._needs_reset = False
        return self._obs()

    # ------------------------------------------------------------------ step
    def step(self, actions, cnn_outputs=None, auto_reset=False, keep_final=False):
        """actions: (B, 2N-1) float32 tensor (gates then barriers) or the reference's
        dict {"action_gate_voltages": (B,N), "action_barrier_voltages": (B,N-1)}.
        Returns (obs, rewards (B,2N-1) float64, terminated (B) bool, truncated (B) bool).
        keep_final: the envs whose episode ends at this step are captured (qd_snapshot, one launch on the same stream)
        after their last step and before auto_reset replaces their devices; `self.final` then holds them (see
        _snapshot), else None.  Rewards and truncation flags are not touched by the reset and stay in the return value."""
        if self._needs_reset:
            raise RuntimeError("step() called before reset()")
        if isinstance(actions, dict):
            actions = torch.cat([torch.as_tensor(actions["action_gate_voltages"]),
                                 torch.as_tensor(actions["action_barrier_voltages"])], dim=-1)
        actions = torch.as_tensor(actions, dtype=torch.float32, device=self.device).reshape(self.B, 2 * self.N - 1).contiguous()
        st = self._stream()
        if cnn_outputs is not None:
            values, log_vars = (t.to(torch.float32).contiguous() for t in cnn_outputs)
            rc = self._lib.qd_step(self._h, actions.data_ptr(), values.data_ptr(), log_vars.data_ptr(),
                                   self.rewards.data_ptr(), self.truncated.data_ptr(), st)
            _lib.check(self._h, rc, "qd_step")
            self._keep = (actions, values, log_vars)
        else:
            _lib.check(self._h, self._lib.qd_apply_actions(self._h, actions.data_ptr(), self.rewards.data_ptr(),
                                                           self.truncated.data_ptr(), st), "qd_apply_actions")
            _lib.check(self._h, self._lib.qd_observe(self._h, None, 0, st), "qd_observe")
            values, log_vars = self._cnn(None)
            vp = values.data_ptr() if values is not None else None
            lp = log_vars.data_ptr() if log_vars is not None else None
            _lib.check(self._h, self._lib.qd_update_capacitance(self._h, None, 0, vp, lp, 1, st),
                       "qd_update_capacitance")
            self._keep = (actions, values, log_vars)
        self._steps_host += 1
        truncated = self.truncated.bool()
        terminated = torch.zeros_like(truncated)
        obs = self._obs()
        self.final = None
        if keep_final:
            done = np.nonzero(self._steps_host >= self.max_steps)[0]
            if done.size:
                self.final = self._snapshot(done.astype(np.int32))
        if auto_reset:
            # the step counter alone decides truncation (env.py:281-285), so the host knows which envs are
            # done without reading the device: sampling the new devices below overlaps the kernels launched above
            done = np.nonzero(self._steps_host >= self.max_steps)[0]
            if done.size:
                truncated = truncated.clone()             # self.truncated is rewritten by the next step only, but be explicit
                obs = self.reset(env_ids=done.astype(np.int32))
        return obs, self.rewards, terminated, truncated

    def _snapshot(self, ids):
        """qd_snapshot of the envs `ids` (host int32) into fresh compact device tensors, stream-ordered, no host wait:
        {"global_image" (n,R,R,C), "plunger_images" (n,N,R,R,2), "barrier_images" (n,C,R,R,1), "voltages" (n,2N-1)
        float32; "state" (n, L.s_size), "params" (n, L.size) float64; "steps" (n,) int32; "env_ids" (n,) host int64}.
        Slot i is env env_ids[i].  final_device_state() / cgd_full_of() read the state and parameter rows."""
        n, N, R, C, dev = int(ids.size), self.N, self.R, self.C, self.device
        ids_dev = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).pin_memory().to(dev, non_blocking=True)
        f = {"global_image": torch.empty((n, R, R, C), dtype=torch.float32, device=dev),
             "plunger_images": torch.empty((n, N, R, R, 2), dtype=torch.float32, device=dev),
             "barrier_images": torch.empty((n, C, R, R, 1), dtype=torch.float32, device=dev),
             "voltages": torch.empty((n, 2 * N - 1), dtype=torch.float32, device=dev),
             "state": torch.empty((n, self.L.s_size), dtype=torch.float64, device=dev),
             "params": torch.empty((n, self.L.size), dtype=torch.float64, device=dev),
             "steps": torch.empty((n,), dtype=torch.int32, device=dev)}
        ptr = [ctypes.c_void_p(f[k].data_ptr()) for k in ("global_image", "plunger_images", "barrier_images", "voltages",
                                                           "state", "params", "steps")]
        _lib.check(self._h, self._lib.qd_snapshot(self._h, ctypes.c_void_p(ids_dev.data_ptr()), n, *ptr, self._stream()),
                   "qd_snapshot")
        f["env_ids"] = ids.astype(np.int64)
        f["env_ids_dev"] = ids_dev
        return f

    def device_state_of(self, state, params, steps):
        """device_state()'s dict for host rows of state / parameter blocks and step counters (e.g. a snapshot's)."""
        return device_state_from_rows(self.L, state, params, steps)

    def cgd_full_of(self, params):
        return cgd_full_from_params(self.L, params)

    def final_device_state(self, final=None):
        """device_state() of the envs of a snapshot (default: self.final), slot by slot, as they were at their last
        step (blocking host copy)."""
        f = self.final if final is None else final
        return self.device_state_of(f["state"].cpu().numpy(), f["params"].cpu().numpy(), f["steps"].cpu().numpy())

    # ------------------------------------------------------------------ state access
    def get_state(self):
        """Host copy of the per-env state blocks and step counters (checkpointing,
        infos, validation)."""
        st = np.zeros((self.B, self.L.s_size)); steps = np.zeros(self.B, np.int32)
        _lib.check(self._h, self._lib.qd_get_state(self._h, st.ctypes.data, steps.ctypes.data), "qd_get_state")
        return st, steps

    def set_state(self, state, steps):
        state = np.ascontiguousarray(state, dtype=np.float64); steps = np.ascontiguousarray(steps, dtype=np.int32)
        _lib.check(self._h, self._lib.qd_set_state(self._h, state.ctypes.data, steps.ctypes.data), "qd_set_state")
        self._steps_host[:] = steps

    def stagger_episodes(self):
        """Spread the episode phases (env e is put at step e mod max_steps) so that a steady 1/max_steps of
        the batch truncates and resets at every step -- what a long-running sampler looks like."""
        st, _ = self.get_state()
        self.set_state(st, (np.arange(self.B) + self.env_id_offset) % self.max_steps)

    # ------------------------------------------------------------------ checkpoint
    def get_checkpoint(self):
        """Everything needed to continue bit-identically (SURVEY 5 "expose RNG seeds/counters"): device state and
        step counters, the current devices' parameter blocks and sampled temperatures ("T"; a checkpoint without it restores
        NaN), every env's host generator state, the Philox observation counter of the stochastic stages and the synthetic CNN's
        call counter if one is used."""
        st, steps = self.get_state()
        ser = ctypes.c_uint64(0)
        _lib.check(self._h, self._lib.qd_get_rng_state(self._h, ctypes.byref(ser)), "qd_get_rng_state")
        return {"state": st, "steps": steps, "params": self._params_host.copy(), "T": self._T_host.copy(),
                "rng": [g.bit_generator.state for g in self._rngs], "obs_serial": int(ser.value),
                "seed": self.seed, "env_id_offset": self.env_id_offset,
                "capacitance_model_calls": getattr(self.capacitance_model, "calls", None)}

    def set_checkpoint(self, ck):
        if ck["params"].shape != self._params_host.shape:
            raise ValueError("checkpoint belongs to an env of a different shape")
        if (ck["seed"], ck["env_id_offset"]) != (self.seed, self.env_id_offset):
            raise ValueError("checkpoint was taken with another seed / env_id_offset (the Philox key differs)")
        ids = np.arange(self.B, dtype=np.int32)
        params = np.ascontiguousarray(ck["params"], dtype=np.float64)
        state = np.ascontiguousarray(ck["state"], dtype=np.float64)
        rc = self._lib.qd_load_episodes(self._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), self.B,
                                        params.ctypes.data, state.ctypes.data, 0, self._stream())
        _lib.check(self._h, rc, "qd_load_episodes")
        self._params_host[:] = params
        self._T_host[:] = ck["T"] if "T" in ck else np.nan
        self.set_state(state, ck["steps"])
        for g, s_ in zip(self._rngs, ck["rng"]):
            g.bit_generator.state = s_
        _lib.check(self._h, self._lib.qd_set_rng_state(self._h, ctypes.c_uint64(ck["obs_serial"])), "qd_set_rng_state")
        if ck.get("capacitance_model_calls") is not None and hasattr(self.capacitance_model, "calls"):
            self.capacitance_model.calls = ck["capacitance_model_calls"]
        self._needs_reset = False

    def device_state(self):
        """The reference's info["current_device_state"] for every env (env.py:214-222)."""
        st, steps = self.get_state()
        return device_state_from_rows(self.L, st, self._params_host, steps)

    def raw(self):
        raw = np.zeros((self.B, self.C, self.R * self.R)); pl = np.zeros((self.B, 2))
        _lib.check(self._h, self._lib.qd_get_raw(self._h, raw.ctypes.data, pl.ctypes.data), "qd_get_raw")
        return raw, pl

    def occupations(self):
        occ = np.zeros((self.B, self.C, self.R * self.R, self.N))
        _lib.check(self._h, self._lib.qd_get_occupations(self._h, occ.ctypes.data), "qd_get_occupations")
        return occ

    def eigen(self):
        """(B,C,P,2): ground energy of each pixel's K-state Hamiltonian (K = num_charge_states; the whole M-state one in
        the full space) and the relative residual of the eigenpair the occupations came from (validate mode)."""
        eg = np.zeros((self.B, self.C, self.R * self.R, 2))
        _lib.check(self._h, self._lib.qd_get_eigen(self._h, eg.ctypes.data), "qd_get_eigen")
        return eg

    def search_stats(self):
        """Tile-search counters (validate mode): tiles, tiles redone whole, pixels redone, mean superset size."""
        out = (ctypes.c_uint64 * 16)()
        _lib.check(self._h, self._lib.qd_get_search_stats(self._h, out), "qd_get_search_stats")
        t = max(int(out[0]), 1)
        return {"tiles": int(out[0]), "tiles_redone": int(out[1]), "pixels_redone": int(out[2]),
                "pixels_redone_few_states": int(out[4]), "mean_superset": int(out[3]) / t,
                "tiles_redone_by_reason": {k: int(out[8 + i]) for i, k in
                                           enumerate(("", "ranges", "seeds", "frontier", "leaves", "superset")) if k}}

    def solver_stats(self):
        """Eigen-solver counters of the ground-state kernel (validate mode): tasks = hop components of >= 2 states
        solved, Laguerre iterations per task and per 64-task wave tile (a tile waits for its slowest lane), tasks by size
        (2 .. 8 states each; "9+": the classes of 9-10, 11-12 and 13-32 states together; the counters are per size class,
        out[4 + class]); wide_tasks: the blocks of 33..64 states (full space only), solved one per wavefront and in no tile."""
        out = (ctypes.c_uint64 * 16)()
        _lib.check(self._h, self._lib.qd_get_solver_stats(self._h, out), "qd_get_solver_stats")
        tasks, tiles = max(int(out[0]), 1), max(int(out[2]), 1)
        by_size = {str(k + 2): int(out[4 + k]) for k in range(7)}
        by_size["9+"] = int(out[11]) + int(out[12]) + int(out[13])
        return {"tasks": int(out[0]), "laguerre_per_task": int(out[1]) / tasks, "tiles": int(out[2]),
                "laguerre_per_tile_max": int(out[3]) / tiles, "lane_fill": (int(out[0]) - int(out[14])) / (64.0 * tiles),
                "tasks_by_size": by_size, "wide_tasks": int(out[14])}

    def candidates(self):
        """(B,C,P,32,N) int32 kept charge states (validate mode): slots 0..K-1 the K = num_charge_states states in the
        reference order (|0..0> padding included), slots K..31 are -1.  The full space keeps no such list: QdError."""
        st = np.zeros((self.B, self.C, self.R * self.R, 32, self.N), np.int32)
        _lib.check(self._h, self._lib.qd_get_candidates(self._h, st.ctypes.data), "qd_get_candidates")
        return st

    def time_ground_kernel(self, iters=3):
        ms = ctypes.c_float(0)
        _lib.check(self._h, self._lib.qd_time_ground_kernel(self._h, iters, ctypes.byref(ms), self._stream()),
                   "qd_time_ground_kernel")
        return float(ms.value)

    def time_candidates_kernel(self, iters=3):
        ms = ctypes.c_float(0)
        _lib.check(self._h, self._lib.qd_time_candidates_kernel(self._h, iters, ctypes.byref(ms), self._stream()),
                   "qd_time_candidates_kernel")
        return float(ms.value)

    def time_kernels(self, iters=3):
        """HIP-event duration (ms) of one launch over a launch chunk of each hot kernel: dict name -> ms, in pipeline order
        (qd_k_tile, qd_k_candidates = redo pass, qd_k_gs_structure, qd_k_gs_solve = all size classes, qd_k_gs_select)."""
        out = (ctypes.c_float * 5)()
        _lib.check(self._h, self._lib.qd_time_kernels(self._h, int(iters), out, self._stream()), "qd_time_kernels")
        return {self._lib.qd_timed_kernel_name(k).decode(): float(out[k]) for k in range(5)}

    def chunk_envs(self):
        """env-steps covered by one launch of the hot kernels."""
        return int(self._lib.qd_chunk_envs(self._h))
