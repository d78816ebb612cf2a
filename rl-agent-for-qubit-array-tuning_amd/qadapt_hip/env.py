"""
QuantumDeviceEnv -- single-environment, NumPy-in / NumPy-out mirror of the
reference class of the same name (src/qadapt/environment/env.py:29-896), backed
by the batched HIP library with a batch of one.  It has the constructor signature
the reference's MultiAgentEnvWrapper expects from `base_env_class`
(multi_agent_wrapper.py:93-106): (training, config_path,
capacitance_model_checkpoint), plus .reset / .step / .close,
.observation_space / .action_space, .num_dots, .use_barriers and
.array.model.cgd_full, so it can be dropped into the reference wrapper or into
qadapt_hip.multi_agent.MultiAgentEnvWrapper unchanged.
"""
from __future__ import annotations

import numpy as np

from . import spaces
from .device_model import load_yaml


class ModelFacade:
    """`env.array.model` of the reference (a TunnelCoupledChargeSensed) as far as it is built: `cgd_full`, the peak width
    `coulomb_peak_width` and the point functions `charge_sensor_open(vg, vb)` / `ground_state_open(vg, vb)`
    (TunnelCoupledChargeSensed.py:312-380), evaluated by the backend's `eval_points` on the env's current device without
    touching the episode and without noise.  `coulomb_peak_width` is the device's own at every reset and is read at call
    time, so it may be assigned as the reference's `_get_obs` does (qarray_base_class.py:192-196).
    The `_closed` siblings (TunnelCoupledChargeSensed.py:256-268, 291-309, 382-426) take the total charge `n_charge` of an
    array that is isolated from its reservoirs: the kept states are the lowest of that total-charge sector around the
    constrained continuous minimiser (DESIGN "closed regime"; the reference leaves its own ground-state half undefined), the
    occupations of every point sum to n_charge, and the sensor half is the open one fed those occupations.
    `thermal_state_open / thermal_state_closed` are the same point functions at the model's temperature `T`, which the
    reference samples and never uses: occupations, their variances and the signal of exp(-H / kT) / Z."""

    def __init__(self, backend, num_dots):
        self._b = backend
        self.n_dot = int(num_dots)
        self.cgd_full = None
        self.coulomb_peak_width = None

    def _points(self, vg, vb, outputs, n_charge=None):
        if vb is None:
            raise NotImplementedError(
                "charge_sensor_open / ground_state_open without barrier voltages: the reference's barrier-less branch uses a "
                "constant model.tc that the env never sets, and cgd_full has 2N columns (gates and barriers) in barrier "
                "mode, so it cannot run there either; pass vb")
        N = self.n_dot
        vg, vb = np.asarray(vg, np.float64), np.asarray(vb, np.float64)
        if vg.shape[-1:] != (N + 1,) or vb.shape[-1:] != (N - 1,) or vg.shape[:-1] != vb.shape[:-1]:
            raise ValueError(f"vg must be (..., {N + 1}) and vb (..., {N - 1}) with equal leading shapes; "
                             f"got {vg.shape} and {vb.shape}")
        lead = vg.shape[:-1]
        gamma = None if self.coulomb_peak_width is None else float(self.coulomb_peak_width)
        kw = {} if n_charge is None else {"n_charge": n_charge}
        out = self._b.eval_points([0], vg.reshape(1, -1, N + 1), vb.reshape(1, -1, N - 1), gamma=gamma, outputs=outputs, **kw)
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        signal = host(out["signal"]).astype(np.float64).reshape(lead + (1,)) if "signal" in outputs else None
        return signal, host(out["occupations"]).astype(np.float64).reshape(lead + (N,))

    def charge_sensor_open(self, vg, vb=None):
        """(signal (..., 1), n_open (..., N)) float64 at physical gate voltages vg (..., N+1) and barrier voltages vb (..., N-1)."""
        return self._points(vg, vb, ("signal", "occupations"))

    def ground_state_open(self, vg, vb=None):
        """n_open (..., N) float64."""
        return self._points(vg, vb, ("occupations",))[1]

    def charge_sensor_closed(self, vg, n_charge, vb=None):
        """(signal (..., 1), n_closed (..., N)) float64 with exactly `n_charge` carriers in the array; arguments in the
        reference's order."""
        return self._points(vg, vb, ("signal", "occupations"), n_charge=n_charge)

    def ground_state_closed(self, vg, n_charge, vb=None):
        """n_closed (..., N) float64; every row sums to n_charge."""
        return self._points(vg, vb, ("occupations",), n_charge=n_charge)[1]

    def _levels(self, vg, vb, n_levels, n_charge=None):
        if vb is None:
            raise NotImplementedError("energy levels without barrier voltages: as charge_sensor_open, pass vb")
        N = self.n_dot
        vg, vb = np.asarray(vg, np.float64), np.asarray(vb, np.float64)
        if vg.shape[-1:] != (N + 1,) or vb.shape[-1:] != (N - 1,) or vg.shape[:-1] != vb.shape[:-1]:
            raise ValueError(f"vg must be (..., {N + 1}) and vb (..., {N - 1}) with equal leading shapes; "
                             f"got {vg.shape} and {vb.shape}")
        lead = vg.shape[:-1]
        kw = {} if n_charge is None else {"n_charge": n_charge}
        out = self._b.eval_points([0], vg.reshape(1, -1, N + 1), vb.reshape(1, -1, N - 1), outputs=(), levels=int(n_levels), **kw)
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        return (host(out["levels"]).astype(np.float64).reshape(lead + (int(n_levels),)),
                host(out["hnorm"]).astype(np.float64).reshape(lead))

    def energy_levels_open(self, vg, vb=None, n_levels=2):
        """(levels (..., n_levels), hnorm (...)) float64: the n_levels (1..8) lowest eigenvalues, in increasing order and
        counted with multiplicity, of the point's Hamiltonian over its valid kept charge states -- the reference's truncated
        K-state matrix without the |0..0> padding copies, NOT the spectrum of the infinite system -- and its infinity norm.
        Levels beyond the number of valid states are +inf.  (levels[..., 1] - levels[..., 0]) / hnorm is the relative gap
        that says whether float64 resolves the point's ground vector (occupations and signal are round-off below ~1e-9)."""
        return self._levels(vg, vb, n_levels)

    def energy_levels_closed(self, vg, n_charge, n_levels=2, vb=None):
        """energy_levels_open on the closed list: the kept states of the total-charge sector `n_charge`."""
        return self._levels(vg, vb, n_levels, n_charge=n_charge)

    @property
    def T(self):
        """the device's sampled temperature (the model's `T` field), read from the backend at call time; NaN for a device
        loaded from raw parameter blocks, None on a backend that keeps none"""
        t = getattr(self._b, "_T_host", None)
        return None if t is None else float(t[0])

    def _thermal(self, vg, vb, T, n_charge=None):
        if vb is None:
            raise NotImplementedError("the thermal state without barrier voltages: as charge_sensor_open, pass vb")
        N = self.n_dot
        vg, vb = np.asarray(vg, np.float64), np.asarray(vb, np.float64)
        if vg.shape[-1:] != (N + 1,) or vb.shape[-1:] != (N - 1,) or vg.shape[:-1] != vb.shape[:-1]:
            raise ValueError(f"vg must be (..., {N + 1}) and vb (..., {N - 1}) with equal leading shapes; "
                             f"got {vg.shape} and {vb.shape}")
        if T is None:
            T = self.T
            if T is None or not np.isfinite(T):
                raise ValueError("T=None needs the device's own sampled temperature, and this device was loaded from raw "
                                 "parameter blocks, which carry none; pass T")
        kT = 8.617333262145e-5 * float(T)
        lead = vg.shape[:-1]
        gamma = None if self.coulomb_peak_width is None else float(self.coulomb_peak_width)
        kw = {} if n_charge is None else {"n_charge": n_charge}
        out = self._b.eval_points([0], vg.reshape(1, -1, N + 1), vb.reshape(1, -1, N - 1), gamma=gamma,
                                  outputs=("signal", "occupations", "variance"), kT=kT, **kw)
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        return (host(out["signal"]).astype(np.float64).reshape(lead + (1,)),
                host(out["occupations"]).astype(np.float64).reshape(lead + (N,)),
                host(out["variance"]).astype(np.float64).reshape(lead + (N,)))

    def thermal_state_open(self, vg, vb=None, T=None):
        """(signal (..., 1), n (..., N), var (..., N)) float64 of the thermal state rho = exp(-H / kT) / Z of the point's
        Hamiltonian over its valid kept charge states (the truncated K-state matrix of `energy_levels_open`): n the mean
        occupations, var their variances, the signal that of `charge_sensor_open` evaluated at n.  `T` is the model's
        temperature field and is converted by the reference's line as it is written (ground_state.py:48),
        kT = 8.617333262145e-5 * T, which the reference itself never uses; the unit-free way in is `kT` on the backend's
        `eval_points`, which also hands out "ztail", the check on the truncation.  T=None: the device's own sampled T
        (`self.T`, the qarray_config draw); a device loaded from raw parameter blocks has none and raises ValueError."""
        return self._thermal(vg, vb, T)

    def thermal_state_closed(self, vg, n_charge, T=None, vb=None):
        """thermal_state_open on the closed list: the kept states of the total-charge sector `n_charge`; every n sums to it."""
        return self._thermal(vg, vb, T, n_charge=n_charge)

    def _response(self, vg, vb, T, n_charge=None):
        if vb is None:
            raise NotImplementedError("the charge response without barrier voltages: as charge_sensor_open, pass vb")
        N = self.n_dot
        vg, vb = np.asarray(vg, np.float64), np.asarray(vb, np.float64)
        if vg.shape[-1:] != (N + 1,) or vb.shape[-1:] != (N - 1,) or vg.shape[:-1] != vb.shape[:-1]:
            raise ValueError(f"vg must be (..., {N + 1}) and vb (..., {N - 1}) with equal leading shapes; "
                             f"got {vg.shape} and {vb.shape}")
        if T is None:
            T = self.T
            if T is None or not np.isfinite(T):
                raise ValueError("T=None needs the device's own sampled temperature, and this device was loaded from raw "
                                 "parameter blocks, which carry none; pass T")
        kT = 8.617333262145e-5 * float(T)
        lead = vg.shape[:-1]
        gamma = None if self.coulomb_peak_width is None else float(self.coulomb_peak_width)
        kw = {} if n_charge is None else {"n_charge": n_charge}
        out = self._b.eval_points([0], vg.reshape(1, -1, N + 1), vb.reshape(1, -1, N - 1), gamma=gamma,
                                  outputs=("signal", "occupations"), kT=kT, response=True, **kw)
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        return (host(out["chi"]).astype(np.float64).reshape(lead + (N, 2 * N - 1)),
                host(out["jacobian"]).astype(np.float64).reshape(lead + (N, 2 * N)),
                host(out["dsignal"]).astype(np.float64).reshape(lead + (2 * N,)))

    def charge_response_open(self, vg, vb=None, T=None):
        """(chi (..., N, 2N-1), jacobian (..., N, 2N), dsignal (..., 2N)) float64 of the thermal state of `thermal_state_open`
        at the point: chi[..., i, k] = d<n_i>/d(eps_k) for H + eps_k n_k (k < N) and d<n_i>/d(ln tc_d) (k = N + d),
        jacobian[..., i, j] = d<n_i>/dv_j over v = (vg, vb) -- the local slopes the capacitance virtualisation estimates --
        and dsignal[..., j] = dS/dv_j, the lock-in transconductance.  The kept list is held fixed (the derivative of the
        truncated K-state model), the jumps of the sensor's rint are not differentiated and the peak width is a constant.
        `T` as in `thermal_state_open`."""
        return self._response(vg, vb, T)

    def charge_response_closed(self, vg, n_charge, T=None, vb=None):
        """charge_response_open on the closed list of the total-charge sector `n_charge`: every column of chi and of the
        jacobian sums to zero over the dots."""
        return self._response(vg, vb, T, n_charge=n_charge)

    def _gate_axis(self, gate):
        """(axis, frame) of one gate of the composer's grammar, as the backend's scans take them"""
        N = self.n_dot
        if isinstance(gate, (int, np.integer)) and not isinstance(gate, bool):
            g = int(gate)
            if not 1 <= g <= N + 1:
                raise ValueError(f"gate must be in the range 1 to {N + 1}")
            axis, frame = g - 1, "physical"
        elif isinstance(gate, str) and gate[:1] == "P" and gate[1:].isdigit():
            g = int(gate[1:])
            if not 1 <= g <= N + 1:
                raise ValueError(f"{gate!r}: P1..P{N + 1} exist for {N} dots (P{N + 1} is the sensor gate)")
            axis, frame = g - 1, "physical"
        elif isinstance(gate, str) and (gate[:2] == "vP" or gate[:1] in ("e", "U")):
            axis, frame = gate, "virtual"
        else:
            raise ValueError(f"Invalid gate {gate!r} must be in the form P[int], vP[int], e[int]_[int], U[int]_[int]")
        return axis, frame

    def do1d_open(self, gate, min, max, points):
        """The reference's `do1d_open(gate, min, max, points)` (TunnelCoupledChargeSensed.py:192-205 over
        GateVoltageComposer.do1d): a noise-free sweep of `points` points of one gate over [min, max] on the env's current
        device, every other gate, the sensor gate and the barriers at 0 -- the base point is zero, as the composer builds it.
        Returns (signal (points, 1), n_open (points, N)) float64, as charge_sensor_open does.  `gate` follows the composer's
        grammar: an int g or "P{g}" (1-indexed; g = N+1 is the sensor gate) sweeps that PHYSICAL gate; "vP{i}", "e{i}_{j}"
        (v_i - v_j) and "U{i}_{j}" ((v_i + v_j) / sqrt(2)) sweep in the VIRTUAL frame through the env's current virtual gate
        matrix.  The composer's grid carries the virtual gate origin once on a "vP" sweep, sqrt(2) times on a "U" sweep, and
        never on an "e" or a physical sweep (each _do1d_virtual term brings it along).  The facade renders through the
        backend's scan1d, whose virtual frame adds the origin exactly ONCE: "vP", "P" and int sweeps are the composer's grid,
        an "e" sweep sits one origin above it and a "U" sweep sqrt(2) - 1 origins below it; with a zero origin all agree."""
        N = self.n_dot
        axis, frame = self._gate_axis(gate)
        gamma = None if self.coulomb_peak_width is None else float(self.coulomb_peak_width)
        out = self._b.scan1d([0], axis, (float(min), float(max)), int(points), np.zeros((1, N)), np.zeros((1, N - 1)), 0.0,
                             frame=frame, gamma=gamma, occupations=True)
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        return (host(out["raw"]).astype(np.float64)[0][:, None], host(out["occupations"]).astype(np.float64)[0])

    def do1d_closed(self, gate, min, max, points, n_charge):
        """The reference's `do1d_closed(gate, min, max, points, n_charge)`: do1d_open's sweep with exactly `n_charge` carriers
        in the array, rendered as a one-row grid (the closed regime has the grid call alone).  Returns (signal (points, 1),
        n_closed (points, N)) float64."""
        N = self.n_dot
        axis, frame = self._gate_axis(gate)
        gamma = None if self.coulomb_peak_width is None else float(self.coulomb_peak_width)
        out = self._b.scan_grid_closed([0], axis, np.zeros(2 * N), (float(min), float(max)), (0.0, 0.0), int(points), 1,
                                       np.zeros((1, N)), np.zeros((1, N - 1)), n_charge, 0.0, frame=frame, gamma=gamma, occupations=True)
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        return (host(out["raw"]).astype(np.float64)[0, 0][:, None], host(out["occupations"]).astype(np.float64)[0, 0])

    def do2d_closed(self, x_gate, x_min, x_max, x_points, y_gate, y_min, y_max, y_points, n_charge):
        """The reference's `do2d_closed(..., n_charge)`: do2d_open's grid with exactly `n_charge` carriers in the array (the
        reference forgets to pass n_charge on; here it arrives).  Shapes, gate grammar and the one-frame rule of do2d_open."""
        return self.do2d_open(x_gate, x_min, x_max, x_points, y_gate, y_min, y_max, y_points, _n_charge=n_charge)

    def do2d_open(self, x_gate, x_min, x_max, x_points, y_gate, y_min, y_max, y_points, *, _n_charge=None):
        """The reference's `do2d_open(x_gate, x_min, x_max, x_points, y_gate, y_min, y_max, y_points)`
        (TunnelCoupledChargeSensed.py:270-289 over GateVoltageComposer.do2d): a noise-free x_points x y_points grid over two
        gates on the env's current device, every other gate, the sensor gate and the barriers at 0 -- the base point is zero, as
        the composer builds it; the peak width is the model's, as in do1d_open.  Returns (signal (y_points, x_points, 1), n_open
        (y_points, x_points, N)) float64: x runs along columns.  The gates follow the grammar of do1d_open.  One call has ONE
        frame: two physical gates (ints, "P{g}") render in the physical frame, two virtual axes ("vP{i}", "e{i}_{j}",
        "U{i}_{j}") in the virtual frame, and a pair that mixes the frames raises NotImplementedError (the composer adds a
        physical and a virtual grid; the backend's grid has one frame per call).  The composer's grid is the sum of its two 1-D
        grids, so it carries the virtual gate origin once per "vP" axis, sqrt(2) times per "U" axis and never per "e" or
        physical axis: twice for "vP" against "vP", 1 + sqrt(2) times for "vP" against "U", not at all for "e" against "e".
        The facade renders through the backend's scan_grid, whose virtual frame adds the origin exactly ONCE: a physical pair is
        the composer's grid, a virtual pair sits (multiplicity - 1) origins below it; with a zero origin all agree."""
        N = self.n_dot
        (x_axis, x_frame), (y_axis, y_frame) = self._gate_axis(x_gate), self._gate_axis(y_gate)
        if x_frame != y_frame:
            raise NotImplementedError(f"do2d_open({x_gate!r}, ..., {y_gate!r}, ...): one call has one frame, and {x_gate!r} is "
                                      f"{x_frame} while {y_gate!r} is {y_frame}; sweep two physical gates or two virtual axes")
        gamma = None if self.coulomb_peak_width is None else float(self.coulomb_peak_width)
        args = ([0], x_axis, y_axis, (float(x_min), float(x_max)), (float(y_min), float(y_max)), int(x_points), int(y_points),
                np.zeros((1, N)), np.zeros((1, N - 1)))
        if _n_charge is None:
            out = self._b.scan_grid(*args, 0.0, frame=x_frame, gamma=gamma, occupations=True)
        else:
            out = self._b.scan_grid_closed(*args, _n_charge, 0.0, frame=x_frame, gamma=gamma, occupations=True)
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        return (host(out["raw"]).astype(np.float64)[0][:, :, None], host(out["occupations"]).astype(np.float64)[0])

    def _grid_kT(self, T):
        """kT of a thermal grid by the rule of _thermal: the reference's line as written, T=None the device's sampled T"""
        if T is None:
            T = self.T
            if T is None or not np.isfinite(T):
                raise ValueError("T=None needs the device's own sampled temperature, and this device was loaded from raw "
                                 "parameter blocks, which carry none; pass T")
        return 8.617333262145e-5 * float(T)

    def do2d_thermal(self, x_gate, x_min, x_max, x_points, y_gate, y_min, y_max, y_points, T=None, n_charge=None):
        """do2d_open (n_charge None) or do2d_closed at the model's temperature: the grid of thermal_state_open /
        thermal_state_closed, rendered by the backend's scan_grid_thermal in one call -- the thermally broadened diagram.  Gate
        grammar, base point, frames and the one-frame rule are do2d_open's; `T` is converted as in thermal_state_open
        (kT = 8.617333262145e-5 * T; T=None is the device's own sampled T, and a device loaded from raw parameter blocks has none
        and raises ValueError).  Returns (signal (y_points, x_points, 1), n (y_points, x_points, N), var (y_points, x_points, N))
        float64."""
        N = self.n_dot
        (x_axis, x_frame), (y_axis, y_frame) = self._gate_axis(x_gate), self._gate_axis(y_gate)
        if x_frame != y_frame:
            raise NotImplementedError(f"do2d_thermal({x_gate!r}, ..., {y_gate!r}, ...): one call has one frame, and {x_gate!r} is "
                                      f"{x_frame} while {y_gate!r} is {y_frame}; sweep two physical gates or two virtual axes")
        kT = self._grid_kT(T)
        gamma = None if self.coulomb_peak_width is None else float(self.coulomb_peak_width)
        args = ([0], x_axis, y_axis, (float(x_min), float(x_max)), (float(y_min), float(y_max)), int(x_points), int(y_points),
                np.zeros((1, N)), np.zeros((1, N - 1)))
        out = self._b.scan_grid_thermal(*args, kT, 0.0, n_charge=n_charge, frame=x_frame, gamma=gamma, occupations=True, variance=True)
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        return (host(out["raw"]).astype(np.float64)[0][:, :, None], host(out["occupations"]).astype(np.float64)[0],
                host(out["variance"]).astype(np.float64)[0])

    def do1d_thermal(self, gate, min, max, points, T=None, n_charge=None):
        """do1d_open (n_charge None) or do1d_closed at the model's temperature, rendered as a one-row thermal grid.  Returns
        (signal (points, 1), n (points, N), var (points, N)) float64; `T` as in do2d_thermal."""
        N = self.n_dot
        axis, frame = self._gate_axis(gate)
        kT = self._grid_kT(T)
        gamma = None if self.coulomb_peak_width is None else float(self.coulomb_peak_width)
        args = ([0], axis, np.zeros(2 * N), (float(min), float(max)), (0.0, 0.0), int(points), 1, np.zeros((1, N)), np.zeros((1, N - 1)))
        out = self._b.scan_grid_thermal(*args, kT, 0.0, n_charge=n_charge, frame=frame, gamma=gamma, occupations=True, variance=True)
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        return (host(out["raw"]).astype(np.float64)[0, 0][:, None], host(out["occupations"]).astype(np.float64)[0, 0],
                host(out["variance"]).astype(np.float64)[0, 0])

    def do2d_response(self, x_gate, x_min, x_max, x_points, y_gate, y_min, y_max, y_points, T=None, n_charge=None):
        """do2d_thermal with the charge response along the two axes of the grid, rendered by the backend's scan_grid_response in
        one call: the lock-in diagram dS/dx, dS/dy and the slopes of the occupations, per unit of the swept gate values.  Gate
        grammar, base point, frames, the one-frame rule and `T` are do2d_thermal's.  Returns (signal (y_points, x_points, 1),
        dS/dx (y_points, x_points), dS/dy (y_points, x_points), d<n>/dx (y_points, x_points, N), d<n>/dy (y_points, x_points, N))
        float64."""
        N = self.n_dot
        (x_axis, x_frame), (y_axis, y_frame) = self._gate_axis(x_gate), self._gate_axis(y_gate)
        if x_frame != y_frame:
            raise NotImplementedError(f"do2d_response({x_gate!r}, ..., {y_gate!r}, ...): one call has one frame, and {x_gate!r} is "
                                      f"{x_frame} while {y_gate!r} is {y_frame}; sweep two physical gates or two virtual axes")
        kT = self._grid_kT(T)
        gamma = None if self.coulomb_peak_width is None else float(self.coulomb_peak_width)
        args = ([0], x_axis, y_axis, (float(x_min), float(x_max)), (float(y_min), float(y_max)), int(x_points), int(y_points),
                np.zeros((1, N)), np.zeros((1, N - 1)))
        out = self._b.scan_grid_response(*args, kT, 0.0, n_charge=n_charge, frame=x_frame, gamma=gamma,
                                         response=("dsignal_axes", "docc_axes"))
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        ds, dn = host(out["dsignal_axes"]).astype(np.float64)[0], host(out["docc_axes"]).astype(np.float64)[0]
        return (host(out["raw"]).astype(np.float64)[0][:, :, None], ds[..., 0], ds[..., 1], dn[..., 0], dn[..., 1])

    def do1d_response(self, gate, min, max, points, T=None, n_charge=None):
        """do1d_thermal with the charge response along the sweep, rendered as a one-row response grid.  Returns (signal
        (points, 1), dS/dx (points,), dS/dy (points,), d<n>/dx (points, N), d<n>/dy (points, N)) float64; the y axis of a sweep
        is the zero direction, so its derivatives are zero; `T` as in do2d_thermal."""
        N = self.n_dot
        axis, frame = self._gate_axis(gate)
        kT = self._grid_kT(T)
        gamma = None if self.coulomb_peak_width is None else float(self.coulomb_peak_width)
        args = ([0], axis, np.zeros(2 * N), (float(min), float(max)), (0.0, 0.0), int(points), 1, np.zeros((1, N)), np.zeros((1, N - 1)))
        out = self._b.scan_grid_response(*args, kT, 0.0, n_charge=n_charge, frame=frame, gamma=gamma,
                                         response=("dsignal_axes", "docc_axes"))
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        ds, dn = host(out["dsignal_axes"]).astype(np.float64)[0, 0], host(out["docc_axes"]).astype(np.float64)[0, 0]
        return (host(out["raw"]).astype(np.float64)[0, 0][:, None], ds[..., 0], ds[..., 1], dn[..., 0], dn[..., 1])

    def do2d_levels(self, x_gate, x_min, x_max, x_points, y_gate, y_min, y_max, y_points, n_levels=2, n_charge=None):
        """The energy levels over do2d_open's grid (n_charge None) or do2d_closed's: the grid of energy_levels_open /
        energy_levels_closed, rendered by the backend's scan_grid_levels in one call -- levels[..., 1] - levels[..., 0] is the gap
        map.  Gate grammar, base point, frames and the one-frame rule are do2d_open's.  Returns (levels (y_points, x_points,
        n_levels), hnorm (y_points, x_points)) float64."""
        N = self.n_dot
        (x_axis, x_frame), (y_axis, y_frame) = self._gate_axis(x_gate), self._gate_axis(y_gate)
        if x_frame != y_frame:
            raise NotImplementedError(f"do2d_levels({x_gate!r}, ..., {y_gate!r}, ...): one call has one frame, and {x_gate!r} is "
                                      f"{x_frame} while {y_gate!r} is {y_frame}; sweep two physical gates or two virtual axes")
        gamma = None if self.coulomb_peak_width is None else float(self.coulomb_peak_width)
        args = ([0], x_axis, y_axis, (float(x_min), float(x_max)), (float(y_min), float(y_max)), int(x_points), int(y_points),
                np.zeros((1, N)), np.zeros((1, N - 1)))
        out = self._b.scan_grid_levels(*args, 0.0, levels=int(n_levels), n_charge=n_charge, frame=x_frame, gamma=gamma)
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        return host(out["levels"]).astype(np.float64)[0], host(out["hnorm"]).astype(np.float64)[0]

    def do1d_levels(self, gate, min, max, points, n_levels=2, n_charge=None):
        """The energy levels over do1d_open's sweep (n_charge None) or do1d_closed's, rendered as a one-row levels grid.  Returns
        (levels (points, n_levels), hnorm (points,)) float64."""
        N = self.n_dot
        axis, frame = self._gate_axis(gate)
        gamma = None if self.coulomb_peak_width is None else float(self.coulomb_peak_width)
        args = ([0], axis, np.zeros(2 * N), (float(min), float(max)), (0.0, 0.0), int(points), 1, np.zeros((1, N)), np.zeros((1, N - 1)))
        out = self._b.scan_grid_levels(*args, 0.0, levels=int(n_levels), n_charge=n_charge, frame=frame, gamma=gamma)
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        return host(out["levels"]).astype(np.float64)[0, 0], host(out["hnorm"]).astype(np.float64)[0, 0]


class ArrayFacade:
    """`env.array` of the reference (a QarrayBaseClass) as far as its users outside step() need it: `model.cgd_full`,
    `model.charge_sensor_open` / `model.ground_state_open` (ModelFacade), `barrier_alpha`, `gate_ground_truth`, the scan geometry (`obs_voltage_min`, `obs_voltage_max`, `obs_image_size`,
    `num_dots`, `num_barrier_voltages`), the stateless single image `_get_charge_sensor_data` and `scan2d` over any two
    controls (the backend's scan2d), and the stateless `_get_obs` (qarray_base_class.py:171-229), rendered by the
    backend's probe on the current device without touching the episode; `_get_obs(..., noise=True)` runs the stochastic
    stages the env was created with, as the reference's call does, with fresh noise at every call (default: a clean scan).  The window is
    (obs_voltage_max - obs_voltage_min) / 2 around each gate voltage; it follows the device (`window_delta`) at every
    reset and may be overwritten, as the reference's scripts do, but must stay symmetric: the kernels hold one
    half-width per scan."""

    def __init__(self, backend, num_dots, resolution):
        self._b = backend
        self.model = ModelFacade(backend, num_dots)
        self.barrier_alpha = None
        self.gate_ground_truth = None
        self.num_dots = int(num_dots)
        self.num_barrier_voltages = int(num_dots) - 1
        self.obs_image_size = int(resolution)
        self.obs_channels = int(num_dots) - 1
        self.obs_voltage_min, self.obs_voltage_max = -1.0, 1.0            # qarray_base_class.py:38-39

    def _get_obs(self, gate_voltages, barrier_voltages=None, sensor_voltage=None, noise=False):
        assert (
            len(gate_voltages) == self.num_dots
        ), f"Incorrect gate voltage shape, expected {self.num_dots}, got {len(gate_voltages)}"
        if barrier_voltages is not None:
            assert (
                len(barrier_voltages) == self.num_dots - 1
            ), f"Incorrect barrier voltage shape, expected {self.num_dots - 1}, got {len(barrier_voltages)}"
        # qarray_base_class.py:142
        assert barrier_voltages is not None, "Barrier voltages must be provided for models with barriers"
        vmin, vmax = float(self.obs_voltage_min), float(self.obs_voltage_max)
        if not abs(vmin + vmax) <= 1e-12 * max(abs(vmin), abs(vmax), 1.0):
            raise ValueError(f"asymmetric scan window: obs_voltage_min = {vmin}, obs_voltage_max = {vmax}; the HIP kernels "
                             "hold one half-width per scan, so obs_voltage_min must equal -obs_voltage_max")
        out = self._b.probe([0], np.asarray(gate_voltages, np.float64)[None, :],
                            np.asarray(barrier_voltages, np.float64)[None, :],
                            sensor_voltage=None if sensor_voltage is None else float(sensor_voltage),
                            window=(vmax - vmin) / 2, **({"noise": True} if noise else {}))
        raw = out["raw"]
        raw = raw.detach().cpu().numpy() if hasattr(raw, "detach") else np.asarray(raw)
        image = np.ascontiguousarray(raw[0].transpose(1, 2, 0))           # (R, R, C) float64, unnormalised
        expected = (self.obs_image_size, self.obs_image_size, self.obs_channels)
        if image.shape != expected:
            raise ValueError(f"Image observation shape {image.shape} does not match expected {expected}")
        return {"image": image, "obs_gate_voltages": gate_voltages, "obs_barrier_voltages": barrier_voltages}

    def _get_charge_sensor_data(self, gate1, gate2, gate_voltages, barrier_voltages=None, sensor_voltage=None):
        """One (R, R) float64 image over the virtual gates `gate1` (columns) and `gate2` (rows), 1-indexed, each over the
        env's window around its voltage (qarray_base_class.py:95-168).  The reference asserts an adjacent pair; any two
        different gates in 1..N+1 are accepted (N+1 is the sensor gate)."""
        assert (
            len(gate_voltages) == self.num_dots
        ), f"Incorrect gate voltage shape, expected {self.num_dots}, got {len(gate_voltages)}"
        assert barrier_voltages is not None, "Barrier voltages must be provided for models with barriers"
        assert (
            len(barrier_voltages) == self.num_dots - 1
        ), f"Incorrect barrier voltage shape, expected {self.num_dots - 1}, got {len(barrier_voltages)}"
        G = self.num_dots + 1
        gate1, gate2 = int(gate1), int(gate2)
        if not (1 <= gate1 <= G and 1 <= gate2 <= G) or gate1 == gate2:
            raise ValueError(f"gate1 and gate2 must be two different gates in 1..{G}, got {gate1} and {gate2}")
        base = list(np.asarray(gate_voltages, np.float64)) + [0.0 if sensor_voltage is None else float(sensor_voltage)]
        vmin, vmax = float(self.obs_voltage_min), float(self.obs_voltage_max)
        ranges = [(base[g - 1] + vmin, base[g - 1] + vmax) for g in (gate1, gate2)]
        out = self.scan2d(gate1 - 1, gate2 - 1, ranges[0], ranges[1], gate_voltages, barrier_voltages,
                          sensor_voltage=sensor_voltage)
        return out["raw"]

    def scan2d(self, x, y, x_range, y_range, gate_voltages, barrier_voltages, sensor_voltage=None, **kw):
        """The backend's scan2d for this env: one query, numpy results without the query axis ("raw" (R, R), ...)."""
        out = self._b.scan2d([0], x, y, x_range, y_range, np.asarray(gate_voltages, np.float64)[None, :],
                             np.asarray(barrier_voltages, np.float64)[None, :],
                             sensor_voltage=None if sensor_voltage is None else float(sensor_voltage), **kw)
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        return {k: host(v)[0] for k, v in out.items()}

    def scan_affine(self, x, y, x_range, y_range, gate_voltages, barrier_voltages, sensor_voltage=None, **kw):
        """The backend's scan_affine for this env (axes such as "e1_2" and "U1_2", a {control: coefficient} dict or a (2N,)
        vector): one query, numpy results without the query axis ("raw" (R, R), ...)."""
        out = self._b.scan_affine([0], x, y, x_range, y_range, np.asarray(gate_voltages, np.float64)[None, :],
                                  np.asarray(barrier_voltages, np.float64)[None, :],
                                  sensor_voltage=None if sensor_voltage is None else float(sensor_voltage), **kw)
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        return {k: host(v)[0] for k, v in out.items()}

    def scan1d(self, axis, s_range, n_points, gate_voltages, barrier_voltages, sensor_voltage=None, **kw):
        """The backend's scan1d for this env (a dense sweep of n_points points along a control, "e1_2", "U1_2", a {control:
        coefficient} dict or a (2N,) vector): one query, numpy results without the query axis ("raw" (n,), "image" (n,),
        "plohi" (2,), "occupations" (n, N))."""
        out = self._b.scan1d([0], axis, s_range, n_points, np.asarray(gate_voltages, np.float64)[None, :],
                             np.asarray(barrier_voltages, np.float64)[None, :],
                             sensor_voltage=None if sensor_voltage is None else float(sensor_voltage), **kw)
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        return {k: host(v)[0] for k, v in out.items()}

    def scan_grid(self, x, y, x_range, y_range, nx, ny, gate_voltages, barrier_voltages, sensor_voltage=None, **kw):
        """The backend's scan_grid for this env (an nx x ny grid of points along two axes, as scan_affine takes them): one
        query, numpy results without the query axis ("raw" (ny, nx), "image" (ny, nx), "plohi" (2,), "occupations"
        (ny, nx, N))."""
        out = self._b.scan_grid([0], x, y, x_range, y_range, nx, ny, np.asarray(gate_voltages, np.float64)[None, :],
                                np.asarray(barrier_voltages, np.float64)[None, :],
                                sensor_voltage=None if sensor_voltage is None else float(sensor_voltage), **kw)
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        return {k: host(v)[0] for k, v in out.items()}

    def scan_grid_thermal(self, x, y, x_range, y_range, nx, ny, gate_voltages, barrier_voltages, kT, sensor_voltage=None, **kw):
        """The backend's scan_grid_thermal for this env (scan_grid at the temperature kT, open or with n_charge= closed): one
        query, numpy results without the query axis, "variance" (ny, nx, N) and "ztail" (ny, nx) among them when asked for."""
        out = self._b.scan_grid_thermal([0], x, y, x_range, y_range, nx, ny, np.asarray(gate_voltages, np.float64)[None, :],
                                        np.asarray(barrier_voltages, np.float64)[None, :], kT,
                                        sensor_voltage=None if sensor_voltage is None else float(sensor_voltage), **kw)
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        return {k: host(v)[0] for k, v in out.items()}

    def scan_grid_levels(self, x, y, x_range, y_range, nx, ny, gate_voltages, barrier_voltages, sensor_voltage=None, **kw):
        """The backend's scan_grid_levels for this env (scan_grid with the energy levels of every point, open or with n_charge=
        closed): one query, numpy results without the query axis, "levels" (ny, nx, L) and "hnorm" (ny, nx) and, for L >= 2,
        "gap" and "rel_gap" (ny, nx) among them."""
        out = self._b.scan_grid_levels([0], x, y, x_range, y_range, nx, ny, np.asarray(gate_voltages, np.float64)[None, :],
                                       np.asarray(barrier_voltages, np.float64)[None, :],
                                       sensor_voltage=None if sensor_voltage is None else float(sensor_voltage), **kw)
        host = lambda t: t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)    # noqa: E731
        return {k: host(v)[0] for k, v in out.items()}



class QuantumDeviceEnv:
    metadata = {"render_modes": []}

    def __init__(self, training=True, config_path="env_config.yaml", num_dots=None, use_barriers=None,
                 capacitance_model_checkpoint=None, capacitance_model=None, backend=None, seed=None,
                 qarray_config_path=None, num_charge_states=None):
        self.config = load_yaml(config_path if config_path != "env_config.yaml" else None, "env_config.yaml")
        sim = self.config["simulator"]
        self.training = training
        self.num_dots = num_dots if num_dots is not None else sim["num_dots"]
        self.use_barriers = use_barriers if use_barriers is not None else sim["use_barriers"]
        self.capacitance_model_checkpoint = capacitance_model_checkpoint
        self.use_deltas = sim["use_deltas"]
        self.max_steps = sim["max_steps"]
        self.num_plunger_voltages = self.num_dots
        self.num_barrier_voltages = self.num_dots - 1
        self.resolution = sim["resolution"]
        if not self.use_barriers:
            raise NotImplementedError("env.py only supports barrier mode for now")      # env.py:61-62
        N, C, R = self.num_dots, self.num_dots - 1, self.resolution
        self.action_space = spaces.Dict({
            "action_gate_voltages": spaces.Box(low=-1.0, high=1.0, shape=(N,), dtype=np.float32),
            "action_barrier_voltages": spaces.Box(low=-1.0, high=1.0, shape=(C,), dtype=np.float32)})
        self.obs_channels = C
        self.observation_space = spaces.Dict({
            "image": spaces.Box(low=0.0, high=1.0, shape=(R, R, C), dtype=np.float32),
            "obs_gate_voltages": spaces.Box(low=-1.0, high=1.0, shape=(N,), dtype=np.float32),
            "obs_barrier_voltages": spaces.Box(low=-1.0, high=1.0, shape=(C,), dtype=np.float32)})
        update_method = self.config["capacitance_model"]["update_method"]
        try:                                                   # env.py:680-802: same exception type
            if update_method in (None, "perfect", "fake"):                 # env.py:683-689: no CNN
                capacitance_model = None
            elif capacitance_model is None:
                if not capacitance_model_checkpoint:
                    raise ValueError("Capacitance model weights must be provided via capacitance_model_checkpoint "
                                     f"when using update_method '{update_method}'.")
                # env.py:716-749: CapacitancePredictionModel(output_size) + checkpoint, on the GPU
                from .capacitance_cnn import build_device_model
                nearest = self.config["capacitance_model"].get("nearest_neighbour", False)
                capacitance_model = build_device_model(checkpoint=capacitance_model_checkpoint,
                                                       output_size=2 if nearest else 3)
        except Exception as e:
            raise RuntimeError(f"Error initialising capacitance model: {e}")
        if backend is None:
            from .vec_env import VecQuantumDeviceEnv
            backend = VecQuantumDeviceEnv(1, num_dots=N, config_path=config_path if config_path != "env_config.yaml" else None,
                                          qarray_config_path=qarray_config_path, resolution=R,
                                          capacitance_model=capacitance_model, num_charge_states=num_charge_states,
                                          seed=seed)            # None: fresh entropy per env, as the reference's unseeded RNGs
        self._b = backend
        self.current_step = 0
        self.array = ArrayFacade(backend, N, R)
        self.reset()

    # -- helpers ---------------------------------------------------------------
    @staticmethod
    def _np(x):
        return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)

    def _observation(self, obs):
        return {"image": self._np(obs["image"])[0].copy(),
                "obs_gate_voltages": self._np(obs["obs_gate_voltages"])[0].copy(),
                "obs_barrier_voltages": self._np(obs["obs_barrier_voltages"])[0].copy()}

    def _refresh_device_state(self):
        ds = self._b.device_state()
        self.device_state = {
            "gate_ground_truth": ds["gate_ground_truth"][0], "barrier_ground_truth": ds["barrier_ground_truth"][0],
            "sensor_ground_truth": float(ds["sensor_ground_truth"][0]),
            "current_gate_voltages": ds["current_gate_voltages"][0],
            "current_barrier_voltages": ds["current_barrier_voltages"][0],
            "virtual_gate_matrix": ds["virtual_gate_matrix"][0], "virtual_gate_origin": ds["virtual_gate_origin"][0]}
        self.array.gate_ground_truth = self.device_state["gate_ground_truth"]
        ep = getattr(self._b, "last_episode", None)
        if ep is not None:
            self.array.model.cgd_full = ep.extras["cgd"][0]
            self.array.barrier_alpha = ep.extras["alpha"][0]

    def _get_info(self):
        return {"current_device_state": self.device_state}

    # -- gym API ----------------------------------------------------------------
    def reset(self, seed=None, options=None):
        self.current_step = 0
        obs = self._b.reset(seed=seed)
        self._refresh_device_state()
        ep, L = getattr(self._b, "last_episode", None), getattr(self._b, "L", None)
        if ep is not None and L is not None:                    # a new device brings its own window (window_delta)
            w = float(ep.params[0, L.scal + 2])
            self.array.obs_voltage_min, self.array.obs_voltage_max = -w, w
            self.array.model.coulomb_peak_width = float(ep.params[0, L.scal + 1])
        return self._observation(obs), self._get_info()

    def step(self, action, skip_obs=False):
        if skip_obs:
            raise NotImplementedError("skip_obs=True has no user in the reference and is not built")
        self.current_step += 1
        g = np.array(action["action_gate_voltages"]).flatten().astype(np.float32)
        b = np.array(action["action_barrier_voltages"]).flatten().astype(np.float32)
        act = np.concatenate([g, b])[None, :]
        obs, rewards, terminated, truncated = self._b.step(act)
        r = self._np(rewards)[0]
        self._refresh_device_state()
        reward = {"gates": r[:self.num_dots].copy(), "barriers": r[self.num_dots:].copy()}
        return (self._observation(obs), reward, bool(self._np(terminated)[0]), bool(self._np(truncated)[0]),
                self._get_info())

    def close(self):
        if hasattr(self._b, "close"):
            self._b.close()

    def _cleanup(self):
        pass
