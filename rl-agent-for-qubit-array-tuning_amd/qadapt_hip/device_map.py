"""
Device-range maps: the reference's map_full_device_range.py and map_device_range.py
(src/qadapt/environment/) on the batched kernels.  Each script tiles a plunger range of one device with
hundreds of `env.array._get_obs` calls and stitches the first channel with NumPy; here ALL tiles of a device are
one `VecQuantumDeviceEnv.probe` call and the stitching and normalisation one `compose` call, both on the GPU, and
the episode the env is in is not disturbed.  No figures are drawn; `save_npz` stores what the scripts pickle.

One deliberate deviation.  The scripts write each tile's ABSOLUTE edges into `env.array.obs_voltage_min / _max`,
which `_get_charge_sensor_data` (qarray_base_class.py:130-131) ADDS to the gate voltages again, using gate 0's
edges for both axes: the images the scripts save are not at the `positions` they save beside them.  The helpers here
render every tile at its saved position (centre +- half the window on both axes), which is what the scripts'
docstrings and plot extents describe.  Two smaller points follow from rendering in float64: the tile centres are not
rounded through the float32 ground-truth array the scripts copy them into, and `pair=i` maps gates (i, i+1) from
channel i where the scripts fix i = 0.
"""
from __future__ import annotations

import numpy as np


def tile_plan_full_range(plunger_min, plunger_max, window_size):
    """The tiling of map_full_device_range.py:66-122 for the two gates' ranges `plunger_min[0:2]`, `plunger_max[0:2]` and
    the full window width `window_size`: ceil(range / window) scans per axis, step = range / n (0 for a single scan,
    which therefore sits at the range's minimum, as in the script), centre (i + 0.5) * step above the minimum.
    Returns n_scans_x, n_scans_y, step_x, step_y, centres (nx*ny, 2) and positions, a list of
    (scan_min_v0, scan_max_v0, scan_min_v1, scan_max_v1), scan (i, j) at index i * n_scans_y + j."""
    v0_range = plunger_max[0] - plunger_min[0]
    v1_range = plunger_max[1] - plunger_min[1]
    n_scans_x = int(np.ceil(v0_range / window_size))
    n_scans_y = int(np.ceil(v1_range / window_size))
    step_x = v0_range / n_scans_x if n_scans_x > 1 else 0
    step_y = v1_range / n_scans_y if n_scans_y > 1 else 0
    centres, positions = [], []
    for i in range(n_scans_x):
        for j in range(n_scans_y):
            center_v0 = plunger_min[0] + (i + 0.5) * step_x
            center_v1 = plunger_min[1] + (j + 0.5) * step_y
            centres.append((center_v0, center_v1))
            positions.append((center_v0 - window_size / 2, center_v0 + window_size / 2,
                              center_v1 - window_size / 2, center_v1 + window_size / 2))
    return {"n_scans_x": n_scans_x, "n_scans_y": n_scans_y, "step_x": step_x, "step_y": step_y,
            "centres": np.asarray(centres, np.float64).reshape(-1, 2), "positions": positions}


def tile_plan_centred(gt0, gt1, half_range=20.0, window_size=3.0):
    """The tiling of map_device_range.py:36-88: the range gt +- half_range on both gates, ceil(range / window) scans per
    axis placed edge to edge from the minimum (the last one may reach past the maximum), centre = middle of the edges.
    Returns v0_min, v0_max, v1_min, v1_max, n_scans_x, n_scans_y, step_x, step_y, centres (nx*ny, 2) and positions, a
    list of (center_v0, center_v1, scan_min_v0, scan_max_v0, scan_min_v1, scan_max_v1), scan (i, j) at i * n_scans_y + j."""
    v0_min = gt0 - half_range
    v0_max = gt0 + half_range
    v1_min = gt1 - half_range
    v1_max = gt1 + half_range
    v0_range = v0_max - v0_min
    v1_range = v1_max - v1_min
    n_scans_x = int(np.ceil(v0_range / window_size))
    n_scans_y = int(np.ceil(v1_range / window_size))
    step_x = window_size
    step_y = window_size
    centres, positions = [], []
    for i in range(n_scans_x):
        for j in range(n_scans_y):
            scan_min_v0 = v0_min + i * step_x
            scan_max_v0 = scan_min_v0 + window_size
            scan_min_v1 = v1_min + j * step_y
            scan_max_v1 = scan_min_v1 + window_size
            center_v0 = (scan_min_v0 + scan_max_v0) / 2
            center_v1 = (scan_min_v1 + scan_max_v1) / 2
            centres.append((center_v0, center_v1))
            positions.append((center_v0, center_v1, scan_min_v0, scan_max_v0, scan_min_v1, scan_max_v1))
    return {"v0_min": v0_min, "v0_max": v0_max, "v1_min": v1_min, "v1_max": v1_max,
            "n_scans_x": n_scans_x, "n_scans_y": n_scans_y, "step_x": step_x, "step_y": step_y,
            "centres": np.asarray(centres, np.float64).reshape(-1, 2), "positions": positions}


def _device(env, env_index):
    """Ground truths (float64 of the float32 values the reference's info dict carries), window half-width and plunger
    ranges of env `env_index` of a VecQuantumDeviceEnv (one blocking state read)."""
    ds = env.device_state()
    L, par = env.L, env._params_host[env_index]
    return (ds["gate_ground_truth"][env_index].astype(np.float64), ds["barrier_ground_truth"][env_index].astype(np.float64),
            float(par[L.scal + 2]), par[L.pmin:L.pmin + L.N].copy(), par[L.pmax:L.pmax + L.N].copy())


def _render(env, env_index, pair, plan, gt_gates, gt_barriers, half_width, mode, noise=None):
    """All tiles of `plan` in one probe (gates pair, pair+1 at the tile centres, the others at their ground truth, the
    barriers at theirs, sensor voltage 0.0 as the scripts' _get_obs calls) and one compose of channel `pair`."""
    nq = plan["n_scans_x"] * plan["n_scans_y"]
    gates = np.tile(gt_gates, (nq, 1))
    gates[:, pair] = plan["centres"][:, 0]
    gates[:, pair + 1] = plan["centres"][:, 1]
    kw = {} if noise is None else {"noise": noise}
    out = env.probe([env_index], gates, np.tile(gt_barriers, (nq, 1)), window=half_width, **kw)
    comp, plohi = env.compose(out["raw"], plan["n_scans_x"], plan["n_scans_y"], channel=pair, mode=mode)
    return out["raw"][:, pair], comp, plohi


def map_full_device_range(env, env_index=0, pair=0, v0_min=None, v0_max=None, v1_min=None, v1_max=None, noise=None):
    """map_full_device_range.py on env `env_index` of a VecQuantumDeviceEnv: its plunger range of gates (pair, pair+1)
    (or the overrides) tiled with the device's own scan window, one probe + one compose, composite normalised by ONE
    0.5 / 99.5 percentile pair (row block j = scan row j: plot with origin='lower').  Tiles are rendered at their saved
    `positions` (see the module docstring for this deviation from the script).  Returns the dict the script pickles
    (`scans` as a (nx*ny, R, R) float64 device tensor, scan (i, j) at i * n_scans_y + j) plus `composite`
    (ny*R, nx*R) float32 and `plohi` (2,) device tensors and `extent`.  noise: handed to `probe` (None: clean scans; True:
    the env's own stochastic stages, so tiles beyond `full_noise_distance` are white noise as in the reference's maps)."""
    gt_gates, gt_barriers, w, pmin, pmax = _device(env, env_index)
    plunger_min = pmin[pair:pair + 2].copy()
    plunger_max = pmax[pair:pair + 2].copy()
    if v0_min is not None:
        plunger_min[0] = v0_min
    if v0_max is not None:
        plunger_max[0] = v0_max
    if v1_min is not None:
        plunger_min[1] = v1_min
    if v1_max is not None:
        plunger_max[1] = v1_max
    obs_window_size = w - (-w)                                   # obs_voltage_max - obs_voltage_min
    plan = tile_plan_full_range(plunger_min, plunger_max, obs_window_size)
    scans, comp, plohi = _render(env, env_index, pair, plan, gt_gates, gt_barriers, obs_window_size / 2, "global", noise)
    return {"scans": scans, "positions": plan["positions"], "n_scans_x": plan["n_scans_x"], "n_scans_y": plan["n_scans_y"],
            "resolution": env.R, "plunger_min": plunger_min, "plunger_max": plunger_max, "obs_window_size": obs_window_size,
            "step_x": plan["step_x"], "step_y": plan["step_y"], "gt_gates": gt_gates, "gt_barriers": gt_barriers,
            "centres": plan["centres"], "composite": comp, "plohi": plohi,
            "extent": [plunger_min[0], plunger_max[0], plunger_min[1], plunger_max[1]]}


def map_device_range(env, env_index=0, pair=0, percentile=None, half_range=20.0, window_size=3.0, noise=None):
    """map_device_range.py on env `env_index`: +- half_range around the ground truth of gates (pair, pair+1) in
    edge-to-edge scans `window_size` wide, every scan normalised by its own percentiles, row blocks flipped (block
    ny-1-j holds scan row j, as the script stitches them).  percentile: the script's optional cap, applied to the
    composite (one host round trip).  Tiles are rendered at their saved `positions` (module docstring).  Returns the
    dict the script pickles plus `composite` (ny*R, nx*R) float32 and `plohi` (nx*ny, 2) device tensors.  noise: handed to
    `probe`, as in map_full_device_range."""
    gt_gates, gt_barriers, _, _, _ = _device(env, env_index)
    plan = tile_plan_centred(gt_gates[pair], gt_gates[pair + 1], half_range, window_size)
    scans, comp, plohi = _render(env, env_index, pair, plan, gt_gates, gt_barriers, window_size / 2, "per_scan", noise)
    if percentile is not None:
        p_cap = float(np.percentile(comp.cpu().numpy().astype(np.float64), percentile))
        comp = (comp.clamp(0, p_cap) / p_cap) if p_cap > 0 else comp
    out = {k: plan[k] for k in ("positions", "n_scans_x", "n_scans_y", "v0_min", "v0_max", "v1_min", "v1_max",
                                "step_x", "step_y", "centres")}
    out.update({"scans": scans, "resolution": env.R, "scan_window_size": window_size, "gt_gates": gt_gates,
                "gt_barriers": gt_barriers, "composite": comp, "plohi": plohi,
                "extent": [plan["v0_min"], plan["v0_max"], plan["v1_min"], plan["v1_max"]]})
    return out


def save_npz(path, result):
    """A map's dict as one compressed .npz (device tensors are copied to the host)."""
    flat = {}
    for k, v in result.items():
        flat[k] = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
    np.savez_compressed(path, **flat)
    return path
