"""
Generate tests/golden/axis_grids.npz: the voltage grids of the reference's importable GateVoltageComposer for 2-D scans
over ANY two virtual plungers and ranges,

    comp.do2d("vP{i}", x_min, x_max, R, "vP{j}", y_min, y_max, R, gate_voltages, True)

(GateVoltageComposer.py:224-251 -> meshgrid_virtual_coupled :170-211), which tests/test_scan_cpu.py compares with the scan
front end (csrc/qd_pixel.h: qd_scan_voltages).  Run once where the reference tree is available:

    QD_REFERENCE_ROOT=<reference checkout> python tests/golden/make_golden_axes.py

The reference source file is loaded by path and executed unmodified; only INPUTS and OUTPUTS (arrays) are stored.  The
composer checks both gates with _check_dot (1..n_dot), so the sensor dot is NOT an axis it accepts and no such case is here.
Written with fixed zip time stamps: running it again gives the same bytes.
"""
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# (n_dot, R, x dot, y dot (1-indexed), kind): non-adjacent pairs, reversed pairs (x index > y index), asymmetric ranges, a
# reversed range (lo > hi)
CASES = [
    (2, 5, 1, 2, "asym"), (2, 8, 2, 1, "asym"), (2, 5, 2, 1, "rev_range"),
    (4, 8, 1, 3, "asym"), (4, 5, 4, 1, "asym"), (4, 8, 3, 2, "sym"), (4, 5, 2, 4, "rev_range"),
    (8, 8, 1, 8, "asym"), (8, 5, 7, 2, "asym"), (8, 8, 5, 3, "rev_range"), (8, 5, 3, 6, "sym"),
]


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _savez_fixed(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def axis_grids(ref_root):
    G = _load(os.path.join(ref_root, "src", "qarray_latched", "DotArrays", "GateVoltageComposer.py"), "ref_gvc")
    out = {}
    for case, (n_dot, R, xd, yd, kind) in enumerate(CASES):
        rng = np.random.default_rng(100 + case)
        Gt = n_dot + 1
        vgm = -np.eye(Gt) + rng.normal(0, 0.2, size=(Gt, Gt))
        origin = rng.normal(0, 1.0, size=Gt)
        gv = rng.uniform(-30, 30, size=n_dot)
        sensor = float(rng.uniform(-1, 1))
        if kind == "sym":
            w = float(rng.uniform(1.5, 2.0))
            ranges = [gv[xd - 1] - w, gv[xd - 1] + w, gv[yd - 1] - w, gv[yd - 1] + w]
        else:
            ranges = [gv[xd - 1] - rng.uniform(0.5, 3.0), gv[xd - 1] + rng.uniform(3.0, 9.0),
                      gv[yd - 1] - rng.uniform(4.0, 6.0), gv[yd - 1] + rng.uniform(0.1, 1.0)]
            if kind == "rev_range":
                ranges = [ranges[1], ranges[0], ranges[2], ranges[3]]
        ranges = [float(r) for r in ranges]
        comp = G.GateVoltageComposer(n_gate=Gt, n_dot=n_dot, n_sensor=1)
        comp.virtual_gate_matrix = vgm
        comp.virtual_gate_origin = origin
        vg = comp.do2d(f"vP{xd}", ranges[0], ranges[1], R, f"vP{yd}", ranges[2], ranges[3], R,
                       np.concatenate([gv, [sensor]]), True)
        assert vg.shape == (R, R, Gt)
        for k, v in dict(n_dot=n_dot, R=R, x_dot=xd, y_dot=yd, vgm=vgm, origin=origin, gate_voltages=gv, sensor=sensor,
                         ranges=np.array(ranges), vg=vg).items():
            out[f"c{case}_{k}"] = np.asarray(v)
    out["n_cases"] = np.array(len(CASES))
    _savez_fixed(os.path.join(HERE, "axis_grids.npz"), out)


if __name__ == "__main__":
    root = os.environ.get("QD_REFERENCE_ROOT") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not root:
        raise SystemExit("set QD_REFERENCE_ROOT (or pass the reference checkout as the first argument)")
    axis_grids(root)
    print("axis_grids.npz written to", HERE)
