"""
Generate tests/golden/grid_grids.npz: the voltage grids of the reference's importable GateVoltageComposer for 2-D scans whose
two axes have DIFFERENT point counts,

    comp.do2d(x_axis, x_min, x_max, nx, y_axis, y_min, y_max, ny)        nx != ny

(GateVoltageComposer.py:224-255 -> _parse_and_construct_scan :35-84) over physical gates "P{g}", virtual plungers "vP{i}",
detuning "e{i}_{j}" and the on-site axis "U{i}_{j}", which tests/test_grid_cpu.py compares with the grid front end
(csrc/qd_grid.h: qd_grid_voltages).  Run once where the reference tree is available:

    QD_REFERENCE_ROOT=<reference checkout> python tests/golden/make_golden_grids.py

The reference source file is loaded by path and executed unmodified; only INPUTS and OUTPUTS (arrays) are stored.  Without
crosstalk the composer holds every gate that is not swept at 0 and adds its two 1-D grids: a "P" axis is rendered without
matrix or origin, a "vP" axis adds the origin once, a "U" axis (v_i + v_j) / sqrt(2) adds it sqrt(2) times, an "e" axis
v_i - v_j not at all.  The multiplicity of the pair (the sum of the two) is stored per case.  Pairs are of one frame: two "P"
gates, or two of "vP", "e", "U".
Written with fixed zip time stamps: running it again gives the same bytes.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_axes import _load, _savez_fixed      # noqa: E402

# (n_dot, nx, ny, x axis, y axis, kind): P x P, vP x vP, e x U, e x vP and U x vP pairs, the sensor gate as a physical axis,
# non-adjacent and reversed dot pairs, wide, tall and one-line grids, asymmetric ranges and a reversed range (lo > hi)
CASES = [
    (2, 5, 3, "P1", "P2", "asym"), (2, 3, 5, "vP1", "vP2", "rev_range"), (2, 8, 1, "e1_2", "U1_2", "asym"),
    (2, 1, 8, "U2_1", "vP1", "rev_range"),
    (4, 7, 2, "P2", "P5", "rev_range"), (4, 3, 5, "vP4", "vP1", "asym"), (4, 5, 3, "e1_3", "U1_3", "asym"),
    (4, 2, 7, "e4_2", "vP3", "rev_range"),
    (8, 6, 4, "P8", "P3", "asym"), (8, 4, 6, "vP5", "vP6", "rev_range"), (8, 5, 3, "e7_2", "U6_3", "rev_range"),
    (8, 3, 5, "U2_7", "vP4", "asym"),
]
ORIGIN_MULTIPLICITY = {"P": 0.0, "e": 0.0, "U": float(np.sqrt(2.0)), "v": 1.0}


def grid_grids(ref_root):
    G = _load(os.path.join(ref_root, "src", "qarray_latched", "DotArrays", "GateVoltageComposer.py"), "ref_gvc")
    out = {}
    for case, (n_dot, nx, ny, xa, ya, kind) in enumerate(CASES):
        rng = np.random.default_rng(500 + case)
        Gt = n_dot + 1
        vgm = -np.eye(Gt) + rng.normal(0, 0.2, size=(Gt, Gt))
        origin = rng.normal(0, 1.0, size=Gt)
        ranges = [-rng.uniform(0.5, 3.0), rng.uniform(3.0, 9.0), -rng.uniform(4.0, 6.0), rng.uniform(0.1, 1.0)]
        if kind == "rev_range":
            ranges = [ranges[1], ranges[0], ranges[2], ranges[3]]
        ranges = [float(r) for r in ranges]
        comp = G.GateVoltageComposer(n_gate=Gt, n_dot=n_dot, n_sensor=1)
        comp.virtual_gate_matrix = vgm
        comp.virtual_gate_origin = origin
        vg = comp.do2d(xa, ranges[0], ranges[1], nx, ya, ranges[2], ranges[3], ny)
        assert vg.shape == (ny, nx, Gt), vg.shape
        mult = ORIGIN_MULTIPLICITY[xa[0]] + ORIGIN_MULTIPLICITY[ya[0]]
        for k, v in dict(n_dot=n_dot, nx=nx, ny=ny, x_axis=np.array(xa), y_axis=np.array(ya), vgm=vgm, origin=origin,
                         ranges=np.array(ranges), origin_multiplicity=mult, vg=vg).items():
            out[f"c{case}_{k}"] = np.asarray(v)
    out["n_cases"] = np.array(len(CASES))
    _savez_fixed(os.path.join(HERE, "grid_grids.npz"), out)


if __name__ == "__main__":
    root = os.environ.get("QD_REFERENCE_ROOT") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not root:
        raise SystemExit("set QD_REFERENCE_ROOT (or pass the reference checkout as the first argument)")
    grid_grids(root)
    print("grid_grids.npz written to", HERE)
