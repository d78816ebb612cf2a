"""
Generate tests/golden/line_grids.npz: the voltage lines of the reference's importable GateVoltageComposer for 1-D sweeps,

    comp.do1d(gate, min, max, n)

(GateVoltageComposer.py:213-222 -> _parse_and_construct_scan :35-84), for its whole gate grammar -- a physical gate "P{g}", a
virtual plunger "vP{i}", detuning "e{i}_{j}" and the on-site axis "U{i}_{j}" -- which tests/test_line_cpu.py compares with the
line front end (csrc/qd_line.h: qd_line_voltages).  Run once where the reference tree is available:

    QD_REFERENCE_ROOT=<reference checkout> python tests/golden/make_golden_lines.py

The reference source file is loaded by path and executed unmodified; only INPUTS and OUTPUTS (arrays) are stored.  The
composer holds every gate that is not swept at 0.  A "P" sweep is physical: no matrix, no origin.  The virtual sweeps are
formed from _do1d_virtual terms, each of which carries the origin: "vP" adds it once, "U" = (v_i + v_j) / sqrt(2) adds it
sqrt(2) times, "e" = v_i - v_j not at all.  That multiplicity is stored per case.
Written with fixed zip time stamps: running it again gives the same bytes.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_axes import _load, _savez_fixed      # noqa: E402

# (n_dot, n, gate, kind): P, vP, e and U on adjacent, non-adjacent and reversed dot pairs, asymmetric ranges and a reversed
# range (lo > hi)
CASES = [
    (2, 5, "P1", "asym"), (2, 8, "vP2", "rev_range"), (2, 5, "e1_2", "asym"), (2, 8, "U2_1", "rev_range"),
    (4, 8, "P5", "rev_range"), (4, 5, "vP3", "asym"), (4, 8, "e1_3", "asym"), (4, 5, "U4_2", "rev_range"), (4, 8, "e3_2", "asym"),
    (8, 5, "P4", "asym"), (8, 8, "vP8", "asym"), (8, 5, "e7_2", "rev_range"), (8, 8, "U1_8", "asym"), (8, 5, "U4_5", "asym"),
]
ORIGIN_MULTIPLICITY = {"P": 0.0, "e": 0.0, "U": float(np.sqrt(2.0)), "v": 1.0}


def line_grids(ref_root):
    G = _load(os.path.join(ref_root, "src", "qarray_latched", "DotArrays", "GateVoltageComposer.py"), "ref_gvc")
    out = {}
    for case, (n_dot, n, gate, kind) in enumerate(CASES):
        rng = np.random.default_rng(500 + case)
        Gt = n_dot + 1
        vgm = -np.eye(Gt) + rng.normal(0, 0.2, size=(Gt, Gt))
        origin = rng.normal(0, 1.0, size=Gt)
        ranges = [-rng.uniform(0.5, 3.0), rng.uniform(3.0, 9.0)]
        if kind == "rev_range":
            ranges = ranges[::-1]
        ranges = [float(r) for r in ranges]
        comp = G.GateVoltageComposer(n_gate=Gt, n_dot=n_dot, n_sensor=1)
        comp.virtual_gate_matrix = vgm
        comp.virtual_gate_origin = origin
        vg = comp.do1d(gate, ranges[0], ranges[1], n)
        assert vg.shape == (n, Gt)
        for k, v in dict(n_dot=n_dot, n=n, gate=np.array(gate), vgm=vgm, origin=origin, ranges=np.array(ranges),
                         origin_multiplicity=ORIGIN_MULTIPLICITY[gate[0]], vg=vg).items():
            out[f"c{case}_{k}"] = np.asarray(v)
    out["n_cases"] = np.array(len(CASES))
    _savez_fixed(os.path.join(HERE, "line_grids.npz"), out)


if __name__ == "__main__":
    root = os.environ.get("QD_REFERENCE_ROOT") or (sys.argv[1] if len(sys.argv) > 1 else None)
    if not root:
        raise SystemExit("set QD_REFERENCE_ROOT (or pass the reference checkout as the first argument)")
    line_grids(root)
    print("line_grids.npz written to", HERE)
