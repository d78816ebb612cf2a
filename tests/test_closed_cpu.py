"""The closed regime's front on the CPU (no GPU): the host build of qd_closed_centre / qd_candidates_closed / qd_closed_record
(csrc/qd_closed.h, the source the device compiles) against the reference of tests/closed_helpers.py, N = 2..8.

Inputs: devices of the oracle's sampler; vg from U(-0.5, 4) for two thirds of the points and U(-3, 3) for the rest, vb from
U(-2, 2); every point at the six total charges {0, 1, Qs - 1, Qs, Qs + 1, 2N + 1}, Qs the rounded total of the open oracle's
occupations at that point.  Bounds: the centre within delta = 64 kappa_2(A) eps max(1, |v'|_inf, Q) (a backward-stable solve
of a system with condition kappa_2(A) and data of that size, with a factor 64 for the N <= 8 terms of its sums); floors and
list order are compared where the reference itself decides them (m_ref farther than delta from an integer >= 1, neighbouring
NumPy energies more than 1e-12 apart relative), and at most 2 % of a case may be exempt."""
import numpy as np
import pytest

import closed_helpers as CH
import helpers as H
import points_helpers as PH
import search_cases as SC
from qadapt_hip.layout import layout

NS = [2, 3, 4, 5, 6, 7, 8]
NPTS = {2: 48, 3: 48, 4: 48, 5: 36, 6: 30, 7: 15, 8: 12}
_CASES = {}


def _case(N):
    """One device per N, NPTS[N] points x 6 total charges; host results at KC = 32 and the reference, computed once."""
    if N not in _CASES:
        par = np.ascontiguousarray(H.sample_blocks(N, [9100 + N]).params[0])
        dev = H.dev_view(N, par)
        rng = np.random.default_rng(9200 + N)
        vg, vb = CH.points(N, rng, NPTS[N])
        qs, _ = CH.open_totals(dev, vg, vb)
        Q = np.array([CH.q_values(N, q) for q in qs]).reshape(-1)
        v_ext = np.repeat(np.concatenate([vg, vb], axis=1), 6, axis=0)
        host = CH.host_closed(N, par, v_ext, Q, 32)
        A = CH.sub_A(N, par)
        n = len(Q)
        mref = np.zeros((n, N)); nfree = np.zeros(n, int); delta = np.zeros(n)
        lists = []
        for p in range(n):
            mref[p], free = CH.m_ref(A, host["vd"][p], int(Q[p]))
            nfree[p] = len(free)
            delta[p] = CH.delta_bound(A, host["vd"][p], int(Q[p]))
            lists.append(CH.brute_list(A, host["vd"][p], np.floor(mref[p]).astype(np.int64), int(Q[p]), 32))
        # points whose floors the reference does not decide: a component within delta of an integer >= 1 (a lone free dot
        # holds exactly Q in the reference and in the code: its floor is not decided by rounding)
        near = (np.abs(mref - np.rint(mref)) <= delta[:, None]) & (np.rint(mref) >= 1) & (nfree > 1)[:, None]
        _CASES[N] = dict(par=par, dev=dev, A=A, Q=Q, v_ext=v_ext, host=host, mref=mref, nfree=nfree, delta=delta, lists=lists,
                         exempt=near.any(axis=1))
    return _CASES[N]


@pytest.mark.parametrize("N", NS)
def test_centre_against_the_enumeration(N):
    c = _case(N)
    err = np.abs(c["host"]["m"] - c["mref"]).max(axis=1)
    print(f"[closed centre] N={N}: {len(err)} points, worst |m - m_ref| {err.max():.3e} (delta >= {c['delta'].min():.3e}), rounds <= "
          f"{c['host']['rounds'].max()}, clamped dots in {int((c['nfree'] < N).sum())}, lone free dot in {int((c['nfree'] == 1).sum())}, "
          f"kappa {np.linalg.cond(c['A']):.3f}")
    assert np.all(err <= c["delta"]), float((err / c["delta"]).max())
    assert c["host"]["rounds"].max() <= 2 * N + 2
    assert np.all(c["host"]["m"] >= 0)


@pytest.mark.parametrize("N", NS)
def test_floors(N):
    c = _case(N)
    ex = c["exempt"]
    print(f"[closed floors] N={N}: exempt {int(ex.sum())} of {len(ex)}")
    assert ex.sum() <= 0.02 * len(ex)
    assert np.array_equal(c["host"]["fl"][~ex], np.floor(c["mref"][~ex]).astype(np.int32))
    # sum(fl) in (Q - N, Q]: a candidate always exists
    s = c["host"]["fl"].sum(axis=1)
    assert np.all((s > c["Q"] - N) & (s <= c["Q"])) and np.all(c["host"]["nvalid"] >= 1)


@pytest.mark.parametrize("N", NS)
def test_kept_list_against_the_brute_force(N):
    c = _case(N)
    host = c["host"]
    n_order_exempt = 0
    for p in np.nonzero(~c["exempt"])[0]:
        st, E, idx, Eall = c["lists"][p]
        nv = int(host["nvalid"][p])
        assert nv == len(idx) == min(32, len(Eall)), p
        assert set(host["idx"][p, :nv].tolist()) == set(idx.tolist()), p
        assert np.all(host["states"][p, :nv].sum(axis=1) == c["Q"][p]) and np.all(host["states"][p, :nv] >= 0)
        # the order, where NumPy's own energies decide it (the first nv + 1 sorted energies)
        e = Eall[:nv + 1]
        if np.all(np.diff(e) > 1e-12 * np.abs(e[1:])):
            assert np.array_equal(host["idx"][p, :nv], idx), p
            assert np.array_equal(host["states"][p, :nv], st), p
        else:
            n_order_exempt += 1
        assert np.allclose(host["E"][p, :nv], E * host["isa"][p], rtol=1e-12, atol=1e-12)
    print(f"[closed list] N={N}: order exempt {n_order_exempt} of {len(c['Q'])}")
    assert n_order_exempt <= 0.02 * len(c["Q"])


@pytest.mark.parametrize("N", NS)
def test_sector_members_of_the_open_list_at_the_same_centre(N):
    """Every entry of the open host search run with ncont := m whose state sums to Q is in the closed list with the same
    energy bits, the same index and in the same relative order; at N = 2 (16 candidates) that is the whole closed list."""
    c = _case(N)
    host = c["host"]
    op = CH.host_open_at(N, c["par"], host["vd"], host["m"], host["isa"], 32)
    assert np.array_equal(op["fl"], host["fl"])
    st_open = CH.states_of(op["fl"], op["idx"])
    found = 0
    for p in range(len(c["Q"])):
        nvo, nv = int(op["nvalid"][p]), int(host["nvalid"][p])
        member = np.nonzero(st_open[p, :nvo].sum(axis=1) == c["Q"][p])[0]
        pos = {int(i): k for k, i in enumerate(host["idx"][p, :nv])}
        where = [pos.get(int(op["idx"][p, k]), -1) for k in member]
        assert all(w >= 0 for w in where), p
        assert where == sorted(where), p
        assert PH.same(host["E"][p, where], op["E"][p, member]), p
        found += len(member)
        if N == 2:
            assert len(member) == nv, p
    assert found > 0


@pytest.mark.parametrize("name", ["dyadic", "exchange"])
@pytest.mark.parametrize("KC", SC.KS)
def test_exact_ties_follow_the_index(name, KC):
    """dyadic (4, 33) and exchange (4, 33) of tests/search_cases.py: every energy is an exact float64, equal energies are equal
    bit for bit, and the closed list is the NumPy (E, idx) order, ties included.  The points are the pixels of channel 0 at
    Q = 6 (four dots at 1.5 electrons) and 5."""
    N, R = 4, 33
    par, st = SC.make(name, N, R)
    v_ext = PH.scan_voltages(N, par, st, 0, R)[0][::3]
    A = CH.sub_A(N, par)
    ties = 0
    for Q in (6, 5):
        host = CH.host_closed(N, par, v_ext, Q, KC)
        for p in range(v_ext.shape[0]):
            stt, E, idx, Eall = CH.brute_list(A, host["vd"][p], host["fl"][p].astype(np.int64), Q, KC)
            nv = int(host["nvalid"][p])
            assert nv == len(idx)
            assert np.array_equal(host["idx"][p, :nv], idx), (Q, p)
            assert PH.same(host["E"][p, :nv], E * host["isa"][p]), (Q, p)
            ties += int(np.any(np.diff(Eall[:nv + 1]) == 0))
    print(f"[closed ties] {name} K={KC}: points with an exact tie inside or at the edge of the list {ties}")
    assert ties > 0


@pytest.mark.parametrize("N", NS)
def test_properties(N):
    c = _case(N)
    host, Q = c["host"], c["Q"]
    z = Q == 0
    assert z.any() and np.all(host["nvalid"][z] == 1) and np.all(host["states"][z] == 0) and np.all(host["m"][z] == 0)
    # a lone free dot holds exactly Q
    lone = (host["m"] > 0).sum(axis=1) == 1
    assert np.all(host["m"][lone].max(axis=1) == Q[lone])
    # fewer than K candidates: idx 0 and the largest kept energy behind them
    short = np.nonzero(host["nvalid"] < 32)[0]
    if N <= 3:
        assert len(short) == len(Q)
    for p in short:
        nv = int(host["nvalid"][p])
        assert np.all(host["idx"][p, nv:] == 0) and np.all(host["states"][p, nv:] == 0)
        assert np.all(PH.bits(host["E"][p, nv:]) == PH.bits(host["E"][p, nv - 1:nv]))
        assert np.all(np.diff(host["E"][p, :nv]) >= 0)


@pytest.mark.parametrize("N", [2, 3, 4, 6, 8])
def test_classical_limit_first_state_is_the_open_ground_state(N):
    """tc_base = 0: the open oracle's occupations are its lowest state; the first closed state at Q = sum(n_open) is that state."""
    L = layout(N)
    par = np.ascontiguousarray(H.sample_blocks(N, [9300 + N]).params[0]).copy()
    par[L.scal] = 0.0
    dev = H.dev_view(N, par)
    vg, vb = CH.points(N, np.random.default_rng(9400 + N), 72)
    qs, n_open = CH.open_totals(dev, vg, vb)
    assert np.all(n_open == np.rint(n_open))
    host = CH.host_closed(N, par, np.concatenate([vg, vb], axis=1), qs, 32)
    same = np.all(host["states"][:, 0] == n_open.astype(np.int32), axis=1)
    print(f"[closed classical] N={N}: {int(same.sum())} of {len(same)}")
    assert same.all()


def test_closed_front_under_the_sanitizers():
    """tests/hosttest_closed/qd_closed_asan: a program of its own (nothing is loaded into Python), built with
    -fsanitize=address,undefined, that runs centre, search and record with the kept buffers and the record in heap blocks of
    exactly their size, total charges from 0 to 32767 included, and checks the lists' invariants."""
    import os
    import subprocess
    hdir = os.path.join(H.ROOT, "tests", "hosttest_closed")
    subprocess.check_call(["make", "-s", "-C", hdir, "qd_closed_asan"])
    r = subprocess.run([os.path.join(hdir, "qd_closed_asan")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "closed asan ok" in r.stdout
