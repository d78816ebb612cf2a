"""The designed devices of tests/search_cases.py without a GPU: the host build of the exact per-pixel search
(csrc/qd_pixel.h through tests/hosttest) against the plain-C 4^N scan, bit for bit, and the conditions that make each family
what it is, asserted so that a later edit of a family cannot defuse it.  The device code runs the same members in
tests/test_gpu_search_adversarial.py."""
import os
import subprocess

import numpy as np
import pytest

import helpers as H
import qd_oracle_c as OC
import search_cases as SC
from qadapt_hip.layout import layout


def _channels(N):
    return list(range(N - 1)) if N <= 6 else [0, N - 2]


_REF = {}


def oracle(name, N, R, ch):
    """the C oracle's channel of a member (computed once, shared, read-only)"""
    if (name, N, R, ch) not in _REF:
        par, st = SC.make(name, N, R)
        dev = H.dev_view(N, par); sv = H.state_view(N, st)
        ref = OC.csd_channel(dev, sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, sv.barrier_v, dev.window, ch, R)
        for v in ref.values():
            v.setflags(write=False)
        _REF[(name, N, R, ch)] = ref
    return _REF[(name, N, R, ch)]


def _members(*names):
    return [m for m in SC.MEMBERS if m[0] in names]


@pytest.mark.parametrize("name,N,R", SC.MEMBERS)
def test_host_search_equals_brute_force(name, N, R):
    par, st = SC.make(name, N, R)
    for ch in _channels(N):
        ref = oracle(name, N, R, ch)
        hf = H.host_front(N, par, st, ch, R)
        assert np.array_equal(hf["floors"], ref["floors"]), ch
        assert (hf["nvalid"] == 32).all()
        bad = (hf["states"] != ref["states"]).any(axis=(1, 2))
        assert not bad.any(), (ch, int(bad.sum()), np.nonzero(bad)[0][:8])


def test_the_designed_block_is_consistent():
    """what make() writes: A = U U^T with U upper, v' = the virtual plunger voltages, an exact step for every R"""
    for name, N, R in SC.MEMBERS:
        par, st = SC.make(name, N, R)
        L = layout(N); G = N + 1
        A = par[L.cdd_inv:L.cdd_inv + G * G].reshape(G, G)
        U = par[L.ufac:L.ufac + N * N].reshape(N, N)
        assert np.array_equal(A[:N, :N], A[:N, :N].T) and np.array_equal(U, np.triu(U))
        assert np.allclose(U @ U.T, A[:N, :N], rtol=0, atol=1e-15)
        assert np.array_equal(par[L.uinv:L.uinv + N], 1 / np.diag(U))
        hf = H.host_front(N, par, st, 0, R)
        vd, _ = SC.v_dash(N, par, st, 0, R)
        assert np.array_equal(hf["vd"], vd)
        if name in SC.EXACT:                                    # the sweep is exactly gate - w + i * step
            x = vd[:R, 0]
            assert np.array_equal(np.diff(x), np.full(R - 1, x[1] - x[0])) and (x * 64 == np.round(x * 64)).all()


@pytest.mark.parametrize("name,N,R", [m for m in SC.MEMBERS if m[0] in SC.EXACT and m[1] <= 5])
def test_exact_families_numpy_scan_equals_canonical_energies(name, N, R):
    """every energy of these families is an exact float64, so the NumPy scan, whatever its summation order, gives the bits
    of the canonical fma chains and the order of the oracle: `E[K-1] == E[K]` below really is a tie of the kernels' numbers"""
    par, st = SC.make(name, N, R)
    for ch in _channels(N):
        ref = oracle(name, N, R, ch)
        E, order = SC.brute_force(N, par, st, ch, R, ref["floors"])
        hf = H.host_front(N, par, st, ch, R)
        assert np.array_equal(E[:, :32], hf["energies"])
        assert np.array_equal(SC.states_of(ref["floors"], order, 32), ref["states"])


@pytest.mark.parametrize("name,N,R", _members(*SC.TIE_FAMILIES))
def test_tie_families_tie_at_the_boundary_of_the_kept_set(name, N, R):
    """at least 10 % of the pixels have E[K-1] == E[K] exactly for K = 8, 16 and 32 (measured with this scan on the CPU:
    see the printed shares); the 8-dot member through the split scan `lowest_energies`, checked against the host energies"""
    par, st = SC.make(name, N, R)
    for ch in (0, N - 2):
        ref = oracle(name, N, R, ch)
        if N <= 5:
            E, _ = SC.brute_force(N, par, st, ch, R, ref["floors"])
            for K in SC.KS:
                share = float((E[:, K - 1] == E[:, K]).mean())
                print(f"[ties] {name} N={N} R={R} ch={ch} K={K}: {share:.2f}")
                assert share >= 0.10, (K, share)
            inside = (np.diff(E[:, :32], axis=1) == 0).sum(axis=1)
            assert inside.min() > 0                              # every pixel has tied neighbours inside its kept list
        else:
            E = SC.lowest_energies(N, par, st, ch, R, ref["floors"], 33)
            assert np.array_equal(E[:, :32], H.host_front(N, par, st, ch, R)["energies"])     # exact: the canonical energies
            for K in SC.KS:
                share = float((E[:, K - 1] == E[:, K]).mean())
                print(f"[ties] {name} N={N} R={R} ch={ch} K={K}: {share:.2f}")
                assert share >= 0.10, (K, share)
            assert float((E[:, 0] == E[:, 1]).mean()) > 0


def _tiles(a, R):
    """a (P, ...) -> list of the 8x8 tiles' pixel blocks"""
    a = a.reshape(R, R, -1)
    return [a[y:y + 8, x:x + 8].reshape(-1, a.shape[2]) for y in range(0, R, 8) for x in range(0, R, 8)]


@pytest.mark.parametrize("name,N,R", _members("straddle"))
def test_straddle_has_both_sides_of_the_packed_limit_in_one_tile(name, N, R):
    for ch in (0, N - 2):
        fl = oracle(name, N, R, ch)["floors"]
        both = [t for t in _tiles(fl, R) if t.min() <= SC.BIAS and t.max() >= SC.BIAS + 1]
        assert len(both) > 0
        # and in one lane: a packable and an unpackable floor in the same pixel
        assert ((fl <= SC.BIAS).any(axis=1) & (fl > SC.BIAS).any(axis=1)).any()


@pytest.mark.parametrize("name,N,R", _members("high_floor", "one_dot_high"))
def test_high_floors(name, N, R):
    for ch in (0, N - 2):
        fl = oracle(name, N, R, ch)["floors"]
        if name == "high_floor":
            assert fl.min() > SC.BIAS
        elif ch == 0:                                            # the high dot is the last one: unswept, the others small
            assert (fl[:, N - 1] > SC.BIAS).all() and fl[:, :N - 1].max() < 8


@pytest.mark.parametrize("name,N,R", _members("depleted"))
def test_depleted_dots_beside_occupied_ones(name, N, R):
    par, st = SC.make(name, N, R)
    met = 0
    for ch in _channels(N):
        fl = oracle(name, N, R, ch)["floors"]
        vd, ncont = SC.v_dash(N, par, st, ch, R)
        assert np.array_equal(np.floor(ncont).astype(np.int32), fl)
        empty = (ncont == 0) & (fl == 0) & (vd <= 0)
        beside = empty[:, :-1] & (fl[:, 1:] >= 1) | empty[:, 1:] & (fl[:, :-1] >= 1)
        met += int(beside.any(axis=1).sum())
        assert len(np.unique(fl)) > 1                            # mixed floors, not all 0
    assert met > 0
    hf = H.host_front(N, par, st, 0, R)
    assert (hf["vd"][:, 1] < 0).any() and (hf["vd"][:, 2] == 0).all() and not np.signbit(hf["vd"][:, 2]).any()
    assert (hf["vd"][:, 3] == 0).all() and np.signbit(hf["vd"][:, 3]).all()          # v' = -0.0


@pytest.mark.parametrize("name,N,R", _members("wide_window"))
def test_wide_window_spans_too_many_electrons_in_part_of_the_image(name, N, R):
    """the tile kernel needs a candidate that is valid in every pixel of a tile: floors of a dot that differ by more than 3"""
    for ch in (0, N - 2):
        span = [int((t.max(axis=0) - t.min(axis=0)).max()) for t in _tiles(oracle(name, N, R, ch)["floors"], R)]
        if N < 6:
            assert min(span) <= 3 < max(span), span
        else:                                                    # a quarter electron per pixel: wide, but every tile has a common box
            assert 2 <= max(span) <= 3, span


@pytest.mark.parametrize("name,N,R", _members("soft_mode"))
def test_soft_mode_is_soft(name, N, R):
    par, _ = SC.make(name, N, R)
    L = layout(N); G = N + 1
    w = np.linalg.eigvalsh(par[L.cdd_inv:L.cdd_inv + G * G].reshape(G, G)[:N, :N])
    assert 0 < w[0] < 0.02 * w[1]


def test_tile_program_under_the_sanitizers():
    """tests/hosttest_tile/qd_tile_asan: a program of its own (nothing is loaded into Python), built with
    -fsanitize=address,undefined; its floor loop draws tiles on both sides of 0x7FFF"""
    hdir = os.path.join(H.ROOT, "tests", "hosttest_tile")
    subprocess.check_call(["make", "-s", "-C", hdir, "qd_tile_asan"])
    r = subprocess.run([os.path.join(hdir, "qd_tile_asan")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "qd_tile_asan: ok" in r.stdout
