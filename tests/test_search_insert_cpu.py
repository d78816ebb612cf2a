"""Both forms of the kept-set insert of the exact per-pixel search (csrc/qd_pixel.h, QdSearch<N, KC, PACKED>), compiled for
the CPU (tests/hosttest_insert), one against the other.  No GPU needed.

  * streams of (E, idx) through qd_search_insert, KC = 8, 16, 32: after EVERY insert the count, each slot's energy and id, the
    group maxima and their slots, maxE / maxI / maxS / maxG and lim are equal bit for bit; the final kept set is also the KC
    smallest by (E, idx) of the valid entries of the stream;
  * whole searches qd_candidates<N, KC> in both forms, unsorted and sorted, N = 2, 3, 4, 6, 8, on device blocks of the
    product's sampler: buffers slot by slot, counts, floors and the search statistics;
  * the selection of the tile search (csrc/qd_tile.h, qd_tile_select) with its group rescan in both forms (QD_TILE_RESCAN8),
    through the entry points of tests/hosttest_tile;
  * the stand-alone program under -fsanitize=address,undefined.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers as H

HDIR = os.path.join(H.ROOT, "tests", "hosttest_insert")
D = ctypes.c_double
I = ctypes.c_int
U32 = ctypes.c_uint32
_LIBS = {}


def lib(name):
    if name not in _LIBS:
        subprocess.check_call(["make", "-s", "-C", HDIR, name])
        _LIBS[name] = ctypes.CDLL(os.path.join(HDIR, name))
    return _LIBS[name]


def insert_lib():
    return lib("libqdsim_hosttest_insert.so")


# ---------------------------------------------------------------------------------------------------------------------
# streams
# ---------------------------------------------------------------------------------------------------------------------
def run_stream(KC, packed, E, idx):
    L = insert_lib(); W = L.qdhi_row_words(); n = len(E)
    E = np.ascontiguousarray(E, np.float64); idx = np.ascontiguousarray(idx, np.uint32)
    rows = np.full((max(n, 1), W), 7 + packed, np.uint64)
    assert L.qdhi_stream(KC, packed, ctypes.c_long(n), H._p(E, D), H._p(idx, U32), H._p(rows, ctypes.c_uint64)) == 0
    return rows[:n]


def make_stream(kind, KC, rng):
    n = int(rng.integers(0, KC)) if kind == "short" else int(rng.integers(3 * KC, 12 * KC))
    idx = rng.permutation(65536)[:n].astype(np.uint32)                      # distinct ids, as the leaves of one tree have
    if kind in ("random", "short"):
        E = rng.normal(0, 1, n)
    elif kind == "ties":                                                    # 4 values: ties at the maximum and inside a group
        E = rng.integers(0, 4, n).astype(float)
    elif kind == "ties_then_lower":                                         # a full buffer of ONE value, then its eviction
        E = np.concatenate([np.full(min(n, KC + 5), 2.0), rng.integers(0, 3, max(n - KC - 5, 0)).astype(float)])
    elif kind == "descending":
        E = np.arange(n, 0, -1).astype(float)
    elif kind == "ascending":
        E = np.arange(n).astype(float)
    elif kind == "nonfinite":
        E = rng.normal(0, 1, n)
        bad = rng.random(n) < 0.25
        E[bad] = rng.choice([np.inf, np.nan, -np.inf], bad.sum())
    else:
        raise AssertionError(kind)
    return E, idx


STREAMS = ["random", "ties", "ties_then_lower", "descending", "ascending", "nonfinite", "short"]


@pytest.mark.parametrize("KC", [8, 16, 32])
@pytest.mark.parametrize("kind", STREAMS)
def test_insert_forms_bit_equal_after_every_insert(KC, kind):
    rng = np.random.default_rng(1000 * KC + STREAMS.index(kind))
    replaced = 0
    for rep in range(40):
        E, idx = make_stream(kind, KC, rng)
        a = run_stream(KC, 0, E, idx); b = run_stream(KC, 1, E, idx)
        assert a.shape == b.shape
        if len(E) == 0:
            continue
        assert a[0, 0] != np.uint64(2 ** 64 - 1) and b[0, 0] != np.uint64(2 ** 64 - 1)   # no write outside the lane's slots
        diff = np.argwhere(a != b)
        assert diff.size == 0, (rep, diff[:4])
        # the kept set at the end: the KC smallest by (E, idx) among the entries below +inf
        ok = E < np.inf
        want = sorted(zip(E[ok].tolist(), idx[ok].tolist()))[:KC]
        cnt = int(b[-1, 0])
        assert cnt == len(want)
        got = sorted(zip(b[-1, 1:1 + cnt].view(np.float64).tolist(), b[-1, 33:33 + cnt].tolist()))
        assert got == want
        if cnt == KC:                                                       # the overall maximum and its slot
            assert (b[-1, 77:78].view(np.float64)[0], int(b[-1, 78])) == want[-1]
            ms = int(b[-1, 79])
            assert (b[-1, 1 + ms:2 + ms].view(np.float64)[0], int(b[-1, 33 + ms])) == want[-1]
            assert int(b[-1, 80]) == ms // 8
        full = b[:, 0] == KC
        replaced += int((np.diff(b[full][:, 1:65], axis=0) != 0).any(axis=1).sum())
    if kind in ("random", "ties", "ties_then_lower", "descending", "nonfinite"):
        assert replaced > 0                                                 # the replacing path ran
    if kind in ("ascending", "short"):
        assert replaced == 0


# ---------------------------------------------------------------------------------------------------------------------
# whole searches
# ---------------------------------------------------------------------------------------------------------------------
def run_front(N, KC, packed, par, st, ch, R, sort):
    P = R * R
    par = np.ascontiguousarray(par); st = np.ascontiguousarray(st)
    e = np.zeros((P, KC)); ids = np.zeros((P, KC), np.uint16); nv = np.zeros(P, np.int32); fl = np.zeros((P, N), np.int32)
    stats = np.zeros(4, np.uint64)
    rc = insert_lib().qdhi_front(N, KC, packed, H._p(par, D), H._p(st, D), ch, R, sort, H._p(e, D), H._p(ids, ctypes.c_uint16),
                                 H._p(nv, ctypes.c_int32), H._p(fl, ctypes.c_int32), H._p(stats, ctypes.c_uint64))
    assert rc == 0
    return e, ids, nv, fl, stats


@pytest.mark.parametrize("N,R,mode", [(2, 12, "near"), (3, 10, "mid"), (4, 10, "far"), (6, 6, "near"), (8, 4, "near"), (8, 3, "far")])
@pytest.mark.parametrize("KC", [8, 16, 32])
def test_candidates_forms_equal_slot_by_slot(N, R, mode, KC):
    eb = H.sample_blocks(N, [4000 + N, 4100 + N])                           # the blocks of test_pixel_code_cpu
    rng = np.random.default_rng(N * 31 + len(mode))
    for k in range(2):
        par = eb.params[k]; st = H.place(N, eb.state[k], mode, rng)
        for ch in sorted({0, N - 2}):
            for sort in (0, 1):
                a = run_front(N, KC, 0, par, st, ch, R, sort)
                b = run_front(N, KC, 1, par, st, ch, R, sort)
                assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64))
                for x, y in zip(a[1:], b[1:]):
                    assert np.array_equal(x, y)
                assert a[4][2] > 0                                           # inserts happened
                if 4 ** N < KC:
                    assert (a[2] < KC).all()                                # the padded path: fewer candidates than slots
            if KC == 32:                                                    # the sorted list is the one the oracle-checked harness gives
                hf = H.host_front(N, par, st, ch, R)
                e, ids, nv, fl, _ = run_front(N, KC, 1, par, st, ch, R, 1)
                assert np.array_equal(nv, hf["nvalid"]) and np.array_equal(fl, hf["floors"])
                dig = (ids[:, :, None].astype(np.int64) >> (2 * (N - 1 - np.arange(N)))) & 3
                states = np.where(np.arange(KC)[None, :, None] < nv[:, None, None], fl[:, None, :] + dig - 1, 0)
                assert np.array_equal(states, hf["states"])


# ---------------------------------------------------------------------------------------------------------------------
# selection of the tile search: the group rescan in both forms
# ---------------------------------------------------------------------------------------------------------------------
SCAP = 383


def run_select(L, KC, fill, nS, nSfront, scode, sD, sa, sb, xs, ys, blo, bhi, amb):
    e = np.zeros(32); ids = np.zeros(32, np.uint16); maxE = D(0); eout = D(0); ms = np.zeros(3, np.int32); redo = I(0)
    rc = L.qdht_select(KC, fill, nS, nSfront, SCAP, H._p(scode, U32), H._p(sD, D), H._p(sa, D), H._p(sb, D), D(xs), D(ys),
                       U32(blo), U32(bhi), D(amb), H._p(e, D), H._p(ids, ctypes.c_uint16), ctypes.byref(maxE), H._p(ms, I),
                       ctypes.byref(eout), ctypes.byref(redo))
    assert rc == 0
    return e[:KC].tobytes(), ids[:KC].tobytes(), maxE.value, tuple(ms), eout.value, redo.value


@pytest.mark.parametrize("KC", [8, 16, 32])
@pytest.mark.parametrize("energies", ["random", "ties"])
def test_tile_select_rescan_forms_equal(KC, energies):
    L0 = lib("libqdsim_hosttest_tile_rescan0.so"); L1 = lib("libqdsim_hosttest_tile_rescan1.so")
    rng = np.random.default_rng(50 + KC + (0 if energies == "random" else 1))
    blo, bhi = 0x00000000, 0x33333333
    evicting = 0
    for rep in range(300):
        nSfront = KC + int(rng.integers(0, 3 * KC)) if rep % 5 else int(rng.integers(0, KC))
        nback = int(rng.integers(0, SCAP - nSfront)) if rep % 3 else 0
        nS = nSfront + nback
        digits = rng.integers(0, 4, (SCAP, 8))
        back = np.ones(SCAP, bool); back[:nSfront] = False
        spoil = back & (rng.random(SCAP) < 0.4)
        digits[spoil, rng.integers(0, 8, spoil.sum())] = rng.integers(4, 8, spoil.sum())
        scode = np.ascontiguousarray((digits << (4 * np.arange(7, -1, -1))).sum(axis=1).astype(np.uint32))
        if energies == "random":
            sD, sa, sb = rng.normal(0, 1, SCAP), rng.normal(0, 0.1, SCAP), rng.normal(0, 0.1, SCAP); amb = 1e-3
        else:
            sD, sa, sb = (rng.integers(0, 5, SCAP).astype(float), rng.integers(-1, 2, SCAP).astype(float),
                          rng.integers(-1, 2, SCAP).astype(float)); amb = 0.5
        xs, ys = float(rng.integers(-3, 5)), float(rng.integers(-3, 5))
        for fill in (0, 1):
            a = run_select(L0, KC, fill, nS, nSfront, scode, sD, sa, sb, xs, ys, blo, bhi, amb)
            b = run_select(L1, KC, fill, nS, nSfront, scode, sD, sa, sb, xs, ys, blo, bhi, amb)
            assert a == b, (rep, fill, a[2:], b[2:])
        evicting += int(a[4] < np.inf)
    assert evicting > 100                                                   # the replacing step, where the rescan is, ran


def test_insert_program_under_the_sanitizers():
    """tests/hosttest_insert/qd_insert_asan: a program of its own (nothing is loaded into Python), built with
    -fsanitize=address,undefined"""
    subprocess.check_call(["make", "-s", "-C", HDIR, "qd_insert_asan"])
    r = subprocess.run([os.path.join(HDIR, "qd_insert_asan")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "qd_insert_asan: ok" in r.stdout
