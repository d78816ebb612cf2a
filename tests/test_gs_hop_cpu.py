"""The pair predicate of the ground-state structure kernel (csrc/qd_groundstate.h: qd_gs_hop), compiled for the CPU
(tests/hosttest_gs), against a digit-by-digit definition written in numpy: two states couple iff exactly two ADJACENT
digits differ, one by +1 and the other by -1, that pair's coupling bit is set, and every other digit is equal.  Also the
kernel's bookkeeping of the 16 exchange rounds (verdicts collected in the lane's rotated frame, rotated into place once),
emulated on the host with the compiled predicate.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers as H

_LIB = None


def gs_lib():
    global _LIB
    if _LIB is None:
        hdir = os.path.join(H.ROOT, "tests", "hosttest_gs")
        subprocess.check_call(["make", "-s", "-C", hdir, "libqdsim_hosttest_gs.so"])
        _LIB = ctypes.CDLL(os.path.join(hdir, "libqdsim_hosttest_gs.so"))
        _LIB.qdhg_hop.restype = None
    return _LIB


def hop(ci, cj, tcq):
    """qd_gs_hop of the arrays, element by element"""
    ci, cj, tcq = np.broadcast_arrays(np.asarray(ci, np.uint32), np.asarray(cj, np.uint32), np.asarray(tcq, np.uint32))
    ci, cj, tcq = (np.ascontiguousarray(a).ravel() for a in (ci, cj, tcq))
    out = np.empty(ci.size, np.uint32)
    gs_lib().qdhg_hop(ctypes.c_long(ci.size), H._p(ci, ctypes.c_uint32), H._p(cj, ctypes.c_uint32), H._p(tcq, ctypes.c_uint32),
                      H._p(out, ctypes.c_uint32))
    return out


def hop_by_digits(ci, cj, tcq, n):
    """the definition, digit by digit: codes of n nibbles, tcq with bit 4q set iff the pair of nibbles (q + 1, q) couples"""
    ci = np.asarray(ci, np.int64); cj = np.asarray(cj, np.int64); tcq = np.asarray(tcq, np.int64)
    d = np.stack([((cj >> (4 * k)) & 15) - ((ci >> (4 * k)) & 15) for k in range(n)], axis=-1)      # (..., n)
    out = np.zeros(np.broadcast(ci, cj, tcq).shape, bool)
    for q in range(n - 1):
        others = np.ones(d.shape[:-1], bool)
        for k in range(n):
            if k not in (q, q + 1):
                others &= d[..., k] == 0
        moved = ((d[..., q + 1] == 1) & (d[..., q] == -1)) | ((d[..., q + 1] == -1) & (d[..., q] == 1))
        out |= moved & others & (((tcq >> (4 * q)) & 1) == 1)
    return out.astype(np.uint32)


def codes_of(n):
    """every code of n nibbles with digits 0..3"""
    c = np.zeros(1, np.uint32)
    for k in range(n):
        c = (c[:, None] | (np.arange(4, dtype=np.uint32) << np.uint32(4 * k))[None, :]).ravel()
    return c


def masks_of(n):
    """every coupling mask of n nibbles: any subset of the bits 4q, q < n - 1"""
    return np.array([sum(((s >> q) & 1) << (4 * q) for q in range(n - 1)) for s in range(1 << (n - 1))], np.uint32)


@pytest.mark.parametrize("n", [2, 3, 4])
def test_every_pair_and_every_mask_up_to_four_nibbles(n):
    c = codes_of(n)
    ci, cj = np.meshgrid(c, c, indexing="ij")
    hops = 0
    for tcq in masks_of(n):
        got = hop(ci, cj, tcq); want = hop_by_digits(ci, cj, tcq, n).ravel()
        assert np.array_equal(got, want), (n, hex(int(tcq)))
        hops += int(want.sum())
    assert hops > 0


def test_every_pair_of_five_nibbles():
    """all 4^5 x 4^5 pairs with every pair coupled, then each with a random mask"""
    c = codes_of(5)
    ci, cj = np.meshgrid(c, c, indexing="ij")
    full = masks_of(5)[-1]
    want = hop_by_digits(ci, cj, full, 5)
    assert np.array_equal(hop(ci, cj, full), want.ravel())
    assert int(want.sum()) == 2 * 4 * 9 * 4 ** 3            # per pair: 3 x 3 moves each way, the other three digits free
    tcq = np.random.default_rng(5).choice(masks_of(5), size=ci.shape)
    assert np.array_equal(hop(ci, cj, tcq), hop_by_digits(ci, cj, tcq, 5).ravel())


def _random_codes(rng, size, n=8):
    dig = rng.integers(0, 4, (size, n)).astype(np.uint32)
    return dig, (dig << (4 * np.arange(n, dtype=np.uint32))[None, :]).sum(axis=1).astype(np.uint32)


def test_random_pairs_of_eight_nibbles():
    """10^6 independent random pairs (almost never neighbours), and 10^6 pairs one or two digit steps apart (neighbours, and
    the near misses: one digit changed, two digits changed the same way, two non-adjacent digits, a step of 2)"""
    rng = np.random.default_rng(20240)
    n, size = 8, 10 ** 6
    masks = masks_of(n)
    _, ci = _random_codes(rng, size); _, cj = _random_codes(rng, size)
    tcq = rng.choice(masks, size)
    assert np.array_equal(hop(ci, cj, tcq), hop_by_digits(ci, cj, tcq, n))
    dig, ci = _random_codes(rng, size)
    dj = dig.astype(np.int64)
    rows = np.arange(size)
    for _ in range(2):
        k = rng.integers(0, n, size); step = rng.choice([-2, -1, -1, -1, 0, 1, 1, 1, 2], size)
        dj[rows, k] = np.clip(dj[rows, k] + step, 0, 3)
    adjacent = rng.random(size) < 0.5                      # half of them: a proper move between neighbouring digits where it fits
    q = rng.integers(0, n - 1, size); sgn = rng.choice([-1, 1], size)
    dk = dig.astype(np.int64)
    dk[rows, q] += sgn; dk[rows, q + 1] -= sgn
    fits = adjacent & (dk.min(axis=1) >= 0) & (dk.max(axis=1) <= 3)
    dj[fits] = dk[fits]
    cj = (dj << (4 * np.arange(n))[None, :]).sum(axis=1).astype(np.uint32)
    tcq = rng.choice(masks, size)
    want = hop_by_digits(ci, cj, tcq, n)
    assert np.array_equal(hop(ci, cj, tcq), want)
    assert 0.1 * size < int(want.sum()) < 0.5 * size       # both verdicts are well represented


def test_equal_codes_do_not_hop():
    """the same state, and the copies of the |0..0> padding"""
    _, c = _random_codes(np.random.default_rng(1), 1000)
    assert not hop(c, c, 0x01111111).any()
    assert not hop(0, 0, 0x01111111).any() and not hop(0, 0, 0).any()
    assert not hop(0x33333333, 0x33333333, 0x01111111).any()


def _hop_cluster(rng, n=8, count=32):
    """`count` distinct codes grown by random hops from a random state: a pixel's kept states look like this"""
    dig, _ = _random_codes(rng, 1, n)
    first = tuple(int(x) for x in dig[0])
    seen = {first}
    order = [first]
    while len(order) < count:
        d = list(order[rng.integers(len(order))])
        q = int(rng.integers(0, n - 1)); s = int(rng.choice([-1, 1]))
        d[q] += s; d[q + 1] -= s
        if rng.random() < 0.15:                            # now and then a state that is no neighbour of its parent
            d[int(rng.integers(n))] += int(rng.choice([-1, 1]))
        if min(d) < 0 or max(d) > 3 or tuple(d) in seen:
            continue
        seen.add(tuple(d)); order.append(tuple(d))
    dig = np.array(order, np.uint32)[rng.permutation(count)]
    return (dig << (4 * np.arange(n, dtype=np.uint32))[None, :]).sum(axis=1).astype(np.uint32)


@pytest.mark.parametrize("seed", range(6))
def test_sixteen_rounds_in_the_rotated_frame_give_the_adjacency_matrix(seed):
    """What a half-wave does: in round j lane m tests lane (m + j) mod 32 and receives the verdict of lane (m - j) mod 32
    (round 16: the forward test only); forward verdicts go to bit j, handed-back ones to bit 32 - j, and the word is
    rotated left by m at the end.  Bit p of lane m's mask must be the pair test of (m, p)."""
    rng = np.random.default_rng(77 + seed)
    code = _hop_cluster(rng)
    tcq = masks_of(8)[-1] if seed % 2 == 0 else rng.choice(masks_of(8))
    m = np.arange(32)
    acc = np.zeros(32, np.uint64)
    for j in range(1, 17):
        verdict = hop(code, code[(m + j) % 32], tcq).astype(np.uint64)
        acc |= verdict << np.uint64(j)
        if j < 16:
            acc |= verdict[(m - j) % 32] << np.uint64(32 - j)
    assert int(acc.max()) < 1 << 32 and not (acc & np.uint64(1)).any()
    nbr = ((acc << m.astype(np.uint64)) | (acc >> (32 - m).astype(np.uint64))) & np.uint64(0xFFFFFFFF)
    mask = ((nbr[:, None] >> m[None, :].astype(np.uint64)) & np.uint64(1)).astype(np.uint32)        # [m, p]
    want = hop_by_digits(code[:, None], code[None, :], tcq, 8)
    assert np.array_equal(mask, want)
    assert np.array_equal(mask, mask.T) and not mask.diagonal().any()
    if seed % 2 == 0:
        assert int(want.sum()) >= 31                        # (every pair couples: the cluster was grown along hops)
