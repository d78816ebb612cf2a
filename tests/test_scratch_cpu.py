"""The buffer owner of csrc/qd_scratch.h (QdBuf, qd_reserve_group) without a GPU: on a fake memory policy that counts,
through the tests/hosttest harness, and once more on malloc in a program built with the address and undefined-behaviour
sanitizers.  The rules under test are the ones the handle's lazily allocated and growing buffers rely on (qd_api.hip):
a buffer that failed to grow is EMPTY, and a group is completely allocated or completely empty."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers as H

OOM = 2            # the fake policy's status of a failed allocation


class Scratch:
    """Four QdBuf<double> on the counting policy; `nbuf` of them are used, which is the fake's bound on live blocks."""

    def __init__(self, nbuf):
        self.h = H.hosttest()
        self.h.qdh_scr_new.restype = ctypes.c_void_p
        self.o = ctypes.c_void_p(self.h.qdh_scr_new(nbuf))

    def reserve(self, k, n):
        return self.h.qdh_scr_reserve(self.o, k, ctypes.c_longlong(n))

    def reserve_group(self, n4):
        n = np.asarray(n4, np.int64)
        return self.h.qdh_scr_reserve_group(self.o, H._p(n, ctypes.c_longlong))

    def fail_in(self, k):
        self.h.qdh_scr_fail_in(k)

    def bufs(self):
        out = np.zeros(8, np.int64)
        self.h.qdh_scr_bufs(self.o, H._p(out, ctypes.c_longlong))
        return out[:4].tolist(), out[4:].tolist()

    def fake(self):
        out = np.zeros(5, np.int64)
        self.h.qdh_scr_fake(H._p(out, ctypes.c_longlong))
        return dict(zip(("live", "over", "allocs", "releases", "last_bytes"), out.tolist()))

    def delete(self):
        self.h.qdh_scr_delete(self.o)
        self.o = None


def test_reserve_on_empty_gives_a_block_of_at_least_n():
    s = Scratch(1)
    p, cap = s.bufs()
    assert p == [0] * 4 and cap == [0] * 4
    assert s.reserve(0, 100) == 0
    p, cap = s.bufs()
    f = s.fake()
    assert p[0] != 0 and cap[0] >= 100 and f["last_bytes"] >= 100 * 8
    assert f["live"] == 1 and f["allocs"] == 1 and f["releases"] == 0
    s.delete()
    assert s.fake()["live"] == 0


def test_reserve_within_capacity_makes_no_policy_call_and_keeps_the_pointer():
    s = Scratch(1)
    assert s.reserve(0, 100) == 0
    p0, cap0 = s.bufs()
    for n in (100, 99, 1, 0):
        assert s.reserve(0, n) == 0
    f = s.fake()
    assert s.bufs() == (p0, cap0) and f["allocs"] == 1 and f["releases"] == 0
    s.delete()


def test_growth_frees_before_it_allocates():
    s = Scratch(1)
    for n in (10, 100, 1000, 1001):
        assert s.reserve(0, n) == 0
        p, cap = s.bufs()
        f = s.fake()
        assert p[0] != 0 and cap[0] >= n and f["last_bytes"] >= n * 8
        assert f["live"] == 1 and f["over"] == 0          # checked inside the fake's alloc(): never a second live block
    f = s.fake()
    assert f["allocs"] == 4 and f["releases"] == 3
    s.delete()
    assert s.fake()["live"] == 0


def test_failed_growth_leaves_the_buffer_empty_and_a_smaller_reserve_succeeds():
    s = Scratch(1)
    assert s.reserve(0, 100) == 0
    s.fail_in(1)
    assert s.reserve(0, 1000) == OOM
    p, cap = s.bufs()
    f = s.fake()
    assert p[0] == 0 and cap[0] == 0 and f["live"] == 0
    assert s.reserve(0, 50) == 0
    p, cap = s.bufs()
    f = s.fake()
    assert p[0] != 0 and cap[0] >= 50 and f["live"] == 1 and f["over"] == 0
    s.delete()
    assert s.fake()["live"] == 0


@pytest.mark.parametrize("allocated_before", [False, True])
@pytest.mark.parametrize("fail_at", [1, 2, 3, 4])
def test_group_of_four_is_all_or_nothing(fail_at, allocated_before):
    """The probe / point scratch (four device buffers behind one first-use reserve) and the staging ring (slots that grow
    together): whichever member's allocation fails, nobody is left holding a block -- neither a new one nor one of the
    old capacity -- and the next call starts over and brings all four to capacity."""
    small, large = [10, 20, 30, 40], [100, 200, 300, 400]
    s = Scratch(4)
    if allocated_before:
        assert s.reserve_group(small) == 0
        assert s.fake()["live"] == 4
    s.fail_in(fail_at)
    assert s.reserve_group(large) == OOM
    p, cap = s.bufs()
    f = s.fake()
    assert p == [0] * 4 and cap == [0] * 4 and f["live"] == 0
    assert s.reserve_group(large) == 0
    p, cap = s.bufs()
    f = s.fake()
    assert all(p) and len(set(p)) == 4 and all(c >= n for c, n in zip(cap, large))
    assert f["live"] == 4 and f["over"] == 0
    # sized: a compare and no policy call
    calls = (f["allocs"], f["releases"])
    assert s.reserve_group(large) == 0 and s.reserve_group(small) == 0
    f = s.fake()
    assert s.bufs() == (p, cap) and (f["allocs"], f["releases"]) == calls
    s.delete()
    assert s.fake()["live"] == 0


def test_destruction_returns_live_blocks_to_zero():
    s = Scratch(4)
    assert s.reserve_group([1, 2, 3, 4]) == 0
    assert s.reserve(2, 64) == 0
    assert s.fake()["live"] == 4
    s.delete()
    f = s.fake()
    assert f["live"] == 0 and f["allocs"] == f["releases"] == 5 and f["over"] == 0


def test_same_sequences_under_the_sanitizers():
    """A program of its own (malloc-backed policy, -fsanitize=address,undefined): leaks, double frees and uses after free
    are the sanitizer's to report, as a non-zero exit status."""
    hdir = os.path.join(H.ROOT, "tests", "hosttest")
    subprocess.check_call(["make", "-s", "-C", hdir, "qd_scratch_asan"])
    r = subprocess.run([os.path.join(hdir, "qd_scratch_asan")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
