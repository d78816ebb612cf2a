"""The candidate search on designed devices (tests/search_cases.py): exact energy ties at the boundary of the kept set and
inside it, floors on both sides of the packed min / max reduction (0x7FFF), depleted dots, and tiles that leave the fast
path for each reason the kernel counts.  References: the plain-C 4^N scan (oracle/qd_oracle.c) for the kept states, the
oracle's dense eigh for the ground energy; nothing is recorded from the library under test.

Every handle holds two envs: the designed block in env 0 and an ordinary sampled one in env 1, whose candidates must not
depend on its neighbour.  The search counters of a handle never reset, so the designed env is first rendered alone (an env-id
list of one) and the counters' increase over that launch is what the coverage assertions read."""
import ctypes

import numpy as np
import pytest

import qd_oracle_c as OC
import helpers as H
import search_cases as SC
from test_gpu_tile_search import RESID_ANY

pytestmark = pytest.mark.gpu

REASONS = ("ranges", "seeds", "frontier", "leaves", "superset")
OWN = {}                                  # (name, N, R, K) -> search counters of the designed env's own launch


def _load(env, pars, sts):
    from qadapt_hip import _lib
    ids = np.arange(len(pars), dtype=np.int32)
    P = np.ascontiguousarray(np.stack(pars)); S = np.ascontiguousarray(np.stack(sts))
    _lib.check(env._h, env._lib.qd_load_episodes(env._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(ids),
                                                 P.ctypes.data, S.ctypes.data, 0, env._stream()), "qd_load_episodes")
    env._params_host[ids] = P


def _stats_delta(a, b):
    d = {k: b[k] - a[k] for k in ("tiles", "tiles_redone", "pixels_redone")}
    d["tiles_redone_by_reason"] = {k: b["tiles_redone_by_reason"][k] - a["tiles_redone_by_reason"][k] for k in REASONS}
    return d


def _handle(N, R, K, par, st, validate=True, pixel_search=False):
    """B = 2 handle with (par, st) in env 0 and the sampled neighbour in env 1, observed.  Returns (env, the search counters
    of env 0's own launch: None without validate)."""
    import torch
    from qadapt_hip.vec_env import VecQuantumDeviceEnv, SyntheticCapacitanceModel
    env = VecQuantumDeviceEnv(2, num_dots=N, resolution=R, seed=77, validate=validate, pixel_search=pixel_search,
                              num_charge_states=K, capacitance_model=SyntheticCapacitanceModel(7))
    spar, sst = SC.sampled(N)
    _load(env, [par, spar[1]], [st, sst[1]])
    own = None
    if validate:
        s0 = env.search_stats()
        env.observe(torch.zeros(1, dtype=torch.int32, device=env.device), 1)
        own = _stats_delta(s0, env.search_stats())
    env.observe()
    return env, own


_ALONE = {}


def _neighbour_alone(N, R, K):
    """candidates of the sampled env 1 beside an ordinary sampled env 0 (computed once per shape)"""
    if (N, R, K) not in _ALONE:
        spar, sst = SC.sampled(N)
        env, _ = _handle(N, R, K, spar[0], sst[0])
        c = env.candidates()[1]
        c.setflags(write=False)
        _ALONE[(N, R, K)] = c
        env.close()
    return _ALONE[(N, R, K)]


_ORACLE = {}


def _oracle(name, N, R, ch, tc_base=None):
    """the C oracle's channel of a family member (computed once, shared, read-only); tc_base does not enter the states"""
    key = (name, N, R, ch, tc_base)
    if key not in _ORACLE:
        par, st = SC.make(name, N, R, tc_base=tc_base)
        dev = H.dev_view(N, par); sv = H.state_view(N, st)
        ref = OC.csd_channel(dev, sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, sv.barrier_v, dev.window, ch, R)
        for v in ref.values():
            v.setflags(write=False)
        _ORACLE[key] = ref
    return _ORACLE[key]


def _channels(N):
    """every channel up to 6 dots; channel 0 and N-2 beyond (the 4^8 scan takes a second per channel)"""
    return list(range(N - 1)) if N <= 6 else [0, N - 2]


CASES = [(name, N, R, K) for name, N, R in SC.MEMBERS for K in (SC.KS if name in SC.TIE_FAMILIES else (32,))]


@pytest.mark.parametrize("name,N,R,K", CASES)
def test_designed_device_against_brute_force(name, N, R, K):
    par, st = SC.make(name, N, R)
    tile, own = _handle(N, R, K, par, st)
    pix, _ = _handle(N, R, K, par, st, pixel_search=True)
    ct = tile.candidates(); cp = pix.candidates()
    print(f"[designed] {name} N={N} R={R} K={K}: {own}")
    OWN[(name, N, R, K)] = own
    dev = H.dev_view(N, par); sv = H.state_view(N, st)
    et = tile.eigen()
    for ch in _channels(N):
        ref = _oracle(name, N, R, ch)
        bad = (ct[0, ch, :, :K] != ref["states"][:, :K]).any(axis=(1, 2))
        assert not bad.any(), (ch, int(bad.sum()), np.nonzero(bad)[0][:8])
        bad = (cp[0, ch, :, :K] != ref["states"][:, :K]).any(axis=(1, 2))
        assert not bad.any(), ("pixel_search", ch, int(bad.sum()))
        # ground energy against the oracle's dense eigh of the K kept states, every pixel
        sp = H.pixel_spectrum(dev, sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, sv.barrier_v, dev.window, ch, R,
                              states=ref["states"][:, :K])
        err = np.abs(et[0, ch, :, 0] - sp["lam0"]) / sp["hnorm"]
        assert np.all(err <= 1e-12), (ch, float(err.max()))
    assert np.array_equal(ct, cp)                                  # every channel, both envs, the padding slots
    assert (ct[0, :, :, K:] == -1).all()
    assert np.array_equal(tile.raw()[0].view(np.uint64), pix.raw()[0].view(np.uint64))
    assert np.array_equal(et.view(np.uint64), pix.eigen().view(np.uint64))
    assert et[..., 1].max() <= RESID_ANY, float(et[..., 1].max())
    # the sampled neighbour does not see the designed block
    assert np.array_equal(ct[1], _neighbour_alone(N, R, K))
    # coverage: the tile kernel ran on the designed env and both of its exits were taken
    tiles = (N - 1) * ((R + 7) // 8) ** 2
    assert own["tiles"] == tiles, own
    if name in SC.TIE_FAMILIES:
        assert own["pixels_redone"] > 0 and own["tiles_redone"] < own["tiles"], own
    if name in ("high_floor", "one_dot_high"):
        assert own["tiles_redone"] < own["tiles"], own            # the plain reductions led into a completed tile search
    if name == "wide_window" and N < 6:                            # floors that differ by more than 3 in part of the image
        assert 0 < own["tiles_redone_by_reason"]["ranges"] < own["tiles"], own
    tile.close(); pix.close()


@pytest.mark.parametrize("name,N,R", [("dyadic", 4, 33), ("exchange", 4, 33), ("dyadic_mixed", 8, 32)])
@pytest.mark.parametrize("K", SC.KS)
def test_classical_limit_with_ties(name, N, R, K):
    """tc_base = 0: the Hamiltonian is diagonal, every state is its own component and the ground state is the first state of
    the brute-force order -- among states of exactly the same energy the one with the lowest candidate index.  A product-mode
    handle keeps its records unsorted, so there the winner must come from the index and not from the slot."""
    par, st = SC.make(name, N, R, tc_base=0.0)
    val, own = _handle(N, R, K, par, st)
    print(f"[classical] {name} N={N} R={R} K={K}: {own}")
    assert 0 < own["pixels_redone"] < (N - 1) * R * R, own          # records of the tile kernel and of the redo pass
    occ = val.occupations(); cand = val.candidates()
    first_tied = 0
    for ch in _channels(N):
        ref = _oracle(name, N, R, ch, tc_base=0.0)
        assert np.array_equal(cand[0, ch, :, :K], ref["states"][:, :K]), ch
        assert np.array_equal(occ[0, ch], ref["states"][:, 0].astype(np.float64)), \
            (ch, int((occ[0, ch] != ref["states"][:, 0]).any(axis=1).sum()))
        if N <= 5:
            E, order = SC.brute_force(N, par, st, ch, R, ref["floors"])
            assert np.array_equal(SC.states_of(ref["floors"], order, 1)[:, 0], ref["states"][:, 0])
            first_tied += int((E[:, 0] == E[:, 1]).sum())
    if N <= 5:
        assert first_tied > 0                                      # the rule was needed: two lowest energies equal in some pixels
    prod, _ = _handle(N, R, K, par, st, validate=False)
    assert np.array_equal(prod.raw()[0][0].view(np.uint64), val.raw()[0][0].view(np.uint64))
    val.close(); prod.close()


def test_every_reachable_hand_over_reason_was_met():
    """Over the designed envs each of `ranges`, `frontier` and `superset` sent at least one tile to the per-pixel search (the
    counters of the tests above; a member that has not run in this process is rendered here).  `seeds` and `leaves` cannot
    occur on finite inputs and stay 0."""
    seen = {k: 0 for k in REASONS}
    for name, N, R in SC.MEMBERS:
        if (name, N, R, 32) not in OWN:
            env, OWN[(name, N, R, 32)] = _handle(N, R, 32, *SC.make(name, N, R))
            env.close()
        for k in REASONS:
            seen[k] += OWN[(name, N, R, 32)]["tiles_redone_by_reason"][k]
    print(f"[designed] hand-over reasons over the members, K = 32: {seen}")
    for k in ("ranges", "frontier", "superset"):
        assert seen[k] > 0, seen
    assert seen["seeds"] == 0 and seen["leaves"] == 0, seen
