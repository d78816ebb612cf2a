"""The conditions of the mixed latched scenes (tests/mixed_cases.py), from the oracle alone: no GPU.  The GPU tier
(tests/test_gpu_mixed_latched.py) first asserts that the handles' states ARE the trajectory rebuilt here, so what these tests
establish about the scene holds for the GPU run: the share of pixels its physics check may exempt, that latching is visible
in every bucket at every compared step (2 dots included) and in a freshly reset env, that both acceptance branches occur,
and that the all-stages variant shows a radial-replaced channel and one inside the ramp."""
import numpy as np
import pytest

import helpers as H
import mixed_cases as MC
import qd_oracle as O
from qadapt_hip import shard

BUCKETS = sorted(MC.COUNTS)


def test_scene_shape():
    assert MC.COUNTS == {2: 5, 4: 5, 6: 5, 8: 5} and MC.R == 20 and MC.ENV_CHUNK == 2 and MC.T == 4
    assert MC.R % 8 != 0 and MC.R * MC.R == 400                       # the image edge cuts the 8 x 8 tiles
    assert [MC.bucket_first(N) for N in BUCKETS] == [0, 5, 10, 15]
    assert -(-5 // MC.ENV_CHUNK) == 3                                 # an observe of 5 envs is three chunks
    assert MC.compared(2) == [0, 1, 4, 2] and MC.compared(3) == [0, 3, 2]
    # the two envs reset in step 2 land in different shards of world = 2, in every bucket: both shards take the partial path
    for N in BUCKETS:
        f0, n0 = shard.shard_mixed(MC.COUNTS, 0, 2, MC.R)[N]
        first = MC.bucket_first(N)
        assert f0 - first <= 1 < f0 - first + n0 <= 4, (N, f0, n0)


@pytest.mark.parametrize("N", BUCKETS)
def test_trajectory_resets_and_observation_numbers(N):
    tr = MC.trajectory(N)
    trunc = np.zeros((MC.T, tr.n), bool)
    trunc[2, [1, 4]] = True; trunc[3, 3] = True
    assert np.array_equal(tr.truncated, trunc)
    assert tr.steps[3].tolist() == [4, 1, 4, 0, 1]
    # one observation number per observe: reset 1, steps 0 and 1: 2 and 3, step 2: 4 and its partial reset 5, step 3: 6 and 7
    assert tr.ck_serial.tolist() == [2, 3, 5, 7]
    assert tr.serial[2].tolist() == [4, 5, 4, 4, 5] and tr.serial[3].tolist() == [6, 6, 6, 7, 6]
    L = tr.L
    for t in range(MC.T):
        for i in range(tr.n):
            if tr.truncated[t, i]:
                continue                                              # (a reset env shows its new device's start voltages)
            par, st = tr.params[t, i], tr.state[t, i]
            off_g = np.abs(st[L.s_gate_v:L.s_gate_v + N] - st[L.s_gate_gt:L.s_gate_gt + N])
            off_b = np.abs(st[L.s_barrier_v:L.s_barrier_v + N - 1] - st[L.s_barrier_gt:L.s_barrier_gt + N - 1])
            role = MC.ROLES[i]
            if role != "far":
                # the float32 action resolves the 80..100 V range to ~1e-5 V
                assert off_g.max() <= MC.SPAN[role][0] + 1e-4 and off_b.max() <= MC.SPAN[role][1] + 1e-4, (t, i)
            assert np.all(np.abs(tr.actions[t, i]) <= 1.0)
            # the voltages are the oracle's mapping of the action on the device's own range
            assert np.array_equal(st[L.s_gate_v:L.s_gate_v + N], O.rescale(tr.actions[t, i, :N], par[L.pmin:L.pmin + N], par[L.pmax:L.pmax + N]))
    # the devices of a reset env differ before and after
    assert not np.array_equal(tr.params[1, 1], tr.params[2, 1]) and np.array_equal(tr.params[1, 0], tr.params[3, 0])
    assert np.all((tr.rewards >= 0) & (tr.rewards <= 1))


@pytest.mark.parametrize("t", MC.CHECK_STEPS)
@pytest.mark.parametrize("N", BUCKETS)
def test_exempt_shares_and_visible_latching(N, t):
    """Near envs: at most 10 % of the pixels below GAP_MIN, the mid env at most 25 % (the far and the freshly reset envs are
    not capped: the per-pixel rule alone applies to them).  Some compared env shows latched pixels, in both variants."""
    seen = {v: 0 for v in MC.VARIANTS}
    for i in MC.compared(t):
        f = MC.frame(N, t, i)
        lat = {v: MC.latched_pixels(f, v) for v in MC.VARIANTS}
        share = "not capped" if f.reset else f"{MC.exempt_share(f):.4f}"
        print(f"[mixed scene] N={N} step {t} env {i} ({'reset' if f.reset else MC.ROLES[i]}): exempt share {share}; latched pixels "
              f"{lat['latch'][0]} (1-dot {lat['latch'][1]}, 2-dot {lat['latch'][2]}), all stages {lat['all'][0]}; "
              f"radial {[c['radial'] for c in f.channels]}")
        if not f.reset:
            assert MC.exempt_share(f) <= (MC.NEAR_EXEMPT_MAX if MC.ROLES[i] == "near" else MC.MID_EXEMPT_MAX), (N, t, i, f.exempt)
        for v in MC.VARIANTS:
            seen[v] += lat[v][0]
    assert all(seen.values()), (N, t, seen)


def test_both_branches_a_latched_reset_env_and_the_radial_regimes():
    branches = np.zeros(2, int)
    reset_latched = {N: 0 for N in BUCKETS}
    reset_latched_all = 0
    radial = {"replaced": 0, "ramp": 0, "flat": 0}
    for N in BUCKETS:
        for t in MC.CHECK_STEPS:
            resets = [i for i in MC.compared(t) if MC.frame(N, t, i).reset]
            assert resets, (N, t)                                     # the serial S + 1 path is compared in every bucket and step
            for i in MC.compared(t):
                f = MC.frame(N, t, i)
                lat = MC.latched_pixels(f, "latch")
                branches += np.array(lat[1:])
                for c in f.channels:
                    radial[c["radial"]] += 1
                if f.reset:
                    reset_latched[N] += lat[0]
                    reset_latched_all += MC.latched_pixels(f, "all")[0]
    print(f"[mixed scene] rejected 1-dot / 2-dot changes {branches.tolist()}; latched pixels of freshly reset envs per bucket "
          f"{reset_latched}, with all stages {reset_latched_all}; compared channels by radial status {radial}")
    assert branches.min() > 0
    # a wrong observation number on the partial path shows only where a reset env has latched pixels
    assert min(reset_latched.values()) > 0 and reset_latched_all > 0
    assert radial["replaced"] > 0 and radial["ramp"] > 0


def test_gap_without_padding_is_never_below_the_projects():
    """mixed_cases.rel_gap against helpers.pixel_spectrum on the 2-dot near env, where half the kept list is padding."""
    import qd_oracle_c as OC
    N, t, i = 2, 2, 0
    tr = MC.trajectory(N)
    dev, sv = H.dev_view(N, tr.params[t, i]), H.state_view(N, MC.full_state_row(N, tr.state[t, i]))
    ref = OC.csd_channel(dev, sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, sv.barrier_v, dev.window, 0, MC.R)
    sp = H.pixel_spectrum(dev, sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, sv.barrier_v, dev.window, 0, MC.R, states=ref["states"])
    gap = MC.rel_gap(dev, sv, 0, ref["states"])
    assert np.all(gap >= sp["rel_gap"])
    changed = gap != sp["rel_gap"]
    # where it changed the ground state is the padded |0 0> itself: integer occupations, nothing unresolved
    assert changed.any() and np.all(ref["occ"][changed] == 0.0)
