"""The ground-state stage on designed devices (tests/gs_cases.py) on the MI355X (run with -m gpu): hop components of every
size 2..32, every size class winning the selection, a batch whose pool is filled to its last double, couplings that are
exactly zero or denormal in some pairs only.  tests/gputest_eig hands the solvers their tasks directly; here the tasks come
from the structure kernel and go to the select kernel: the size word of the padded and memory classes, the packed lower
triangle and its zero fill, link / rank, the padded write-back and the winner's vector read by rank.

References: the plain-C oracle and its dense eigh, by the unchanged `_check_channel` of test_gpu_parity (32 kept states) and of
test_gpu_num_charge_states (K kept states); what the members contain is asserted on the CPU by tests/test_gs_cases_cpu.py,
whose counts bound the device's own task counters here.

Every handle holds two envs: the designed block in env 0 and an ordinary sampled one in env 1 (search_cases.sampled).  The
solver counters of a handle never reset, so the designed env is first rendered alone (an env-id list of one) and the
counters' increase over that launch is what the coverage assertions read.  A scene is rendered once per (member, K, mode,
pruning flag) and shared by the tests, read-only."""
import numpy as np
import pytest

import gs_cases as GS
import helpers as H
import points_helpers as PH
import search_cases as SC
from qadapt_hip.layout import layout
from test_gpu_search_adversarial import _load

pytestmark = pytest.mark.gpu

SAMPLED = "sampled"                       # in place of a member's name: the ordinary sampled block in env 0 as well
_RENDER = {}
WORST = {}                                # member -> measured worst figures of the parity test (what DESIGN 2 tabulates)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _env(N, R, K, validate, zero=False):
    import torch
    from qadapt_hip.vec_env import VecQuantumDeviceEnv, SyntheticCapacitanceModel
    assert torch.cuda.is_available()
    return VecQuantumDeviceEnv(2, num_dots=N, resolution=R, seed=77, validate=validate, num_charge_states=K,
                               capacitance_model=SyntheticCapacitanceModel(7), gs_gershgorin_zero=zero)


def _blocks(name, N, R):
    """the two envs' parameter and state blocks"""
    spar, sst = SC.sampled(N)
    par, st = (spar[0], sst[0]) if name == SAMPLED else GS.make(name, N, R)
    return [par, spar[1]], [st, sst[1]]


def _counters(s):
    return dict(s["tasks_by_size"], tasks=s["tasks"], wide_tasks=s["wide_tasks"])


def _render(name, N, R, K=32, validate=True, zero=False):
    """dict(raw (2, C, P)[, occ, eig, cand, own]) of the scene; own: the solver counters of env 0's own launch"""
    import torch
    key = (name, N, R, K, validate, zero)
    if key not in _RENDER:
        env = _env(N, R, K, validate, zero)
        _load(env, *_blocks(name, N, R))
        out = {}
        if validate:
            s0 = _counters(env.solver_stats())
            env.observe(torch.zeros(1, dtype=torch.int32, device=env.device), 1)
            s1 = _counters(env.solver_stats())
            out["own"] = {k: s1[k] - s0[k] for k in s0}
        env.observe()
        out["raw"] = env.raw()[0]
        if validate:
            out["occ"] = env.occupations(); out["eig"] = env.eigen(); out["cand"] = env.candidates()
        env.close()
        for k, v in out.items():
            if k != "own":
                v.setflags(write=False)
        _RENDER[key] = out
    return _RENDER[key]


def _product_rule(tag, raw, z_ref, ok):
    """product mode: the raw signal within 1e-6 relative of the oracle's wherever validate mode compares (the rule of
    test_config2_shape_in_product_mode_against_oracle); returns the worst error"""
    d = np.abs(raw - z_ref) / np.maximum(np.abs(z_ref), 1e-3)
    worst = float(d[ok].max()) if ok.any() else 0.0
    assert np.all(d[ok] <= 1e-6), (tag, worst)
    return worst


@pytest.mark.parametrize("name,N,R", GS.MEMBERS)
def test_member_against_the_oracle_in_both_modes(name, N, R):
    import test_gpu_parity as P
    par, st = GS.make(name, N, R)
    dev = H.dev_view(N, par); sv = H.state_view(N, st)
    v = _render(name, N, R)
    C = N - 1
    z_ref = np.zeros((C, R * R)); ok = np.zeros((C, R * R), bool)
    w = dict(occ=0.0, sig=0.0, lam=0.0, resid=float(v["eig"][0, :, :, 1].max()))
    for ch in GS.channels(N):
        z_ref[ch], ok[ch], wo, ws = P._check_channel((name, N, R, ch), dev, sv, ch, R, v["cand"][0, ch], v["occ"][0, ch],
                                                     v["raw"][0, ch], v["eig"][0, ch])
        c = GS.census(name, N, R, ch)
        w["occ"] = max(w["occ"], wo); w["sig"] = max(w["sig"], ws)
        w["lam"] = max(w["lam"], float((np.abs(v["eig"][0, ch, :, 0] - c["lam0"]) / c["hnorm"]).max()))
    w["product sig"] = _product_rule((name, N, R), _render(name, N, R, validate=False)["raw"][0], z_ref, ok)
    w["excluded"] = int((~ok).sum()); w["pixels"] = int(ok.size)
    WORST[(name, N, R)] = w
    print(f"[gs designed] {name} N={N} R={R}: {w['excluded']} of {w['pixels']} pixels excluded (relative gap <= {H.GAP_MIN}); worst "
          f"|occ - oracle| {w['occ']:.2e}, relative signal error {w['sig']:.2e} (product mode {w['product sig']:.2e}), "
          f"|lam - eigh| / ||H|| {w['lam']:.2e}, residual {w['resid']:.2e}; tasks of env 0's own launch {v['own']}")


@pytest.mark.parametrize("K", GS.KEPT)
def test_kept_set_sizes(K):
    """one_sector with K kept states: both sides of every class boundary (8 | 9-10 | 11-12 | 13+) and of the kept-set
    instantiations 8 / 16 / 32, by the K rule of test_gpu_num_charge_states, then product mode against the same reference"""
    import test_gpu_num_charge_states as NK
    name, N, R = "one_sector", 5, 16
    par, st = GS.make(name, N, R)
    dev = H.dev_view(N, par); sv = H.state_view(N, st)
    v = _render(name, N, R, K)
    p = _render(name, N, R, K, validate=False)
    worst = 0.0; excluded = 0
    for ch in GS.KEPT_CHANNELS:
        z, ok = NK._check_channel((name, K, ch), dev, sv, ch, R, K, v["cand"][0, ch], v["occ"][0, ch], v["raw"][0, ch], v["eig"][0, ch])
        worst = max(worst, _product_rule((name, K, ch), p["raw"][0, ch], z, ok)); excluded += int((~ok).sum())
    # the pixels whose winning block has s states solved at least that many tasks of s states (the other channels only add)
    win = GS.by_key(GS.size_counts(name, N, R, K, chs=GS.KEPT_CHANNELS)[1])
    print(f"[gs designed] one_sector K={K}: {excluded} of {len(GS.KEPT_CHANNELS) * R * R} pixels excluded, product mode worst "
          f"relative signal error {worst:.2e}; tasks {v['own']}")
    for k in GS.SIZE_KEYS:
        assert v["own"][k] >= win[k], (K, k, v["own"], win)


@pytest.mark.parametrize("name,N,R", GS.MEMBERS)
def test_device_counters_between_winners_and_components(name, N, R):
    """From the device's own counters: of every size (2 .. 8 states, 9 and more) at least as many tasks as pixels whose winning
    component has that size -- the winner is always a task -- and at most as many as components of that size -- pruning only
    removes tasks."""
    own = _render(name, N, R)["own"]
    comp, win = GS.size_counts(name, N, R)
    lo, hi = GS.by_key(win), GS.by_key(comp)
    for k in GS.SIZE_KEYS:
        assert lo[k] <= own[k] <= hi[k], (name, k, lo[k], own[k], hi[k])
    assert own["wide_tasks"] == 0 and own["tasks"] == sum(own[k] for k in GS.SIZE_KEYS), own


def test_every_size_class_was_solved_on_the_device():
    total = {k: 0 for k in GS.SIZE_KEYS}
    for name, N, R in GS.MEMBERS:
        for k in GS.SIZE_KEYS:
            total[k] += _render(name, N, R)["own"][k]
    print(f"[gs designed] tasks by size over the members' own launches: {total}")
    assert all(total[k] > 0 for k in GS.SIZE_KEYS), total
    # the full batches: 256 tasks of 32 states in every batch of ("one_sector", 5, 16), nothing else
    assert _render("one_sector", 5, 16)["own"]["9+"] == 4 * GS.PPB and _render("one_sector", 5, 17)["own"]["9+"] == 4 * 289


@pytest.mark.parametrize("validate", [True, False], ids=["validate", "product"])
@pytest.mark.parametrize("R", [16, 17])
def test_full_slab_leaves_the_neighbour_alone(R, validate):
    """256 pixels of one 32-state block each fill a batch's pool exactly (qd_gs_pool_doubles); at 17 x 17 a channel's second
    batch ends in a half-wave that runs a clamped duplicate beside a live 32-state pixel.  The sampled neighbour in env 1 must
    render the bits it renders beside an ordinary sampled env 0 (the designed env itself is compared with the oracle above)."""
    a = _render("one_sector", 5, R, validate=validate); b = _render(SAMPLED, 5, R, validate=validate)
    for key in (("raw", "occ", "eig") if validate else ("raw",)):
        assert np.array_equal(_bits(a[key][1]), _bits(b[key][1])), (R, validate, key)
        assert not np.array_equal(_bits(a[key][0]), _bits(b[key][0]))
    assert np.isfinite(a["raw"]).all() and np.ptp(a["raw"][0]) > 0.0 and np.ptp(a["raw"][1]) > 0.0


@pytest.mark.parametrize("name,N,R", GS.MEMBERS)
def test_pruning_flag_changes_no_bit(name, N, R):
    """QD_FLAG_GS_GERSHGORIN_ZERO (prune against the bound 0 alone) against the default pair bound: the pruned components
    cannot win, so every output agrees bit for bit, in both modes, and the tasks do not grow"""
    zero = _render(name, N, R, zero=True); pair = _render(name, N, R)
    for key in ("raw", "occ", "eig"):
        assert np.array_equal(_bits(zero[key]), _bits(pair[key])), (name, key)
    assert pair["own"]["tasks"] <= zero["own"]["tasks"], (pair["own"], zero["own"])
    for k in GS.SIZE_KEYS:
        assert pair["own"][k] <= zero["own"][k], (k, pair["own"], zero["own"])
    pzero = _render(name, N, R, validate=False, zero=True); ppair = _render(name, N, R, validate=False)
    assert np.array_equal(_bits(pzero["raw"]), _bits(ppair["raw"])), (name, "product raw")
    print(f"[gs designed] {name} N={N} R={R}: tasks {zero['own']['tasks']} (bound 0) -> {pair['own']['tasks']} (pair bound)")


def test_zero_against_denormal_coupling():
    """cut_pair (tc[1] == 0.0: pair 1 links nothing, blocks of 1..15 states) and denormal_pair (tc[1] ~ 1e-316: it links, one
    block of 32) are the same physics solved through different tasks.  Each agrees with its own oracle within 1e-6 (the
    parity test above); so their occupations agree within 2e-6 wherever both resolve."""
    N, R = 5, 16
    a = _render("cut_pair", N, R); b = _render("denormal_pair", N, R)
    assert np.array_equal(a["cand"][0], b["cand"][0])
    worst = 0.0
    for ch in GS.channels(N):
        ok = (GS.census("cut_pair", N, R, ch)["rel_gap"] > H.GAP_MIN) & (GS.census("denormal_pair", N, R, ch)["rel_gap"] > H.GAP_MIN)
        d = np.abs(a["occ"][0, ch] - b["occ"][0, ch]).max(axis=1)
        worst = max(worst, float(d[ok].max()))
        assert np.all(d[ok] <= 2e-6), (ch, float(d[ok].max()))
    print(f"[gs designed] cut_pair against denormal_pair: worst occupation difference {worst:.2e}")
    assert a["own"] != b["own"] and b["own"]["9+"] == 4 * GS.PPB


def test_probe_and_points_on_the_full_sector():
    """qd_probe, qd_probe_ex and qd_eval_points launch the same three kernels with other geometry: the one_sector scene at
    the envs' own voltages.  Bit-equal where the probe and points tests demand it of a step -- the probe's signal and the
    points' signal against the step's raw signal (test_gpu_probe, test_gpu_points), qd_probe_ex's signal against qd_probe's
    (test_gpu_probe_noise), the points' occupations against a validate handle's -- and the occupations of qd_probe_ex, which
    no step hands out in product mode, against the oracle by the 1e-6 rule."""
    import torch
    name, N, R = "one_sector", 5, 16
    L = layout(N); C = N - 1; P = R * R
    pars, sts = _blocks(name, N, R)
    S = np.stack(sts)
    gv = S[:, L.s_gate_v:L.s_gate_v + N]; bv = S[:, L.s_barrier_v:L.s_barrier_v + C]; sens = S[:, L.s_sensor_gt]
    v_ext = np.stack([PH.scan_points(N, pars[e], sts[e], R) for e in range(2)])             # (2, C P, 2N)
    env = _env(N, R, 32, False)
    _load(env, pars, sts)
    env.observe()
    step_raw = env.raw()[0]
    plain = env.probe([0, 1], gv, bv, sensor_voltage=sens)
    ex = env.probe([0, 1], gv, bv, sensor_voltage=sens, occupations=True)
    pts = env.eval_points([0, 1], v_ext[..., :N + 1], v_ext[..., N + 1:])
    torch.cuda.synchronize()
    got = {"probe": plain["raw"].cpu().numpy().reshape(2, C, P), "probe_ex": ex["raw"].cpu().numpy().reshape(2, C, P),
           "probe_ex occ": ex["occupations"].cpu().numpy().reshape(2, C, P, N),
           "points": pts["signal"].cpu().numpy().reshape(2, C, P), "points occ": pts["occupations"].cpu().numpy().reshape(2, C, P, N)}
    env.close()
    assert np.array_equal(_bits(step_raw), _bits(_render(name, N, R, validate=False)["raw"]))
    for key in ("probe", "probe_ex", "points"):
        assert np.array_equal(_bits(got[key]), _bits(step_raw)), key
    assert np.array_equal(_bits(got["points occ"]), _bits(_render(name, N, R)["occ"])), "points occ"
    worst = 0.0
    for ch in GS.channels(N):
        c = GS.census(name, N, R, ch)
        d = np.abs(got["probe_ex occ"][0, ch] - c["ref"]["occ"]).max(axis=1)
        assert np.all(c["rel_gap"][d > 1e-6] <= H.GAP_MIN), (ch, float(d.max()))
        worst = max(worst, float(d[c["rel_gap"] > H.GAP_MIN].max()))
    print(f"[gs designed] one_sector: qd_probe_ex occupations against the oracle, worst {worst:.2e}")
