"""The mixed-N latched batch (BASELINE config 5: dot counts {2, 4, 6, 8} in one process, one handle per dot count, the
latched model on, auto_reset) on the MI355X, through steps and automatic resets, against the oracle (run with -m gpu).
The scenes are those of tests/mixed_cases.py; tests/test_mixed_cases_cpu.py holds their conditions.

Scene A (deterministic state, designed actions; noise ["latch"] -- config 5 -- and ("sensor", "radial", "latch")), whole job on
the streams of MixedVecQuantumDeviceEnv, validate mode.  First the handles' states must BE the host-side trajectory.  After
steps 2 and 3, for the compared envs of every bucket (a near env that was not reset, the envs reset in that step -- observation
number S + 1, rendered through an env-id list -- and the mid env):
  (a) a noise-free twin handle is given the bucket's parameter blocks and state rows and renders the un-latched occupations of
      the device itself; the numpy restatement (oracle/qd_noise_oracle.py) walks THOSE, so every pixel of every channel is
      compared, none exempt: latched occupations bit for bit, raw signal at rtol 1e-6 / atol 1e-9, a radial-replaced channel
      at 1e-12;
  (b) the twin's occupations and signal against the C oracle by the project's per-pixel rule (envs 0 and 2, and the first
      reset env at step 2; the far env 3 is left to (a), (c), (d), (e));
  (c) image and percentiles are numpy's of the raw signal, bit for bit;
  (d) rewards and truncation flags of every step are the oracle's;
  (e) the same bits per global env id at every step from the whole job with and without streams, the two shards of world = 2
      and four homogeneous handles stepped one after the other.
Scene B (the benched setup: Kalman updater with a synthetic capacitance model per bucket, product mode, random actions,
staggered episodes with a reset in every bucket at every step, no host wait between steps): streams, no streams and
homogeneous handles give the same bits.

The observation number of the noise streams counts the observes of a HANDLE, partial ones included.  Two shards whose envs
reset in different steps therefore drift apart from the step after; scene A ends with step 3, the first step in which only
one shard resets, so (e) never reaches that state ("The mixed latched batch").

Measured on the MI355X (seed 1; DESIGN.md has the table per bucket): (a) latched occupations equal in every pixel, worst raw
deviation 1.0e-11 relative to max(|z|, 1e-3); (b) worst occupation deviation 1.1e-11, signal 3.6e-12, no pixel exempt."""
import ctypes

import numpy as np
import pytest

import helpers as H
import mixed_cases as MC
import qd_noise_oracle as NO
import qd_oracle as O
import qd_oracle_c as OC
from test_gpu_parity import RESID_MAX

pytestmark = pytest.mark.gpu

BUCKETS = sorted(MC.COUNTS)
FIELDS = ("raw", "plohi", "image", "rewards", "truncated", "state", "steps")
_RUNS = {}
_TWINS = {}


@pytest.fixture(scope="module")
def cfg_path(tmp_path_factory):
    return MC.write_env_config(str(tmp_path_factory.mktemp("mixed_scene_a")))


def _kw(variant, cfg_path):
    return dict(resolution=MC.R, seed=MC.SEED, noise=list(MC.VARIANTS[variant]), validate=True, env_chunk=MC.ENV_CHUNK,
                config_path=cfg_path)


def _preset(env):
    """the scene's step counters, through set_state after reset()"""
    st, _ = env.get_state()
    env.set_state(st, MC.preset_steps(env.max_steps, env.env_id_offset - MC.bucket_first(env.N), env.B))


def _record(env, out):
    """what env shows after a step, per global env id"""
    raw, plohi = env.raw()
    st, steps = env.get_state()
    img, rew, trunc = env.global_image.cpu().numpy(), env.rewards.cpu().numpy(), env.truncated.cpu().numpy()
    for k in range(env.B):
        out[env.env_id_offset + k] = dict(raw=raw[k].copy(), plohi=plohi[k].copy(), image=img[k].copy(), rewards=rew[k].copy(),
                                          truncated=trunc[k].copy(), state=st[k].copy(), steps=steps[k].copy())


def _actions(env, t):
    import torch
    tr = MC.trajectory(env.N)
    lo = env.env_id_offset - tr.first
    return torch.as_tensor(tr.actions[t, lo:lo + env.B]).to(env.device)


def _checkpoint(env):
    ck = env.get_checkpoint()
    return dict(params=ck["params"], state=ck["state"], steps=ck["steps"], obs_serial=ck["obs_serial"], occ=env.occupations(),
                raw=env.raw()[0], plohi=env.raw()[1], image=env.global_image.cpu().numpy().copy())


def _run_a(variant, mode, cfg_path):
    """Scene A in one of the four ways of running the job.  Returns {"steps": [per step {global id: fields}], "ck": {(N, t):
    checkpoint}} -- checkpoints only for the whole job on streams."""
    import torch
    from qadapt_hip.mixed import MixedVecQuantumDeviceEnv
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    key = (variant, mode)
    if key in _RUNS:
        return _RUNS[key]
    kw = _kw(variant, cfg_path)
    res = dict(steps=[dict() for _ in range(MC.T)], ck={})
    if mode in ("streams", "no_streams", "shards"):
        jobs = [dict(rank=r, world=2) for r in range(2)] if mode == "shards" else [dict(rank=0, world=1)]
        for job in jobs:
            mix = MixedVecQuantumDeviceEnv(MC.COUNTS, streams=mode != "no_streams", **job, **kw)
            mix.reset()
            for env in mix.buckets.values():
                _preset(env)
            for t in range(MC.T):
                mix.step({N: _actions(env, t) for N, env in mix.buckets.items()}, auto_reset=True)
                for N, env in mix.buckets.items():
                    _record(env, res["steps"][t])
                    if mode == "streams" and t in MC.CHECK_STEPS:
                        res["ck"][(N, t)] = _checkpoint(env)
            mix.close()
    else:
        envs = {N: VecQuantumDeviceEnv(MC.COUNTS[N], num_dots=N, env_id_offset=MC.bucket_first(N), **kw) for N in BUCKETS}
        for env in envs.values():
            env.reset(); torch.cuda.synchronize()
            _preset(env)
        for t in range(MC.T):
            for env in envs.values():
                env.step(_actions(env, t), auto_reset=True); torch.cuda.synchronize()
            for env in envs.values():
                _record(env, res["steps"][t])
        for env in envs.values():
            env.close()
    _RUNS[key] = res
    return res


def _twin(variant, N, t, cfg_path):
    """A noise-free handle with the parameter blocks, state rows and step counters the bucket holds after step t: what it
    renders are the device's own occupations before latching, its signal before any noise stage."""
    from qadapt_hip import _lib
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    key = (variant, N, t)
    if key not in _TWINS:
        ck = _run_a(variant, "streams", cfg_path)["ck"][(N, t)]
        n = MC.COUNTS[N]
        tw = VecQuantumDeviceEnv(n, num_dots=N, resolution=MC.R, seed=MC.SEED, env_id_offset=MC.bucket_first(N), env_chunk=MC.ENV_CHUNK,
                                 validate=True, config_path=cfg_path)
        ids = np.arange(n, dtype=np.int32)
        params, state = np.ascontiguousarray(ck["params"]), np.ascontiguousarray(ck["state"])
        _lib.check(tw._h, tw._lib.qd_load_episodes(tw._h, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n, params.ctypes.data,
                                                   state.ctypes.data, 0, tw._stream()), "qd_load_episodes")
        tw.set_state(state, ck["steps"])
        tw.observe()
        _TWINS[key] = dict(occ=tw.occupations(), raw=tw.raw()[0], cand=tw.candidates(), eig=tw.eigen())
        assert np.array_equal(tw.get_state()[0], state)
        tw.close()
    return _TWINS[key]


@pytest.mark.parametrize("variant", list(MC.VARIANTS))
def test_states_rewards_and_truncation_are_the_host_trajectory(variant, cfg_path):
    """get_state() after every step equals the trajectory rebuilt without the GPU (voltages, ground truths and VGM at rtol
    1e-13, step counters exactly), so the conditions of the CPU tier hold for this run; (d) rewards and truncation flags of
    every env and step are the oracle's, at the rule of test_episode_matches_oracle_env."""
    run = _run_a(variant, "streams", cfg_path)
    for N in BUCKETS:
        tr = MC.trajectory(N)
        L = tr.L
        for t in range(MC.T):
            for i in range(tr.n):
                got = run["steps"][t][tr.first + i]
                assert np.allclose(got["state"][:L.s_kmean], tr.state[t, i], rtol=1e-13, atol=0.0), (N, t, i)
                assert int(got["steps"]) == int(tr.steps[t, i]), (N, t, i)
                assert np.allclose(got["rewards"], tr.rewards[t, i], rtol=1e-9, atol=1e-12), (N, t, i)
                assert bool(got["truncated"]) == bool(tr.truncated[t, i]), (N, t, i)
        for t in MC.CHECK_STEPS:
            ck = run["ck"][(N, t)]
            assert np.allclose(ck["params"], tr.params[t], rtol=1e-13, atol=0.0), (N, t)
            assert ck["obs_serial"] == tr.ck_serial[t], (N, t)


@pytest.mark.parametrize("t", MC.CHECK_STEPS)
@pytest.mark.parametrize("N", BUCKETS)
@pytest.mark.parametrize("variant", list(MC.VARIANTS))
def test_stochastic_stages_exact_and_images(variant, N, t, cfg_path):
    """(a) and (c)."""
    flags = set(MC.VARIANTS[variant])
    ck = _run_a(variant, "streams", cfg_path)["ck"][(N, t)]
    tw = _twin(variant, N, t, cfg_path)
    tr = MC.trajectory(N)
    L = tr.L
    reset_here = [i for i in MC.compared(t) if tr.truncated[t, i]]
    assert reset_here
    worst = 0.0; latched = 0; latched_reset = 0; replaced = 0
    for i in MC.compared(t):
        par, st = ck["params"][i], ck["state"][i]
        dev, sv = H.dev_view(N, par), H.state_view(N, st)
        # the checkpoint's observation number for the envs reset in this step, one less for the others
        serial = ck["obs_serial"] if i in reset_here else ck["obs_serial"] - 1
        assert serial == tr.serial[t, i]
        stream = NO.Stream(MC.SEED, tr.first + i, serial)
        nz = MC.noise_params(par, L)
        p_leads, p_inter = MC.latch_probabilities(par, L)
        for ch in range(N - 1):
            z, used = NO.observe_channel(dev, nz, stream, ch, MC.R, sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, sv.barrier_v,
                                         dev.window, sv.gate_gt, tw["occ"][i, ch], flags, p_leads, p_inter)
            tag = (variant, N, t, i, ch)
            if "radial" in flags and NO.radial_replaced(sv.gate_v[ch], sv.gate_v[ch + 1], sv.gate_gt[ch], sv.gate_gt[ch + 1],
                                                        nz["full_noise_distance"]):
                assert np.allclose(ck["raw"][i, ch], z, rtol=1e-12, atol=1e-12), tag               # the pure N(0, 1) image
                replaced += 1
                continue
            assert np.array_equal(ck["occ"][i, ch], used), (tag, int((ck["occ"][i, ch] != used).any(axis=1).sum()))
            dz = np.abs(ck["raw"][i, ch] - z)
            worst = max(worst, float((dz / np.maximum(np.abs(z), 1e-3)).max()))
            assert np.allclose(ck["raw"][i, ch], z, rtol=1e-6, atol=1e-9), (tag, float(dz.max()))
            n_lat = int((used != tw["occ"][i, ch]).any(axis=1).sum())
            latched += n_lat
            latched_reset += n_lat if i in reset_here else 0
        # (c) the image and the percentiles are numpy's of the raw signal
        raw = ck["raw"][i]
        assert np.array_equal(ck["image"][i], O.normalise_image(raw.reshape(N - 1, MC.R, MC.R).transpose(1, 2, 0))), (variant, N, t, i)
        assert np.array_equal(ck["plohi"][i], np.percentile(raw, [0.5, 99.5])), (variant, N, t, i)
    print(f"[mixed latched, {variant}] N={N} step {t} envs {MC.compared(t)}: worst |raw - restatement| / max(|z|, 1e-3) = {worst:.2e}; "
          f"latched pixels {latched}, of them in the envs reset in this step {latched_reset}; radial-replaced channels {replaced}")
    assert latched > 0, "the scene was meant to contain latched pixels"


@pytest.mark.parametrize("t", MC.CHECK_STEPS)
@pytest.mark.parametrize("N", BUCKETS)
def test_physics_under_the_stages_against_the_c_oracle(N, t, cfg_path):
    """(b) on the twin of the config-5 variant.  The all-stages variant walks the same states (asserted), so its twin renders
    the same bits."""
    tw = _twin("latch", N, t, cfg_path)
    ck = _run_a("latch", "streams", cfg_path)["ck"][(N, t)]
    other = _run_a("all", "streams", cfg_path)["ck"][(N, t)]
    assert np.array_equal(ck["state"], other["state"]) and np.array_equal(ck["params"], other["params"])
    tr = MC.trajectory(N)
    envs = [0, 2] + [i for i in MC.compared(t) if tr.truncated[t, i] and MC.ROLES[i] != "far"][:1]
    worst = dict(occ=0.0, sig=0.0, res=0.0, lam=0.0)
    shares = {}
    for i in envs:
        dev, sv = H.dev_view(N, ck["params"][i]), H.state_view(N, ck["state"][i])
        exempt = 0
        for ch in range(N - 1):
            tag = (N, t, i, ch)
            ref = OC.csd_channel(dev, sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, sv.barrier_v, dev.window, ch, MC.R)
            assert np.array_equal(tw["cand"][i, ch], ref["states"]), tag
            sp = MC.spectrum(dev, sv, ch, ref["states"])
            ok = sp["rel_gap"] > H.GAP_MIN
            exempt += int((~ok).sum())
            eig = tw["eig"][i, ch]
            res = float(eig[:, 1].max()); dl = float((np.abs(eig[:, 0] - sp["lam0"]) / sp["hnorm"]).max())
            assert res <= RESID_MAX, (tag, res)
            assert dl <= 1e-12, (tag, dl)
            d_occ = np.abs(tw["occ"][i, ch] - ref["occ"]).max(axis=1)
            d_sig = np.abs(tw["raw"][i, ch] - ref["z"]) / np.maximum(np.abs(ref["z"]), 1e-3)
            if ok.any():
                worst["occ"] = max(worst["occ"], float(d_occ[ok].max())); worst["sig"] = max(worst["sig"], float(d_sig[ok].max()))
            worst["res"] = max(worst["res"], res); worst["lam"] = max(worst["lam"], dl)
            assert np.all(sp["rel_gap"][d_occ > 1e-6] <= H.GAP_MIN), (tag, float(d_occ[ok].max()) if ok.any() else None)
            assert np.all(sp["rel_gap"][d_sig > 1e-6] <= H.GAP_MIN), (tag, float(d_sig[ok].max()) if ok.any() else None)
            tot = tw["occ"][i, ch].sum(axis=1)
            assert np.abs(tot - np.round(tot)).max() < 1e-9, tag
        shares[i] = exempt / ((N - 1) * MC.R * MC.R)
        if not tr.truncated[t, i]:
            assert shares[i] <= (MC.NEAR_EXEMPT_MAX if MC.ROLES[i] == "near" else MC.MID_EXEMPT_MAX), (N, t, i, shares[i])
    print(f"[mixed latched, physics] N={N} step {t} envs {envs}: worst |occ - oracle| {worst['occ']:.2e}, rel signal error {worst['sig']:.2e} "
          f"over the pixels above the gap; exempt shares {shares}; every pixel: residual <= {worst['res']:.1e}, "
          f"|lam - lam_oracle| / ||H|| <= {worst['lam']:.1e}")


@pytest.mark.parametrize("variant", list(MC.VARIANTS))
def test_independent_of_how_the_job_is_run(variant, cfg_path):
    """(e)"""
    want = _run_a(variant, "streams", cfg_path)["steps"]
    for mode in ("no_streams", "shards", "homogeneous"):
        got = _run_a(variant, mode, cfg_path)["steps"]
        for t in range(MC.T):
            assert sorted(got[t]) == sorted(want[t]) == list(range(sum(MC.COUNTS.values()))), (mode, t)
            for g in want[t]:
                for f in FIELDS:
                    assert np.array_equal(got[t][g][f], want[t][g][f]), (variant, mode, t, g, f)


# ---------------------------------------------------------------------------------------------------------
# Scene B: the benched setup
# ---------------------------------------------------------------------------------------------------------
def _run_b(kind):
    """reset, stagger_episodes, presets (bucket env k < 4 truncates at step k), four steps with uniform random actions from one
    seeded CPU generator.  The mixed runs never read the device between steps: what a step shows is cloned on the stream."""
    import torch
    from qadapt_hip.mixed import MixedVecQuantumDeviceEnv
    from qadapt_hip.vec_env import VecQuantumDeviceEnv, SyntheticCapacitanceModel
    fac = lambda n: SyntheticCapacitanceModel(MC.SEED + 10 * n)
    kw = dict(resolution=MC.R, seed=MC.SEED, noise=["latch"], env_chunk=MC.ENV_CHUNK)
    mix = None
    if kind == "homogeneous":
        envs = {N: VecQuantumDeviceEnv(MC.COUNTS[N], num_dots=N, env_id_offset=MC.bucket_first(N), capacitance_model=fac(N), **kw)
                for N in BUCKETS}
        for env in envs.values():
            env.reset(); torch.cuda.synchronize()
    else:
        mix = MixedVecQuantumDeviceEnv(MC.COUNTS, capacitance_model_factory=fac, streams=kind == "streams", **kw)
        envs = mix.buckets
        mix.reset()
    assert all(env.chunk_envs() == MC.ENV_CHUNK and not env.validate for env in envs.values())
    raw0 = {N: env.raw()[0] for N, env in envs.items()}
    for env in envs.values():
        env.stagger_episodes()
        st, steps = env.get_state()
        steps[:4] = env.max_steps - 1 - np.arange(4)
        env.set_state(st, steps)
    gen = torch.Generator(device="cpu").manual_seed(MC.SEED)
    acts = [{N: (torch.rand((MC.COUNTS[N], 2 * N - 1), generator=gen) * 2 - 1).cuda() for N in BUCKETS} for _ in range(MC.T)]
    torch.cuda.synchronize()
    shown = []
    for t in range(MC.T):
        if mix is not None:
            out = mix.step(acts[t], auto_reset=True)
        else:
            out = {}
            for N, env in envs.items():
                out[N] = env.step(acts[t][N], auto_reset=True); torch.cuda.synchronize()
        shown.append({N: dict(image=o[0]["image"].clone(), voltages=envs[N].voltages.clone(), rewards=o[1].clone(), truncated=o[3].clone())
                      for N, o in out.items()})
    res = dict(raw0=raw0, steps=[{N: {k: v.cpu().numpy() for k, v in d.items()} for N, d in s.items()} for s in shown], last={})
    for N, env in envs.items():
        raw, plohi = env.raw()
        st, steps = env.get_state()
        res["last"][N] = dict(raw=raw, plohi=plohi, state=st, steps=steps)
    for env in envs.values():
        env.close()
    return res


def test_benched_setup_streams_no_streams_and_homogeneous_handles_agree():
    from qadapt_hip.vec_env import VecQuantumDeviceEnv, SyntheticCapacitanceModel
    runs = {k: _run_b(k) for k in ("streams", "no_streams", "homogeneous")}
    want = runs["homogeneous"]
    for t in range(MC.T):
        for N in BUCKETS:
            w = want["steps"][t][N]
            # some env of every bucket resets in every step
            assert w["truncated"].tolist() == [k == t for k in range(MC.COUNTS[N])], (N, t)
            assert np.isfinite(w["image"]).all() and w["image"].min() >= 0.0 and w["image"].max() <= 1.0, (N, t)
            for kind in ("streams", "no_streams"):
                for f, a in runs[kind]["steps"][t][N].items():
                    assert np.array_equal(a, w[f]), (kind, N, t, f)
    for N in BUCKETS:
        for kind in ("streams", "no_streams"):
            assert np.array_equal(runs[kind]["raw0"][N], want["raw0"][N]), (kind, N)
            for f, a in runs[kind]["last"][N].items():
                assert np.array_equal(a, want["last"][N][f]), (kind, N, f)
    # latching changed at least one bucket's raw signal against a handle without it
    changed = False
    for N in BUCKETS:
        plain = VecQuantumDeviceEnv(MC.COUNTS[N], num_dots=N, resolution=MC.R, seed=MC.SEED, env_id_offset=MC.bucket_first(N),
                                    env_chunk=MC.ENV_CHUNK, capacitance_model=SyntheticCapacitanceModel(MC.SEED + 10 * N))
        plain.reset()
        changed |= not np.array_equal(plain.raw()[0], want["raw0"][N])
        plain.close()
    assert changed, "latching was meant to change at least one bucket's raw signal"
