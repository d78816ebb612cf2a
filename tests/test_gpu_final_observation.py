"""Episode ends under auto-reset on the GPU: qd_snapshot captures a truncating env's outputs, state and parameters
after its last step and before the in-step reset replaces the device -- bit-identical to a twin env that is never
reset, and equal to the oracle's observation of the old device; final_observation="step" and the distance / cgd logs
on the HIP backend; the C ABI's argument checks."""
import ctypes

import numpy as np
import pytest
import yaml

import helpers as H
import qd_oracle as O
from qadapt_hip import device_model as DM

pytestmark = pytest.mark.gpu

N, R, B, MAX, SEED = 4, 16, 6, 3, 4242          # stagger: env e starts at step e mod 3 -> envs {2,5}, {1,4}, {0,3} end


def _cfg(tmp_path):
    cfg = DM.load_yaml(None, "env_config.yaml")
    cfg["simulator"]["max_steps"] = MAX
    cfg["capacitance_model"]["update_method"] = None          # deterministic physics, no CNN in the loop
    p = tmp_path / "env.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def _vec(path):
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    env = VecQuantumDeviceEnv(B, num_dots=N, resolution=R, config_path=path, seed=SEED)
    env.reset()
    env.stagger_episodes()
    return env


def _actions():
    return np.random.default_rng(7).uniform(-1, 1, (MAX, B, 2 * N - 1)).astype(np.float32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def test_snapshot_is_the_last_step_of_the_old_device(tmp_path):
    import torch
    path = _cfg(tmp_path)
    main, twin = _vec(path), _vec(path)
    acts = _actions()
    seen = []
    for t in range(MAX):
        a = torch.as_tensor(acts[t]).cuda()
        main.step(a, auto_reset=True, keep_final=True)
        twin.step(a)                                          # never reset: its envs stay on their first device
        f = main.final
        ids = np.nonzero(twin._steps_host == MAX)[0]
        assert f is not None and np.array_equal(f["env_ids"], ids) and 0 < ids.size < B, (t, f and f["env_ids"])
        raw, _ = twin.raw()                                   # (synchronises)
        st, steps = twin.get_state()
        for name in ("global_image", "plunger_images", "barrier_images", "voltages"):
            got, want = f[name].cpu().numpy(), getattr(twin, name).cpu().numpy()[ids]
            assert np.array_equal(_bits(got), _bits(want)), (t, name)
            if name != "voltages":                            # the live buffers already hold the new devices
                assert not np.array_equal(got, getattr(main, name).cpu().numpy()[ids]), (t, name)
        assert np.array_equal(_bits(f["state"].cpu().numpy()), _bits(st[ids]))
        assert np.array_equal(_bits(f["params"].cpu().numpy()), _bits(twin._params_host[ids]))
        assert np.array_equal(f["steps"].cpu().numpy(), steps[ids]) and np.all(steps[ids] == MAX)
        fds, tds = main.final_device_state(), twin.device_state()
        for k, v in fds.items():
            assert np.array_equal(v, np.asarray(tds[k])[ids]), (t, k)
        assert np.array_equal(main.cgd_full_of(f["params"].cpu().numpy()), twin.cgd_full_of(twin._params_host[ids]))
        if t == 0:                                            # env 2 began at step 2: one step on its first device
            k = int(np.nonzero(ids == 2)[0][0])
            oe = O.OracleEnv(N, R, max_steps=MAX, update_method=None)
            zero = np.zeros((N - 1, 3), np.float32)
            oe.reset(O.sample_episode(np.random.default_rng(SEED + 2), N), zero, zero)
            oobs, _, _, otrunc = oe.step(acts[0][2, :N], acts[0][2, N:], zero, zero)
            img = f["global_image"][k].cpu().numpy()
            H.image_parity(oe, img, raw[2])
            ag = O.agent_images(img, N)
            pim, bim = f["plunger_images"][k].cpu().numpy(), f["barrier_images"][k].cpu().numpy()
            assert all(np.array_equal(pim[i], ag[f"plunger_{i}"]) for i in range(N))
            assert all(np.array_equal(bim[j], ag[f"barrier_{j}"]) for j in range(N - 1))
            v = f["voltages"][k].cpu().numpy()
            assert np.allclose(v[:N], oobs["obs_gate_voltages"], rtol=1e-6, atol=1e-6)
            assert np.allclose(v[N:], oobs["obs_barrier_voltages"], rtol=1e-6, atol=1e-6)
            cgd = O.device_from_sample(O.sample_episode(np.random.default_rng(SEED + 2), N)).cgd_full
            assert np.allclose(main.cgd_full_of(f["params"][k:k + 1].cpu().numpy())[0], cgd, rtol=1e-12, atol=0)
        seen.extend(ids.tolist())
    assert sorted(seen) == list(range(B))
    main.close(); twin.close()


class _CountingLib:
    def __init__(self, lib):
        object.__setattr__(self, "_lib", lib)
        object.__setattr__(self, "counts", {})

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("qd_"):
            return fn

        def wrapped(*a):
            self.counts[name] = self.counts.get(name, 0) + 1
            return fn(*a)
        return wrapped


def _batched(path, **kw):
    from qadapt_hip.multi_agent import BatchedMultiAgentEnv
    env = BatchedMultiAgentEnv(B, num_dots=N, resolution=R, seed=SEED, env_config_path=path, return_voltage=True,
                               return_global_state=True, **kw)
    for v in env.views:
        v.reset()
    env.vec.stagger_episodes()
    return env


def _agent_acts(acts_t, ids):
    return [{a: acts_t[b, k:k + 1] for k, a in enumerate(ids)} for b in range(B)]


def test_step_mode_returns_the_old_episode_and_reset_the_new_one(tmp_path):
    path = _cfg(tmp_path)
    step_env, plain = _batched(path, final_observation="step"), _batched(path)
    ids = step_env.roster.ids
    acts = _actions()
    for t in range(MAX):
        for env in (step_env, plain):
            for b, a in enumerate(_agent_acts(acts[t], ids)):
                env.views[b].stage(a)
        f = step_env.vec.final
        fp = {n: f[n].cpu().numpy() for n in ("plunger_images", "barrier_images", "voltages", "global_image")}
        fds = step_env.vec.final_device_state()
        slot = {int(e): k for k, e in enumerate(f["env_ids"])}
        res = [v.collect() for v in step_env.views]
        pres = [v.collect() for v in plain.views]
        for b in range(B):
            obs, rew, term, trunc, info = res[b]
            assert rew == pres[b][1] and trunc == pres[b][3]
            if b not in slot:
                assert not trunc["__all__"]
                continue
            k = slot[b]
            assert trunc["__all__"]
            for i, a in enumerate(ids):
                img = fp["plunger_images"][k, i] if i < N else fp["barrier_images"][k, i - N]
                assert np.array_equal(_bits(obs[a]["image"]), _bits(img))
                assert np.array_equal(_bits(obs[a]["voltage"]), _bits(fp["voltages"][k, i:i + 1]))
                assert np.array_equal(_bits(obs[a]["global_image"]), _bits(fp["global_image"][k]))
                kind, j = ("gate", i) if i < N else ("barrier", i - N)
                assert info[a] == {"ground_truth": fds[f"{kind}_ground_truth"][k][j],
                                   "current_voltage": fds[f"current_{kind}_voltages"][k][j]}
            vec = step_env.vec
            vec._lib = counting = _CountingLib(vec._lib)
            launches = step_env.launches
            o2, i2 = step_env.views[b].reset()               # the new episode's first observation, no launch
            vec._lib = counting._lib
            assert counting.counts == {} and step_env.launches == launches
            assert int(i2["plunger_0"]["current_device_state"]["steps"]) == 0
            po = pres[b][0]                                  # what mode None handed out for this step
            for a in ids:
                for key in ("image", "voltage", "global_image", "global_voltages"):
                    assert np.array_equal(_bits(o2[a][key]), _bits(po[a][key])), (t, b, a, key)
            plain.views[b].reset()
    step_env.close(); plain.close()


def _expected_logs(twin_ds, truncs, collecting):
    """The reference wrapper's file sequence (multi_agent_wrapper.py:459-570) for views reset once, then stepped, a
    truncated view reset after each step: list of (kind, payload) in count order per folder kind."""
    hist = {b: [] for b in range(B)}
    files = []
    for ds, tr in zip(twin_ds, truncs):
        for b in range(B):
            if tr[b]:
                files.append(("dist", list(hist[b])))
                if collecting:
                    files.append(("cgd", b))
                hist[b] = []
            d = np.concatenate([ds["current_gate_voltages"][b] - ds["gate_ground_truth"][b],
                                ds["current_barrier_voltages"][b] - ds["barrier_ground_truth"][b]])
            hist[b].append(d)
        for b in range(B):
            if tr[b]:
                if not collecting:
                    files.append(("dist", list(hist[b])))
                hist[b] = []
    return files


@pytest.mark.parametrize("collecting", [False, True])
def test_distance_and_cgd_logs_on_the_hip_backend(tmp_path, collecting):
    import glob
    import json
    import os
    import torch
    path = _cfg(tmp_path)
    out = tmp_path / "logs"
    env = _batched(path, distance_data_dir=str(out), is_collecting_data=collecting)
    twin = _vec(path)
    ids = env.roster.ids
    acts = _actions()
    twin_ds, truncs = [], []
    for t in range(MAX):
        for b, a in enumerate(_agent_acts(acts[t], ids)):
            env.views[b].stage(a)
        res = [v.collect() for v in env.views]
        twin.step(torch.as_tensor(acts[t]).cuda())
        twin_ds.append(twin.device_state())
        truncs.append([r[3]["__all__"] for r in res])
        assert truncs[-1] == [bool(s == MAX) for s in twin._steps_host]
        for b in range(B):
            if truncs[-1][b]:
                env.views[b].reset()
    want = _expected_logs(twin_ds, truncs, collecting)
    dist = [w for w in want if w[0] == "dist"]
    for k, a in enumerate(ids):
        files = sorted(glob.glob(os.path.join(out, a, "*.npy")))
        assert [int(os.path.basename(f)[:4]) for f in files] == list(range(1, len(dist) + 1))
        for f, (_, rows) in zip(files, dist):
            arr = np.load(f)
            assert arr.dtype == np.float64 and np.array_equal(arr, np.array([r[k] for r in rows], np.float64)), (a, f)
    cgds = sorted(glob.glob(os.path.join(out, "cgd", "*.json")))
    cgd_envs = [w[1] for w in want if w[0] == "cgd"]
    assert len(cgds) == len(cgd_envs) == (B if collecting else 0)
    for f, b in zip(cgds, cgd_envs):
        got = np.array(json.load(open(f)))
        assert np.array_equal(got, twin.cgd_full_of(twin._params_host[b:b + 1])[0])
        ref = O.device_from_sample(O.sample_episode(np.random.default_rng(SEED + b), N)).cgd_full
        assert np.allclose(got, ref, rtol=1e-12, atol=0)
    env.close(); twin.close()


def test_snapshot_argument_checks(tmp_path):
    import torch
    from qadapt_hip import _lib
    env = _vec(_cfg(tmp_path))
    L, h, st = env._lib, env._h, env._stream()
    nul = ctypes.c_void_p(None)
    ids = torch.tensor([4, -1, B, 1], dtype=torch.int32, device=env.device)
    vol = torch.full((4, 2 * N - 1), -7.0, dtype=torch.float32, device=env.device)
    steps = torch.full((4,), -7, dtype=torch.int32, device=env.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert L.qd_snapshot(h, p(ids), 0, nul, nul, nul, p(vol), nul, nul, p(steps), st) == 0
    assert L.qd_snapshot(h, p(ids), B + 1, nul, nul, nul, p(vol), nul, nul, p(steps), st) == 1
    assert L.qd_snapshot(h, nul, 2, nul, nul, nul, p(vol), nul, nul, p(steps), st) == 1
    assert L.qd_snapshot(h, p(ids), 4, nul, nul, nul, nul, nul, nul, nul, st) == 0
    torch.cuda.synchronize()
    assert bool((vol == -7.0).all()) and bool((steps == -7).all())                    # nothing written so far
    _lib.check(h, L.qd_snapshot(h, p(ids), 4, nul, nul, nul, p(vol), nul, nul, p(steps), st), "qd_snapshot")
    torch.cuda.synchronize()
    live, sv = env.voltages.cpu().numpy(), env.get_state()[1]
    v, s = vol.cpu().numpy(), steps.cpu().numpy()
    assert np.array_equal(v[0], live[4]) and np.array_equal(v[3], live[1])
    assert np.array_equal(s[[0, 3]], sv[[4, 1]])
    assert np.all(v[1:3] == -7.0) and np.all(s[1:3] == -7)                             # ids outside [0, B) skipped
    env.close()
