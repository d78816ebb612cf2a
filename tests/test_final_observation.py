"""Episode ends under auto-reset, host side (no GPU): final_observation="info" / "step" of BatchedMultiAgentEnv and
MultiAgentEnvWrapper, and the reference wrapper's distance-history / cgd logs (multi_agent_wrapper.py:118-133,
459-483, 527-570, 587-660), over a fake backend with the keep_final surface of VecQuantumDeviceEnv."""
import glob
import json
import os
import random
from pathlib import Path

import numpy as np
import pytest
import torch

from qadapt_hip.layout import layout
from qadapt_hip.multi_agent import BatchedMultiAgentEnv, MultiAgentEnvWrapper
from qadapt_hip.vec_env import cgd_full_from_params, device_state_from_rows


class FakeVec:
    """Shape-faithful stand-in for VecQuantumDeviceEnv: B envs, host tensors, real state / parameter block layout.
    Every device is numbered; its parameters, ground truth and every image are functions of (device, step), so an
    output that comes from the wrong device or step is caught.  `trace` records each step's outputs, device state and
    cgd BEFORE any automatic reset."""

    def __init__(self, B, N, R, max_steps):
        self.num_envs, self.B, self.N, self.R, self.C, self.max_steps = B, B, N, R, N - 1, max_steps
        self.L = layout(N)
        self.device = torch.device("cpu")
        C = N - 1
        self.global_image = torch.zeros((B, R, R, C), dtype=torch.float32)
        self.plunger_images = torch.zeros((B, N, R, R, 2), dtype=torch.float32)
        self.barrier_images = torch.zeros((B, C, R, R, 1), dtype=torch.float32)
        self.voltages = torch.zeros((B, 2 * N - 1), dtype=torch.float32)
        self.rewards = torch.zeros((B, 2 * N - 1), dtype=torch.float64)
        self.truncated = torch.zeros((B,), dtype=torch.uint8)
        self.state = np.zeros((B, self.L.s_size))
        self.params = np.zeros((B, self.L.size))
        self._steps_host = np.zeros(B, np.int64)
        self.dev_id = np.zeros(B, np.int64)
        self.next_device = 0
        self.final = None
        self.trace = []
        self.step_calls = []

    def _new_device(self, b):
        self.dev_id[b] = d = self.next_device
        self.next_device += 1
        rng = np.random.default_rng(1000 + d)
        self.params[b] = rng.normal(size=self.L.size)
        self.state[b] = rng.normal(size=self.L.s_size) * 3
        self._steps_host[b] = 0

    def _render(self, b):
        rng = np.random.default_rng([int(self.dev_id[b]), int(self._steps_host[b])])
        for t in (self.global_image, self.plunger_images, self.barrier_images, self.voltages):
            t[b] = torch.from_numpy(rng.random(tuple(t.shape[1:])).astype(np.float32))

    def reset(self, env_ids=None, seed=None, **kw):
        for b in (range(self.B) if env_ids is None else env_ids):
            self._new_device(int(b))
            self._render(int(b))

    def step(self, actions, auto_reset=False, keep_final=False):
        self.step_calls.append(dict(auto_reset=auto_reset, keep_final=keep_final))
        L, N = self.L, self.N
        a = np.asarray(actions, np.float64)
        for b in range(self.B):
            self._steps_host[b] += 1
            self.state[b, L.s_gate_v:L.s_gate_v + N] = 7.0 * a[b, :N] + self.dev_id[b]
            self.state[b, L.s_barrier_v:L.s_barrier_v + N - 1] = -3.0 * a[b, N:]
            self.rewards[b] = torch.from_numpy(a[b] / 10 + self.dev_id[b])
            self.truncated[b] = int(self._steps_host[b] >= self.max_steps)
            self._render(b)
        self.trace.append(dict(truncated=self.truncated.numpy().astype(bool), ds=self.device_state(),
                               cgd=self.cgd_full_of(self.params),
                               host={n: getattr(self, n).numpy().copy() for n in
                                     ("plunger_images", "barrier_images", "voltages", "global_image")}))
        done = np.nonzero(self._steps_host >= self.max_steps)[0]
        self.final = None
        if keep_final and done.size:
            self.final = {n: getattr(self, n)[torch.from_numpy(done)].clone() for n in
                          ("global_image", "plunger_images", "barrier_images", "voltages")}
            self.final.update(state=torch.from_numpy(self.state[done].copy()),
                              params=torch.from_numpy(self.params[done].copy()),
                              steps=torch.from_numpy(self._steps_host[done].astype(np.int32)), env_ids=done.astype(np.int64))
        if auto_reset:
            self.reset(env_ids=done)

    def device_state(self):
        return device_state_from_rows(self.L, self.state, self.params, self._steps_host.astype(np.int32))

    def device_state_of(self, state, params, steps):
        return device_state_from_rows(self.L, state, params, steps)

    def cgd_full_of(self, params):
        return cgd_full_from_params(self.L, params)


class ReferenceLog:
    """Literal restatement of the reference wrapper's logging (multi_agent_wrapper.py:118-133, 459-483, 527-570,
    587-660) for ONE env: glob-counted file names, save before append at an episode end, save at reset."""

    def __init__(self, distance_data_dir, agent_ids, is_collecting_data):
        self.distance_data_dir, self.all_agent_ids = distance_data_dir, agent_ids
        self.is_collecting_data = is_collecting_data
        self.distance_history = None
        for agent_id in agent_ids + ["cgd"]:
            (Path(distance_data_dir) / agent_id).mkdir(parents=True, exist_ok=True)

    def reset(self):
        if self.distance_history is not None and not self.is_collecting_data:
            self._save_agent_histories(self.distance_history)
        if self.distance_data_dir is not None:
            self.distance_history = {_id: [] for _id in self.all_agent_ids}

    def step(self, terminated, truncated, device_state_info, cgd_full, num_gates):
        if (terminated or truncated) and self.distance_history is not None:
            self._save_agent_histories(self.distance_history)
            if self.is_collecting_data:
                self._save_cgd_matrix(cgd_full)
            self.distance_history = {_id: [] for _id in self.all_agent_ids}
        for idx in range(num_gates):
            gt = device_state_info["gate_ground_truth"][idx]; cv = device_state_info["current_gate_voltages"][idx]
            self.distance_history[f"plunger_{idx}"].append(cv - gt)
        for idx in range(num_gates - 1):
            gt = device_state_info["barrier_ground_truth"][idx]; cv = device_state_info["current_barrier_voltages"][idx]
            self.distance_history[f"barrier_{idx}"].append(cv - gt)

    def _next(self, folder, ext):
        existing_files = glob.glob(str(folder / f"*{ext}"))
        if len(existing_files) == 0:
            next_count = 1
        else:
            next_count = max(int(Path(f).stem.split('_')[0]) for f in existing_files) + 1
        return folder / f"{next_count:04d}_{random.randint(0, 999999):06d}{ext}"

    def _save_agent_histories(self, history):
        for agent_id in self.all_agent_ids:
            np.save(self._next(Path(self.distance_data_dir) / agent_id, ".npy"), np.array(history[agent_id]))

    def _save_cgd_matrix(self, cgd):
        with open(self._next(Path(self.distance_data_dir) / "cgd", ".json"), "w") as f:
            json.dump(np.array(cgd).tolist(), f)


def _ids(N):
    return [f"plunger_{i}" for i in range(N)] + [f"barrier_{j}" for j in range(N - 1)]


def _files(d, folder, ext):
    """count -> loaded content of <d>/<folder>/*.<ext>, after checking the name pattern."""
    out = {}
    for f in sorted(glob.glob(os.path.join(d, folder, "*" + ext))):
        stem = os.path.basename(f)[:-len(ext)]
        count, rnd = stem.split("_")
        assert len(count) == 4 and len(rnd) == 6 and count.isdigit() and rnd.isdigit(), f
        assert int(count) not in out, f
        out[int(count)] = np.load(f) if ext == ".npy" else np.array(json.load(open(f)))
    return out


def _actions(rng, B, N):
    ids = _ids(N)
    return [{a: rng.uniform(-1, 1, 1).astype(np.float32) for a in ids} for _ in range(B)]


def _stagger(env, steps):
    env.vec._steps_host[:] = steps


B, N, R, MAX = 4, 3, 5, 3
STAGGER = [0, 2, 0, 2]           # envs 1 and 3 end at steps 1, 4, 7; envs 0 and 2 at steps 3, 6


@pytest.mark.parametrize("collecting", [False, True])
def test_distance_logs_follow_the_reference_call_for_call(tmp_path, collecting):
    ours, ref_dir = tmp_path / "ours", tmp_path / "ref"
    for d in (ours, ref_dir):                                               # counts continue from existing files
        for a in _ids(N):
            (d / a).mkdir(parents=True)
            np.save(d / a / "0041_000123.npy", np.zeros(1))
            np.save(d / a / "0007_000001.npy", np.zeros(1))
    env = BatchedMultiAgentEnv(backend=FakeVec(B, N, R, MAX), distance_data_dir=str(ours),
                               is_collecting_data=collecting)
    refs = [ReferenceLog(str(ref_dir), _ids(N), collecting) for _ in range(B)]
    for b in range(B):
        env.views[b].reset()
        refs[b].reset()
    _stagger(env, STAGGER)
    rng = np.random.default_rng(3)
    for t in range(8):
        acts = _actions(rng, B, N)
        for b in range(B):
            env.views[b].stage(acts[b])
        res = [env.views[b].collect() for b in range(B)]
        tr = env.vec.trace[-1]
        for b in range(B):
            assert res[b][3]["__all__"] == bool(tr["truncated"][b])
            refs[b].step(False, bool(tr["truncated"][b]), {k: v[b] for k, v in tr["ds"].items()}, tr["cgd"][b], N)
        for b in range(B):
            if tr["truncated"][b]:
                env.views[b].reset()
                refs[b].reset()
    lengths = []
    for a in _ids(N):
        got, want = _files(ours, a, ".npy"), _files(ref_dir, a, ".npy")
        assert sorted(got) == sorted(want) and len(got) > 4, a
        for c in want:
            assert got[c].dtype == np.float64 and np.array_equal(got[c], want[c]), (a, c)
        assert min(c for c in got if c > 41) == 42
        lengths.append([len(got[c]) for c in sorted(got) if c > 41])
    assert all(ln == lengths[0] for ln in lengths)                         # all agents of an episode share a count
    assert MAX - 1 in lengths[0] and (1 in lengths[0]) != collecting       # full episodes; the reset's one-entry file
    got, want = _files(ours, "cgd", ".json"), _files(ref_dir, "cgd", ".json")
    assert sorted(got) == sorted(want)
    assert (len(got) > 0) == collecting
    for c in want:
        assert np.array_equal(got[c], want[c])


def test_vector_step_saves_only_at_truncation(tmp_path):
    env = BatchedMultiAgentEnv(backend=FakeVec(2, N, R, MAX), distance_data_dir=str(tmp_path))
    env.reset()
    rng = np.random.default_rng(0)
    for t in range(2 * MAX):
        env.step(_actions(rng, 2, N))
    lens = [len(v) for _, v in sorted(_files(tmp_path, "barrier_0", ".npy").items())]
    # first episode: max_steps - 1 entries; then the final distance of the old device runs on into the next history
    assert lens == [MAX - 1, MAX - 1, MAX, MAX]


def _run(mode, steps=7, zero_copy=False, **kw):
    env = BatchedMultiAgentEnv(backend=FakeVec(B, N, R, MAX), final_observation=mode, zero_copy=zero_copy,
                               return_global_state=True, **kw)
    out = [env.reset()]
    _stagger(env, STAGGER)
    rng = np.random.default_rng(5)
    for t in range(steps):
        out.append(env.step(_actions(rng, B, N)))
    return env, out


def _same(x, y):
    if isinstance(x, dict):
        return isinstance(y, dict) and x.keys() == y.keys() and all(_same(x[k], y[k]) for k in x)
    if isinstance(x, (list, tuple)):
        return len(x) == len(y) and all(_same(a, b) for a, b in zip(x, y))
    return np.array_equal(np.asarray(x), np.asarray(y)) and np.asarray(x).dtype == np.asarray(y).dtype


def _agent_obs(host, b):
    """Per-agent (image, voltage) arrays of env b in a trace entry."""
    p, br, v = host["plunger_images"][b], host["barrier_images"][b], host["voltages"][b]
    out = {f"plunger_{i}": (p[i], v[i:i + 1]) for i in range(N)}
    out.update({f"barrier_{j}": (br[j], v[N + j:N + j + 1]) for j in range(N - 1)})
    return out


def test_default_mode_is_todays_output():
    env0, plain = _run(None)
    env_plain = BatchedMultiAgentEnv(backend=FakeVec(B, N, R, MAX), return_global_state=True)
    out = [env_plain.reset()]
    _stagger(env_plain, STAGGER)
    rng = np.random.default_rng(5)
    for t in range(7):
        out.append(env_plain.step(_actions(rng, B, N)))
    assert _same(plain, out)
    assert all(c == dict(auto_reset=True, keep_final=False) for c in env_plain.vec.step_calls)
    assert env0.vec.step_calls == env_plain.vec.step_calls


def test_info_mode_adds_final_keys_on_truncated_envs_only():
    _, base = _run(None)
    env, info_run = _run("info")
    envz, zero_run = _run("info", zero_copy=True)      # read after the last step: final arrays must have survived it
    seen = 0
    for t in range(1, len(info_run)):
        obs, rews, terms, truncs, infos = info_run[t]
        zinfos = zero_run[t][4]
        bobs, brews, _, btruncs, binfos = base[t]
        tr = env.vec.trace[t - 1]
        assert _same(obs, bobs) and _same(rews, brews) and _same(truncs, btruncs)
        for b in range(B):
            done = bool(tr["truncated"][b])
            ref = _agent_obs(tr["host"], b)
            for i, a in enumerate(_ids(N)):
                assert ("final_observation" in infos[b][a]) == done and ("final_info" in infos[b][a]) == done
                rest = {k: v for k, v in infos[b][a].items() if k not in ("final_observation", "final_info")}
                assert _same(rest, binfos[b][a])
                if not done:
                    continue
                seen += 1
                fo = infos[b][a]["final_observation"]
                assert np.array_equal(fo["image"], ref[a][0]) and np.array_equal(fo["voltage"], ref[a][1])
                assert np.array_equal(fo["global_image"], tr["host"]["global_image"][b])
                kind, k = ("gate", i) if i < N else ("barrier", i - N)
                assert infos[b][a]["final_info"] == {"ground_truth": tr["ds"][f"{kind}_ground_truth"][b][k],
                                                     "current_voltage": tr["ds"][f"current_{kind}_voltages"][b][k]}
                assert _same(zinfos[b][a]["final_observation"], fo)
    assert seen > 0


def test_step_mode_returns_the_old_episode_and_reset_the_new_one():
    _, base = _run(None)
    env = BatchedMultiAgentEnv(backend=FakeVec(B, N, R, MAX), final_observation="step", return_global_state=True)
    views = env.views
    for b in range(B):
        views[b].reset()
    _stagger(env, STAGGER)
    rng = np.random.default_rng(5)
    seen = 0
    for t in range(1, 8):
        acts = _actions(rng, B, N)
        for b in range(B):
            views[b].stage(acts[b])
        launches = env.launches
        tr = env.vec.trace[-1]
        bobs, brews, _, btruncs, binfos = base[t]
        for b in range(B):
            obs, rew, term, trunc, info = views[b].collect()
            assert _same(rew, brews[b]) and _same(trunc, btruncs[b])
            if not tr["truncated"][b]:
                assert _same(obs, bobs[b]) and _same(info, binfos[b])
                continue
            seen += 1
            ref = _agent_obs(tr["host"], b)
            for i, a in enumerate(_ids(N)):
                assert np.array_equal(obs[a]["image"], ref[a][0]) and np.array_equal(obs[a]["voltage"], ref[a][1])
                kind, k = ("gate", i) if i < N else ("barrier", i - N)
                assert info[a] == {"ground_truth": tr["ds"][f"{kind}_ground_truth"][b][k],
                                   "current_voltage": tr["ds"][f"current_{kind}_voltages"][b][k]}
            o2, i2 = views[b].reset()                      # the new episode's first observation, as mode None hands out
            assert _same(o2, bobs[b])
            assert i2["plunger_0"]["current_device_state"]["steps"] == 0
            assert env.launches == launches
    assert seen > 0


def test_bad_mode_is_refused():
    with pytest.raises(ValueError, match="final_observation"):
        BatchedMultiAgentEnv(backend=FakeVec(2, N, R, MAX), final_observation="obs")
    with pytest.raises(ValueError, match="final_observation"):
        MultiAgentEnvWrapper(final_observation=True, base_env_class=object)


class _ForeignEnv:
    """A gym-style base env of the reference's `base_env_class` hook: nothing resets it but reset()."""

    def __init__(self, training=True, capacitance_model_checkpoint=None, max_steps=MAX):
        from qadapt_hip import spaces
        self.num_dots, self.use_barriers, self.max_steps = N, True, max_steps
        self.observation_space = {"image": spaces.Box(low=0.0, high=1.0, shape=(R, R, N - 1), dtype=np.float32)}
        self.action_space = None
        self.episode = 0
        self.array = type("A", (), {})()
        self.array.model = type("M", (), {})()

    def _obs(self):
        rng = np.random.default_rng([self.episode, self.t])
        return {"image": rng.random((R, R, N - 1)).astype(np.float32),
                "obs_gate_voltages": rng.uniform(-1, 1, N).astype(np.float32),
                "obs_barrier_voltages": rng.uniform(-1, 1, N - 1).astype(np.float32)}

    def _info(self):
        return {"current_device_state": {"gate_ground_truth": np.full(N, self.episode, np.float32),
                                         "barrier_ground_truth": np.full(N - 1, -0.5, np.float32),
                                         "current_gate_voltages": self.v[:N].copy(),
                                         "current_barrier_voltages": self.v[N:].copy()}}

    def reset(self, seed=None, options=None):
        self.episode += 1
        self.t = 0
        self.v = np.zeros(2 * N - 1)
        self.array.model.cgd_full = np.full((N + 1, 2 * N), float(self.episode))
        return self._obs(), self._info()

    def step(self, action):
        self.t += 1
        self.v = np.concatenate([action["action_gate_voltages"], action["action_barrier_voltages"]]).astype(np.float64) * 5
        rew = {"gates": np.zeros(N), "barriers": np.zeros(N - 1)}
        return self._obs(), rew, False, self.t >= self.max_steps, self._info()


def test_wrapper_over_a_foreign_base_env(tmp_path):
    """_SingleEnvBackend: the step's own info is the final one; logs and both modes work there too."""
    w = MultiAgentEnvWrapper(return_voltage=True, base_env_class=_ForeignEnv, final_observation="info",
                             distance_data_dir=str(tmp_path / "ours"), is_collecting_data=True)
    ref = ReferenceLog(str(tmp_path / "ref"), _ids(N), True)
    w.reset(); ref.reset()
    rng = np.random.default_rng(1)
    for t in range(2 * MAX):
        acts = _actions(rng, 1, N)[0]
        obs, rew, term, trunc, infos = w.step(acts)
        ds = w.base_env._info()["current_device_state"]
        ref.step(False, trunc["__all__"], ds, w.base_env.array.model.cgd_full, N)
        if trunc["__all__"]:
            fo = infos["plunger_1"]["final_observation"]
            assert np.array_equal(fo["image"], obs["plunger_1"]["image"]) and fo["image"] is not obs["plunger_1"]["image"]
            assert infos["barrier_0"]["final_info"] == {"ground_truth": np.float32(-0.5),
                                                        "current_voltage": ds["current_barrier_voltages"][0]}
            w.reset(); ref.reset()
        else:
            assert "final_observation" not in infos["plunger_1"]
    for a in _ids(N):
        got, want = _files(tmp_path / "ours", a, ".npy"), _files(tmp_path / "ref", a, ".npy")
        assert sorted(got) == sorted(want) == [1, 2]
        assert all(np.array_equal(got[c], want[c]) for c in want)
    got, want = _files(tmp_path / "ours", "cgd", ".json"), _files(tmp_path / "ref", "cgd", ".json")
    assert sorted(got) == sorted(want) == [1, 2] and all(np.array_equal(got[c], want[c]) for c in want)
