"""Handle life cycle on the MI355X (run with -m gpu): three handles built, driven through every lazily allocated or growing
buffer of qd_api.hip and destroyed in one process -- the staging ring at its minimum and grown, the probe scratch over two
launch chunks, the compose scratch growing once, the point scratch over several launches -- must return the same bits,
and a scratch that is used again must give what it gave when it was fresh."""
import numpy as np
import pytest
import torch
import yaml

from qadapt_hip import device_model as DM
from qadapt_hip.layout import layout

pytestmark = pytest.mark.gpu

N, R, B, SEED = 4, 8, 72, 8812          # 72 envs: above the ring's 64-row minimum and above the 64 point slots
C, P = N - 1, R * R


def _physical(L, par, st, virt):
    """virtual plunger voltages (n, N) with the sensor at its ground truth -> physical gate voltages (n, N+1)"""
    G = N + 1
    vgm = st[L.s_vgm:L.s_vgm + G * G].reshape(G, G)
    full = np.concatenate([virt, np.full((virt.shape[0], 1), st[L.s_sensor_gt])], axis=1)
    return full @ vgm.T + par[L.origin:L.origin + G]


def _stateless(env, st, rng_seed):
    """probe with 100 queries (two launch chunks, 72 + 28), the three composites, points in groups of 1 and C P + 1"""
    L, out = layout(N), {}
    rng = np.random.default_rng(rng_seed)
    ids = np.arange(100) % B
    gv = st[ids, L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-3, 3, (100, N))
    bv = st[ids, L.s_barrier_gt:L.s_barrier_gt + C] + rng.uniform(-3, 3, (100, C))
    pr = env.probe(ids, gv, bv, sensor_voltage=st[ids, L.s_sensor_gt], normalised=True)
    for k in ("raw", "image", "plohi"):
        out["probe_" + k] = pr[k].cpu().numpy()
    for name, n, mode in (("1x1_global", 1, "global"), ("2x2_global", 2, "global"), ("2x2_per_scan", 2, "per_scan")):
        comp, plohi = env.compose(pr["raw"][:n * n], n, n, channel=1, mode=mode)
        out["compose_" + name] = comp.cpu().numpy()
        out["compose_" + name + "_plohi"] = plohi.cpu().numpy()
    envs, counts = [3, 70], [1, C * P + 1]
    vg = [_physical(L, env._params_host[e], st[e], st[e, L.s_gate_gt:L.s_gate_gt + N] + rng.uniform(-3, 3, (m, N)))
          for e, m in zip(envs, counts)]
    vb = [st[e, L.s_barrier_gt:L.s_barrier_gt + C] + rng.uniform(-3, 3, (m, C)) for e, m in zip(envs, counts)]
    pt = env.eval_points(envs, vg, vb)
    for g in range(2):
        out[f"points_signal_{g}"] = pt["signal"][g].cpu().numpy()
        out[f"points_occupations_{g}"] = pt["occupations"][g].cpu().numpy()
    return out


def _cycle(config_path):
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    out = {}
    env = VecQuantumDeviceEnv(B, num_dots=N, resolution=R, seed=SEED, config_path=config_path)
    assert env.chunk_envs() == B                                   # one lane, one launch chunk of 72
    obs = env.reset(env_ids=[0])                                   # staging ring at its minimum of 64 rows
    out["reset_one_image"] = obs["image"][0].cpu().numpy()
    obs = env.reset()                                              # 72 rows: the ring grows
    for k, v in obs.items():
        out["reset_" + k] = v.cpu().numpy()
    st, steps = env.get_state()
    first = _stateless(env, st, SEED + 1)
    out.update(first)
    act = torch.as_tensor(np.random.default_rng(SEED + 2).uniform(-1, 1, (B, 2 * N - 1)).astype(np.float32)).cuda()
    obs, rew, term, trunc = env.step(act)
    for k, v in obs.items():
        out["step_" + k] = v.cpu().numpy()
    out["step_rewards"], out["step_truncated"] = rew.cpu().numpy(), trunc.cpu().numpy()
    out["raw"], out["plohi"] = env.raw()
    out["state"], out["steps"] = env.get_state()
    # the scratch sets used a second time, on the state of the first time
    env.set_state(st, steps)
    again = _stateless(env, st, SEED + 1)
    env.close()
    return out, first, again


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.dtype, a.shape, a.tobytes()


def test_three_handles_in_one_process_return_the_same_bits(tmp_path):
    cfg = DM.load_yaml(None, "env_config.yaml")
    cfg["capacitance_model"]["update_method"] = None               # deterministic physics, no CNN in the loop
    path = tmp_path / "env.yaml"
    path.write_text(yaml.safe_dump(cfg))
    ref, first, again = _cycle(str(path))
    assert first and set(first) == set(again)
    for k in first:
        assert _bits(first[k]) == _bits(again[k]), f"re-used scratch differs from a fresh one: {k}"
    assert ref["probe_raw"].shape == (100, C, R, R) and ref["points_signal_1"].shape == (C * P + 1,)
    assert np.isfinite(ref["probe_raw"]).all() and np.isfinite(ref["points_signal_1"]).all() and ref["raw"].any()
    for cycle in (2, 3):
        out, first, again = _cycle(str(path))
        assert set(out) == set(ref)
        for k in ref:
            assert _bits(out[k]) == _bits(ref[k]), f"cycle {cycle} differs from cycle 1: {k}"
        for k in first:
            assert _bits(first[k]) == _bits(again[k]), f"cycle {cycle}: re-used scratch differs from a fresh one: {k}"
