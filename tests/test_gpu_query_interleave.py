"""Query types interleaved on one handle (run with -m gpu): noisy probe, noisy axis scan, point evaluation, plain probe, plain
scan and a step share the stateless-query runner, the launchers and lane 0's scratch, each with a buffer view of its own shape.
Every call must return what the same call returns alone on a fresh handle: nothing one query type leaves behind (a view
field, a scratch pointer, a noise word) may reach the next."""
import numpy as np
import pytest
import yaml

import helpers as H
from qadapt_hip import device_model as DM
from qadapt_hip.layout import layout

pytestmark = pytest.mark.gpu

B, CHUNK, NQ = 3, 2, 5                       # five queries in launch chunks of two slots: three chunks, the last one short
NOISE = ("sensor", "latch")


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _env(tmp_path, N, R, K, seed):
    """a handle with sensor noise and latching, its three devices placed near, mid-way and far from their ground truths"""
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    cfg = DM.load_yaml(None, "env_config.yaml")
    cfg["capacitance_model"]["update_method"] = None          # deterministic physics, no CNN in the loop
    p = tmp_path / "env.yaml"
    p.write_text(yaml.safe_dump(cfg))
    env = VecQuantumDeviceEnv(B, num_dots=N, resolution=R, seed=seed, config_path=str(p), env_chunk=CHUNK, noise=NOISE,
                              num_charge_states=K)
    env.reset(seed=seed)
    st, steps = env.get_state()
    rng = np.random.default_rng(seed)
    for e, mode in enumerate(("near", "mid", "far")):
        st[e] = H.place(N, st[e], mode, rng)
    env.set_state(st, steps)
    return env, st


def _calls(N, st, axes):
    """the six calls, each env -> dict of host arrays; the inputs depend on the placed state `st` alone"""
    L, C = layout(N), N - 1
    rng = np.random.default_rng(99)
    ids = np.array([0, 1, 2, 1, 0], np.int32)
    gv = st[ids, L.s_gate_v:L.s_gate_v + N] + rng.uniform(-1.0, 1.0, (NQ, N))
    bv = st[ids, L.s_barrier_v:L.s_barrier_v + C] + rng.uniform(-0.5, 0.5, (NQ, C))
    sv = st[ids, L.s_sensor_gt] + rng.uniform(-0.3, 0.3, NQ)
    centre = np.concatenate([gv, sv[:, None], bv], axis=1)[:, list(axes)]             # (NQ, 2): the swept controls' own values
    xr = np.stack([centre[:, 0] - rng.uniform(0.5, 2.0, NQ), centre[:, 0] + rng.uniform(2.0, 4.0, NQ)], axis=1)
    yr = np.stack([centre[:, 1] + rng.uniform(2.0, 4.0, NQ), centre[:, 1] - rng.uniform(0.5, 2.0, NQ)], axis=1)   # downwards
    pts = np.array([2, 0, 1], np.int32)
    m = 7
    sp = st[pts][:, None, :]                                                          # (3, 1, state block)
    vg = np.concatenate([sp[..., L.s_gate_v:L.s_gate_v + N] + rng.uniform(-2.0, 2.0, (3, m, N)),
                         sp[..., L.s_sensor_gt:L.s_sensor_gt + 1] + rng.uniform(-0.3, 0.3, (3, m, 1))], axis=2)
    vb = sp[..., L.s_barrier_v:L.s_barrier_v + C] + rng.uniform(-1.0, 1.0, (3, m, C))
    act = rng.uniform(-1.0, 1.0, (B, 2 * N - 1)).astype(np.float32)
    noisy = dict(noise=NOISE, occupations=True, serial=7, stream_base=11)

    def step(env):
        import torch
        obs, rew, term, trunc = env.step(torch.as_tensor(act, device=env.device))
        out = _np(obs)
        out.update(rewards=rew.cpu().numpy(), terminated=term.cpu().numpy(), truncated=trunc.cpu().numpy())
        out["state"], out["steps"] = env.get_state()
        out["raw"], out["plohi"] = env.raw()
        return out

    return [lambda env: _np(env.probe(ids, gv, bv, sensor_voltage=sv, normalised=True, **noisy)),
            lambda env: _np(env.scan2d(ids, axes[0], axes[1], xr, yr, gv, bv, sensor_voltage=sv, normalised=True, **noisy)),
            lambda env: _np(env.eval_points(pts, vg, vb)),
            lambda env: _np(env.probe(ids, gv, bv, sensor_voltage=sv, normalised=True)),
            lambda env: _np(env.scan2d(ids, axes[0], axes[1], xr, yr, gv, bv, sensor_voltage=sv, normalised=True)),
            step]


# N = 4, R = 32: the tile search runs (K = 8: the smallest kept set), non-adjacent plungers.  N = 2, R = 8: the per-pixel
# search, and C = 1, where probe and scan select the same latching and sensor instantiations; plunger against barrier.
@pytest.mark.parametrize("N,R,K,axes", [(4, 32, 8, (0, 2)), (2, 8, None, (0, 3))])
def test_interleaved_calls_equal_calls_alone(tmp_path, N, R, K, axes):
    seed = 7300 + N
    env, st = _env(tmp_path, N, R, K, seed)
    assert env.chunk_envs() == CHUNK
    calls = _calls(N, st, axes)
    got = [call(env) for call in calls]
    env.close()
    # the sequence is worth its name: signals with structure, and the noise stages really ran on calls 1 and 2
    for k in (0, 1, 3, 4):
        assert np.isfinite(got[k]["raw"]).all() and np.ptp(got[k]["raw"]) > 0, k
    assert not np.array_equal(got[0]["raw"], got[3]["raw"]) and not np.array_equal(got[1]["raw"], got[4]["raw"])
    assert got[0]["raw"].shape == (NQ, N - 1, R, R) and got[1]["raw"].shape == (NQ, R, R)
    for k, call in enumerate(calls):
        # the queries change nothing of the episodes, so the interleaved env reaches every call in the state a fresh one has
        alone, st_alone = _env(tmp_path, N, R, K, seed)
        assert np.array_equal(st_alone, st)
        want = call(alone)
        alone.close()
        assert want.keys() == got[k].keys(), k
        for name in want:
            assert np.array_equal(got[k][name], want[name], equal_nan=True), (k, name)
