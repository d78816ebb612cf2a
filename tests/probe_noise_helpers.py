"""Scenes of the noisy-probe tests (tests/test_gpu_probe_noise.py), built on the CPU alone: devices from the product's host
sampler, states placed by hand, and the oracle's answers (oracle/qd_oracle_c.py, oracle/qd_noise_oracle.py).  Everything
a test demands of a scene (latched pixels, a replaced channel, how many pixels the float64 ground vector does not resolve)
is decided here, without a GPU, and asserted by the test before it renders anything."""
import functools
import types

import numpy as np

import helpers as H
import qd_noise_oracle as NO
import qd_oracle_c as OC
from qadapt_hip import device_model as DM
from qadapt_hip.layout import layout

ALL = ("sensor", "radial", "latch")
# the scene of tests/test_gpu_noise.py::test_noisy_observation_matches_numpy_restatement: three 4-dot devices of seed 99 with
# global env ids 40..42 at 24x24, env 0 near its ground truth, env 1 in the radial ramp, env 2 beyond full_noise_distance
B, N, R, SEED, OFF = 3, 4, 24, 99, 40
OFFSETS = (1.5, 27.0, 70.0)


def sampled(n_dot, seed, first_id, count):
    """Parameter and state blocks as VecQuantumDeviceEnv(count, seed=seed, env_id_offset=first_id).load_new_devices(seed=seed)
    samples them."""
    q, e = H.configs()
    s = DM.DeviceSampler(n_dot, q, e)
    return s.build(np.stack([np.random.Generator(np.random.PCG64(seed + first_id + k)).random(s.n_draws) for k in range(count)]))


@functools.lru_cache(maxsize=None)
def noise_scene():
    """(params (B, L.size), state (B, L.s_size)): gates OFFSETS[e] volts off the ground truth, barriers at theirs, and a
    virtual gate matrix that is not the identity."""
    L, G = layout(N), N + 1
    eb = sampled(N, SEED, OFF, B)
    st = eb.state.copy()
    rng = np.random.default_rng(4099)
    for e, off in enumerate(OFFSETS):
        st[e, L.s_gate_v:L.s_gate_v + N] = st[e, L.s_gate_gt:L.s_gate_gt + N] + off
        st[e, L.s_barrier_v:L.s_barrier_v + N - 1] = st[e, L.s_barrier_gt:L.s_barrier_gt + N - 1]
        st[e, L.s_vgm:L.s_vgm + G * G] += rng.normal(0, 0.02, G * G)
    return eb.params.copy(), st


def noise_params(par, L):
    return dict(white_amp=par[L.noise + 0], tel_p01=par[L.noise + 1], tel_p10=par[L.noise + 2], tel_amp=par[L.noise + 3],
                zero_radius=par[L.noise + 4], ramp_distance=par[L.noise + 5],
                full_noise_distance=par[L.noise + 6] if par[L.noise + 6] > 0 else None, max_amplitude=par[L.noise + 7])


def load_scene(env, params, state):
    """The scene as the handle's devices and states (Kalman blocks stay as qd_create left them)."""
    eb = env.load_new_devices(seed=env.seed)
    assert np.array_equal(eb.params, params), "the handle samples other devices than the scene's"
    st, steps = env.get_state()
    k = env.L.s_kmean
    st[:, :k] = state[:, :k]
    env.set_state(st, steps)
    return st


@functools.lru_cache(maxsize=None)
def noise_reference(stream_base, serial, flags=ALL):
    """Query q = env q of noise_scene() at its own voltages, drawn from NO.Stream(SEED, stream_base + q, serial): per query
    and channel dict(z (P,), occ (P, N), ok (P,) where tc < 1e6, replaced, latched pixels)."""
    params, state = noise_scene()
    L = layout(N)
    out = []
    for q in range(B):
        par = params[q]
        dev, sv = H.dev_view(N, par), H.state_view(N, state[q])
        s = NO.Stream(SEED, stream_base + q, serial)
        nz = noise_params(par, L)
        p_leads = par[L.pleads:L.pleads + N]; p_inter = par[L.pinter:L.pinter + N * N].reshape(N, N)
        chans = []
        for ch in range(N - 1):
            det = OC.csd_channel(dev, sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, sv.barrier_v, dev.window, ch, R)
            z, used = NO.observe_channel(dev, nz, s, ch, R, sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, sv.barrier_v,
                                         dev.window, sv.gate_gt, det["occ"], set(flags), p_leads, p_inter)
            rep = "radial" in flags and NO.radial_replaced(sv.gate_v[ch], sv.gate_v[ch + 1], sv.gate_gt[ch], sv.gate_gt[ch + 1],
                                                           nz["full_noise_distance"])
            chans.append(types.SimpleNamespace(z=z, occ=used, ok=det["tc"].max(axis=1) < 1e6, replaced=bool(rep),
                                               latched=0 if rep else int((used != det["occ"]).any(axis=1).sum())))
        out.append(chans)
    return out


# ------------------------------------------------------------------ occupations without noise
OCC_CASES = {4: 6104, 8: 6108}                       # dots -> seed of the two devices ("near" and "far" from the ground truth)


@functools.lru_cache(maxsize=None)
def occ_scene(n_dot, Rr=16):
    """Two devices of seed OCC_CASES[n_dot], placed "near" and "far" (helpers.place); per env and channel the oracle's
    occupations and the relative gap of its 32-state Hamiltonian (helpers.pixel_spectrum on the oracle's own states)."""
    seed = OCC_CASES[n_dot]
    eb = sampled(n_dot, seed, 0, 2)
    rng = np.random.default_rng(seed)
    st = np.stack([H.place(n_dot, eb.state[e], mode, rng) for e, mode in enumerate(("near", "far"))])
    ref = []
    for e in range(2):
        dev, sv = H.dev_view(n_dot, eb.params[e]), H.state_view(n_dot, st[e])
        chans = []
        for ch in range(n_dot - 1):
            det = OC.csd_channel(dev, sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, sv.barrier_v, dev.window, ch, Rr)
            sp = H.pixel_spectrum(dev, sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, sv.barrier_v, dev.window, ch, Rr,
                                  states=det["states"])
            chans.append(types.SimpleNamespace(occ=det["occ"], rel_gap=sp["rel_gap"]))
        ref.append(chans)
    return eb.params.copy(), st, ref


@functools.lru_cache(maxsize=None)
def full_scene(Rr=8, m=4, seed=6203):
    """(3 dots, m carriers) full space: two devices near and far; per env and channel the relative gap of the whole M x M
    Hamiltonian (dense eigvalsh, as tests/test_gpu_full_charge_space.py forms it)."""
    from test_full_charge_space import full_hamiltonian, full_states, pixel_inputs
    n_dot = 3
    eb = sampled(n_dot, seed, 0, 2)
    rng = np.random.default_rng(seed)
    st = np.stack([H.place(n_dot, eb.state[e], mode, rng) for e, mode in enumerate(("near", "far"))])
    states = full_states(n_dot, m)
    gaps = []
    for e in range(2):
        dev, sv = H.dev_view(n_dot, eb.params[e]), H.state_view(n_dot, st[e])
        row = []
        for ch in range(n_dot - 1):
            F, tc, _, _ = pixel_inputs(dev, sv, ch, Rr, states, vc=dev.vc)
            Hm = full_hamiltonian(F, tc, states)
            w = np.linalg.eigvalsh(Hm)
            row.append((w[:, 1] - w[:, 0]) / np.abs(Hm).sum(axis=2).max(axis=1))
        gaps.append(row)
    return eb.params.copy(), st, gaps
