"""The scenes of the mixed latched batch (BASELINE config 5 in miniature), shared by the no-GPU tier
(tests/test_mixed_cases_cpu.py) and the GPU tier (tests/test_gpu_mixed_latched.py).

Whole job: counts {2: 5, 4: 5, 6: 5, 8: 5}, global env ids 0..19 bucket after bucket; R = 20 (the image edge cuts the 8 x 8
tiles, P = 400); env_chunk = 2 (5 envs are three chunks); T = 4 steps, numbered 0..3; the checks run after steps 2 and 3.

Scene A (deterministic state: `capacitance_model.update_method: null`, so nothing rewrites the VGM after an image).  Roles by
the env's index in its WHOLE bucket, whatever the shard:
    0  near (gates +-3, barriers +-3, helpers.place's "near")
    1  near, step counter preset so that it truncates at step 2
    2  mid (gates +-10, barriers +-6)
    3  a uniform random action (far regime), truncates at step 3
    4  near, truncates at step 2: the partial reset of step 2 has two ids
Every step every env gets the target ground truth + offset, turned into an action by inverting the oracle's rescale on the
device's own range (formed in float32 by the sampler, as the reference forms it) and clipped to [-1, 1].

`trajectory(N)` rebuilds the whole state history of a bucket on the host: devices from DeviceSampler draws of PCG64(SEED +
global id) (the first at reset, the next at each automatic reset), voltages from the oracle's action mapping, rewards from
the oracle's reward, observation numbers from the handle's rule (one per observe: the reset, every step, every partial
reset).  `frame(N, t, i)` is the oracle's view of what env i of the bucket shows after step t: its C-oracle channels, the
relative gaps and the latching walk of the restatement on the oracle's occupations.
"""
import os
import tempfile
import types

import numpy as np
import yaml

import helpers as H
import qd_noise_oracle as NO
import qd_oracle as O
import qd_oracle_c as OC
from qadapt_hip import device_model as DM
from qadapt_hip import shard
from qadapt_hip.layout import layout

COUNTS = {2: 5, 4: 5, 6: 5, 8: 5}
R = 20
ENV_CHUNK = 2
T = 4
SEED = 1                                     # the first of SEEDS_TRIED for which the conditions of the CPU tier hold (0 fails: see DESIGN.md)
SEEDS_TRIED = (0, 1)
CHECK_STEPS = (2, 3)
ROLES = ("near", "near", "mid", "far", "near")
SPAN = {"near": (3.0, 3.0), "mid": (10.0, 6.0)}          # helpers.place
TRUNCATE_AT = {1: 2, 3: 3, 4: 2}
VARIANTS = {"latch": ("latch",), "all": ("sensor", "radial", "latch")}
NEAR_EXEMPT_MAX, MID_EXEMPT_MAX = 0.10, 0.25


def env_config():
    cfg = DM.load_yaml(None, "env_config.yaml")
    cfg["capacitance_model"]["update_method"] = None          # deterministic physics, no CNN in the loop
    return cfg


def write_env_config(directory=None):
    """The env config of scene A as a file (VecQuantumDeviceEnv takes a path)."""
    fd, path = tempfile.mkstemp(suffix=".yaml", prefix="mixed_scene_a_", dir=directory)
    with os.fdopen(fd, "w") as f:
        f.write(yaml.safe_dump(env_config()))
    return path


def bucket_first(N):
    return shard.shard_mixed(COUNTS, 0, 1, R)[N][0]


def compared(t):
    """Bucket indices compared after step t: near env 0 (never reset), the envs reset in step t, the mid env 2."""
    return [0] + sorted(i for i, s in TRUNCATE_AT.items() if s == t) + [2]


def preset_steps(max_steps, first=0, count=None):
    """Step counters written after reset(): env i truncates at step TRUNCATE_AT[i] (steps count from 0)."""
    n = max(COUNTS.values()) if count is None else count
    out = np.zeros(n, np.int32)
    for k in range(n):
        i = first + k
        if i in TRUNCATE_AT:
            out[k] = max_steps - (TRUNCATE_AT[i] + 1)
    return out


def inverse_rescale(target, lo, hi):
    """The float32 action whose oracle rescale (O.rescale) lands closest to `target`, clipped to [-1, 1]."""
    return np.clip(2.0 * (target - lo) / (hi - lo) - 1.0, -1.0, 1.0).astype(np.float32)


_TRAJ = {}


def trajectory(N, seed=None):
    """The host-side history of bucket N of scene A.  Arrays over (step t, bucket index i):
      actions (T, n, 2N-1) float32; rewards (T, n, 2N-1); truncated (T, n) bool
      params (T, n, L.size), state (T, n, L.s_kmean), steps (T, n): what the handle holds AFTER step t (a reset env: its new
          device at its start voltages) -- the state the images it shows were rendered from
      serial (T, n): the observation number of the image env i shows after step t; ck_serial (T,): the handle's counter
      reset0: (params, state) after reset()."""
    seed = SEED if seed is None else seed
    if (N, seed) in _TRAJ:
        return _TRAJ[(N, seed)]
    n, first, L = COUNTS[N], bucket_first(N), layout(N)
    cfg = env_config()
    max_steps = int(cfg["simulator"]["max_steps"])
    sampler = DM.DeviceSampler(N, DM.load_yaml(None, "qarray_config.yaml"), cfg)
    rngs = [np.random.Generator(np.random.PCG64(seed + first + i)) for i in range(n)]
    design = [np.random.default_rng([seed, first + i, 77]) for i in range(n)]

    def draw(i):
        eb = sampler.build(rngs[i].random(sampler.n_draws)[None])
        return eb.params[0].copy(), eb.state[0, :L.s_kmean].copy()

    par = np.zeros((n, L.size)); st = np.zeros((n, L.s_kmean))
    for i in range(n):
        par[i], st[i] = draw(i)
    tr = types.SimpleNamespace(N=N, n=n, first=first, L=L, max_steps=max_steps, seed=seed, reset0=(par.copy(), st.copy()),
                               actions=np.zeros((T, n, 2 * N - 1), np.float32), rewards=np.zeros((T, n, 2 * N - 1)),
                               truncated=np.zeros((T, n), bool), params=np.zeros((T, n, L.size)), state=np.zeros((T, n, L.s_kmean)),
                               steps=np.zeros((T, n), np.int32), serial=np.zeros((T, n), np.int64), ck_serial=np.zeros(T, np.int64))
    steps = preset_steps(max_steps, 0, n)
    serial = 1                                                    # reset() rendered observation number 1
    for t in range(T):
        serial += 1
        tr.serial[t] = serial
        for i in range(n):
            p, s = par[i], st[i]
            pgt, bgt = s[L.s_gate_gt:L.s_gate_gt + N], s[L.s_barrier_gt:L.s_barrier_gt + N - 1]
            plo, phi = p[L.pmin:L.pmin + N], p[L.pmax:L.pmax + N]
            blo, bhi = p[L.bmin:L.bmin + N - 1], p[L.bmax:L.bmax + N - 1]
            if ROLES[i] == "far":
                act = design[i].uniform(-1, 1, 2 * N - 1).astype(np.float32)
            else:
                sg, sb = SPAN[ROLES[i]]
                act = np.concatenate([inverse_rescale(pgt + design[i].uniform(-sg, sg, N), plo, phi),
                                      inverse_rescale(bgt + design[i].uniform(-sb, sb, N - 1), blo, bhi)])
            gv, bv = O.rescale(act[:N], plo, phi), O.rescale(act[N:], blo, bhi)
            gr, br = O.reward(H.dev_view(N, p), pgt, bgt, gv, bv)          # against the ground truth before the step
            tr.actions[t, i] = act
            tr.rewards[t, i] = np.concatenate([gr, br])
            s[L.s_gate_v:L.s_gate_v + N] = gv
            s[L.s_barrier_v:L.s_barrier_v + N - 1] = bv
            steps[i] += 1
            tr.truncated[t, i] = steps[i] >= max_steps
        if tr.truncated[t].any():
            serial += 1                                           # the partial observe of the envs reset in this step
            for i in np.nonzero(tr.truncated[t])[0]:
                par[i], st[i] = draw(i)
                steps[i] = 0
                tr.serial[t, i] = serial
        tr.params[t], tr.state[t], tr.steps[t], tr.ck_serial[t] = par, st, steps, serial
    _TRAJ[(N, seed)] = tr
    return tr


def noise_params(par, L):
    return dict(white_amp=par[L.noise + 0], tel_p01=par[L.noise + 1], tel_p10=par[L.noise + 2], tel_amp=par[L.noise + 3],
                zero_radius=par[L.noise + 4], ramp_distance=par[L.noise + 5],
                full_noise_distance=par[L.noise + 6] if par[L.noise + 6] > 0 else None, max_amplitude=par[L.noise + 7])


def latch_probabilities(par, L):
    N = L.N
    return par[L.pleads:L.pleads + N].copy(), par[L.pinter:L.pinter + N * N].reshape(N, N).copy()


def latch_census(occ_det, occ_used, R_):
    """(latched pixels, of them rejected 1-dot changes, rejected 2-dot changes) of one channel: a pixel is latched when the
    walk left it another pixel's occupations; the branch is the number of dots in which the held state (the walk's output at
    the pixel before) differs from the pixel's own occupations in the numpy.isclose sense of the walk."""
    latched = np.nonzero((occ_used != occ_det).any(axis=1))[0]
    assert not np.any(latched % R_ == 0)                          # a row starts clean
    hold, nn = occ_used[latched - 1], occ_det[latched]
    ndiff = (~(np.abs(hold - nn) <= 1e-8 + 1e-5 * np.abs(nn))).sum(axis=1)
    assert np.all((ndiff == 1) | (ndiff == 2))
    return len(latched), int((ndiff == 1).sum()), int((ndiff == 2).sum())


def radial_status(par, sv, L, ch, R_):
    """"replaced", "ramp" (some pixel of the channel lies strictly inside the amplitude ramp), "flat" otherwise"""
    nz = noise_params(par, L)
    if NO.radial_replaced(sv.gate_v[ch], sv.gate_v[ch + 1], sv.gate_gt[ch], sv.gate_gt[ch + 1], nz["full_noise_distance"]):
        return "replaced"
    w = float(par[L.scal + 2])
    V1, V2 = np.meshgrid(np.linspace(sv.gate_v[ch] - w, sv.gate_v[ch] + w, R_), np.linspace(sv.gate_v[ch + 1] - w, sv.gate_v[ch + 1] + w, R_))
    dist = np.sqrt((V1 - sv.gate_gt[ch]) ** 2 + (V2 - sv.gate_gt[ch + 1]) ** 2)
    return "ramp" if np.any((dist > nz["zero_radius"]) & (dist < nz["ramp_distance"])) else "flat"


def full_state_row(N, row):
    """A state row of the trajectory (cut before the Kalman block) padded to the layout's width, for helpers.state_view."""
    out = np.zeros(layout(N).s_size)
    out[:len(row)] = row
    return out


def spectrum(dev, sv, ch, states):
    """helpers.pixel_spectrum of one channel, its rel_gap with the kept list's padding taken out where it matters.  A pixel
    with fewer than 32 valid candidates keeps copies of |0..0> (always at 2 dots: 16 candidates); where that state is the
    ground state the copies make the padded spectrum exactly degenerate although every copy is the same basis state and the
    occupations are well defined.  Such pixels are solved again on their distinct states.  Removing copies of an eigenvalue
    can only raise lam1, so this gap is never below the padded one: no pixel is exempt here that the project's rule compares."""
    sp = H.pixel_spectrum(dev, sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, sv.barrier_v, dev.window, ch, R, states=states)
    sp["rel_gap_padded"] = sp["rel_gap"]
    gap = sp["rel_gap"] = sp["rel_gap"].copy()
    N = dev.n_dot
    low = np.nonzero(gap <= H.GAP_MIN)[0]
    if len(low):
        vg = O.sweep_voltages(sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, ch, -dev.window, dev.window, R)
        vb = np.broadcast_to(np.asarray(sv.barrier_v, float), (R * R, N - 1))
        v_ext = np.concatenate([vg, vb], axis=1)
        tc = O.tunnel_couplings(O.effective_barrier_potential(vg, vb, dev.Cbg, dev.Cbb), dev.tc_base, dev.alpha)
        for p in low:
            uniq = np.unique(states[p], axis=0)
            if len(uniq) == states.shape[1] or len(uniq) < 2:
                continue
            F = O.free_energy_states(v_ext[p:p + 1], dev.cdd_inv_full, dev.cgd_full, uniq[None], N)
            Hm = F[0][:, None] * np.eye(len(uniq)) + O.tunnel_hamiltonian(tc[p:p + 1], uniq[None])[0]
            w = np.linalg.eigvalsh(Hm)
            gap[p] = (w[1] - w[0]) / np.abs(Hm).sum(axis=1).max()
    return sp


def rel_gap(dev, sv, ch, states):
    return spectrum(dev, sv, ch, states)["rel_gap"]


_FRAMES = {}


def frame(N, t, i, seed=None):
    """What the oracle alone says about env i of bucket N after step t of scene A: per channel the C oracle's kept states,
    occupations and signal, the relative gap of every pixel, the channel's radial status and the latching walk of the
    restatement on the oracle's occupations with this env's observation number."""
    seed = SEED if seed is None else seed
    key = (N, t, i, seed)
    if key in _FRAMES:
        return _FRAMES[key]
    tr = trajectory(N, seed)
    L = tr.L
    par = tr.params[t, i]
    dev, sv = H.dev_view(N, par), H.state_view(N, full_state_row(N, tr.state[t, i]))
    p_leads, p_inter = latch_probabilities(par, L)
    stream = NO.Stream(seed, tr.first + i, int(tr.serial[t, i]))
    chans = []
    for ch in range(N - 1):
        ref = OC.csd_channel(dev, sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, sv.barrier_v, dev.window, ch, R)
        used = NO.latch_walk(stream, ch, ref["occ"], R, p_leads, p_inter)
        chans.append(dict(ref=ref, census=latch_census(ref["occ"], used, R), radial=radial_status(par, sv, L, ch, R)))
    f = types.SimpleNamespace(N=N, t=t, i=i, reset=bool(tr.truncated[t, i]), channels=chans, dev=dev, sv=sv, exempt=None)
    _FRAMES[key] = f
    return f


def exempt_share(f):
    """The share of a frame's pixels whose relative gap (rel_gap) is at most helpers.GAP_MIN, over all channels"""
    if f.exempt is None:
        gaps = [rel_gap(f.dev, f.sv, ch, c["ref"]["states"]) for ch, c in enumerate(f.channels)]
        f.exempt = float(np.mean([np.mean(g <= H.GAP_MIN) for g in gaps]))
    return f.exempt


def latched_pixels(f, variant):
    """(latched, 1-dot, 2-dot) over the channels of a frame that the variant's radial stage does not replace"""
    tot = np.zeros(3, int)
    for c in f.channels:
        if "radial" in VARIANTS[variant] and c["radial"] == "replaced":
            continue
        tot += np.array(c["census"])
    return tuple(int(x) for x in tot)
