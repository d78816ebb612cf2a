"""Designed devices for the ground-state stage (csrc/qd_groundstate.h, csrc/qd_kernels.h: qd_k_gs_structure ->
qd_k_gs_solve<class> -> qd_k_gs_select), one source for both tiers: tests/test_gs_cases_cpu.py says from the oracle alone what
each family contains, tests/test_gpu_gs_designed.py runs them through the device code.  The sampler's scenes hold hop
components of 1..10 states and, in one pixel of a thousand, one of the memory class; the scenes here are built by hand so that
every block size 2..32 occurs, every size class wins the selection somewhere, and a batch's pool is filled to its last double.

A scene is search_cases.build's recipe (cdd_inv[:N,:N] = 0.25 I + r (J - I), cgd = [I 0], vgm = I, origin = 0,
window = (R - 1) step / 2) with generic, non-tying gate voltages and, optionally, barrier voltages overridden in the state
block.  With r close to 0.25 the matrix all but loses every mode except the uniform one: adding an electron costs far more
than moving one, so the 32 lowest states share one total-charge sector, and states of one sector are connected by hops.

    one_sector     r = 0.2499: one 32-state component per pixel
    all_sizes      r = 0.2: the sectors interleave, components of every size 1..32
    cut_pair       one_sector with barrier 1 at +800 V: tc[1] = tc_base exp(-alpha (800 + ...)) underflows to exactly 0.0, the
                   sector falls apart along pair 1
    denormal_pair  barrier 1 at 725 / alpha[1] V: tc[1] ~ 1e-316, a denormal -- non-zero, so it links: the components of
                   one_sector with the physics of cut_pair
    cut_two        barriers 0 and 2 at +800 V and +1200 V: only pairs 1 and 3 couple

The barrier voltages sit well inside the zero / denormal range of exp (the arguments are near -1600, -725 and -2400 with
exp reaching 0 at -745.2 and the denormals at -708.4), so that the device's exp and NumPy's agree on which it is.  NEGATIVE
barrier voltages of that size overflow tc to +inf and the Hamiltonian to NaN: that is out of scope here.

`make(name, N, R)` builds a member, `MEMBERS` lists what both tiers run, `census(name, N, R, ch, K)` is the oracle's view of
one channel (computed once per process, read-only): kept states, Hamiltonian parts, hop components, the component that holds
the ground vector and the relative gap."""
import numpy as np

import helpers as H
import qd_oracle as O
import qd_oracle_c as OC
import search_cases as SC
from qadapt_hip.layout import layout
from test_gs_prune_cpu import components

# Generic to four decimals on purpose.  Inside a sector E = (0.25 - r) sum (c_i - v_i)^2 + const, so two states tie in exact
# arithmetic wherever an integer combination of the v_i is an integer or a half: with (2.3, 1.9, 2.6, 2.1, 1.7) 2.3 + 1.9 = 2 * 2.1
# makes |3 2 3 1 2> and |2 1 3 3 2> tie along a diagonal of channel 0, where rounding decides the order and NumPy's einsum and
# the canonical arithmetic of the C oracle and the device decide differently (33 of 256 pixels).  The ties that matter to the
# search have tests/search_cases.py; here every oracle has to name the same kept states.
# The first five add up to 10.609375 = 10.5 + 3.5 / 32: the sector changes where the sum of the v_i passes a half-integer (within
# 2e-3 of it the 32 lowest states mix two sectors), and the pixels of a 5-dot scan have sums 10.609375 + k / 32, which stay
# 1 / 64 away from it.
GATES = (2.3137, 1.8891, 2.6173, 2.0719, 1.717375, 2.4397, 2.0113, 2.2259)
STEP = 1 / 32
PPB = 256                          # QD_GS_PPB of csrc/qd_groundstate.h: pixels per batch of the ground-state stage
CLASSES = [(s, s) for s in range(2, 9)] + [(9, 10), (11, 12), (13, 32)]      # size classes of the solve launches
SIZE_KEYS = [str(s) for s in range(2, 9)] + ["9+"]                           # solver_stats()["tasks_by_size"]

# name -> (r, {barrier index: volts, or ("over_alpha", x) for x / alpha[index]})
FAMILIES = {"one_sector": (0.2499, {}),
            "all_sizes": (0.2, {}),
            "cut_pair": (0.2499, {1: 800.0}),
            "denormal_pair": (0.2499, {1: ("over_alpha", 725.0)}),
            "cut_two": (0.2499, {0: 800.0, 2: 1200.0})}
CUT = {"cut_pair": (1,), "cut_two": (0, 2)}

# (family, N, R): 5 dots at 16 x 16 (one batch per channel), one_sector also at 17 x 17 (a second batch that ends in a
# half-wave with a clamped duplicate), and one 8-dot member for the neighbour slots in LDS (QD_NBREG < 2 (N - 1))
MEMBERS = [("one_sector", 5, 16), ("one_sector", 5, 17), ("all_sizes", 5, 16), ("cut_pair", 5, 16), ("denormal_pair", 5, 16),
           ("cut_two", 5, 16), ("all_sizes", 8, 16)]
# kept-set sizes of ("one_sector", 5, 16): both sides of every class boundary and of the kept-set instantiations 8 / 16 / 32
KEPT = (2, 3, 8, 9, 10, 11, 12, 13, 16, 17, 31, 32)
# ... compared on channels 0 and 3: with 8 to 17 kept states up to 58 of the 512 pixels of channels 1 and 2 have a relative gap
# below helpers.GAP_MIN (the couplings of 4e2 and 1e6 set ||H||, the lowest levels of a truncated sector lie 1e-3 apart), which
# puts K = 16 at 59 of 1024 = 5.8 % excluded pixels over all four channels, above the cap of the CPU tier; channels 0 and 3 have
# 10 of 512 at the most (K = 8) and the same block sizes
KEPT_CHANNELS = (0, 3)


def make(name, N, R):
    """(par, st) of family `name` with N dots, to be rendered at resolution R"""
    r, barriers = FAMILIES[name]
    par, st = SC.build(dict(r=r, gate=np.array([GATES[i % len(GATES)] for i in range(N)]), step=STEP), N, R)
    L = layout(N)
    for b, v in barriers.items():
        st[L.s_barrier_v + b] = v[1] / par[L.alpha + b] if isinstance(v, tuple) else v
    return par, st


def channels(N):
    return list(range(N - 1))


_CENSUS = {}


def census(name, N, R, ch, K=32):
    """The oracle alone on channel `ch` of a member with K kept states (the first K of the C oracle's 32: the truncation
    tests/test_num_charge_states.py pins).  dict of read-only arrays over the P = R * R pixels:
      states (P, K, N), F (P, K), tc (P, N - 1), Ht (P, K, K)
      sizes     list of P arrays: the sizes of the pixel's hop components (non-zero pattern of Ht)
      winner    (P,) size of the component with the lowest eigenvalue (numpy eigvalsh per component): it holds the ground vector
      rel_gap, lam0, hnorm   of the dense K x K Hamiltonian, as helpers.pixel_spectrum gives them
      ref       the C oracle's channel (states, floors, occ, z, tc) for K = 32"""
    key = (name, N, R, ch, K)
    if key not in _CENSUS:
        par, st = make(name, N, R)
        dev = H.dev_view(N, par); sv = H.state_view(N, st)
        if (name, N, R, ch, 32) in _CENSUS:
            ref = _CENSUS[(name, N, R, ch, 32)]["ref"]
        else:
            ref = OC.csd_channel(dev, sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, sv.barrier_v, dev.window, ch, R)
        states = np.ascontiguousarray(ref["states"][:, :K])
        vg = O.sweep_voltages(sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, ch, -dev.window, dev.window, R)
        vb = np.broadcast_to(sv.barrier_v, (R * R, N - 1))
        v_ext = np.concatenate([vg, vb], axis=1)
        F = O.free_energy_states(v_ext, dev.cdd_inv_full, dev.cgd_full, states, N)
        with np.errstate(under="ignore"):
            tc = O.tunnel_couplings(O.effective_barrier_potential(vg, vb, dev.Cbg, dev.Cbb), dev.tc_base, dev.alpha)
            Ht = O.tunnel_hamiltonian(tc, states)
        Hm = F[:, :, None] * np.eye(K) + Ht
        w = np.linalg.eigvalsh(Hm)
        hn = np.abs(Hm).sum(axis=2).max(axis=1)
        sizes, winner = [], np.zeros(R * R, np.int64)
        for p in range(R * R):
            comps = components(Ht[p] != 0.0)
            lam = [np.linalg.eigvalsh(Hm[p][np.ix_(c, c)])[0] for c in comps]
            sizes.append(np.array([c.size for c in comps]))
            winner[p] = comps[int(np.argmin(lam))].size
        c = dict(states=states, F=F, tc=tc, Ht=Ht, winner=winner, lam0=w[:, 0], hnorm=hn,
                 rel_gap=(w[:, 1] - w[:, 0]) / hn if K > 1 else np.full(R * R, np.inf))
        for v in c.values():
            v.setflags(write=False)
        for v in ref.values():
            v.setflags(write=False)
        c["sizes"] = sizes; c["ref"] = ref
        _CENSUS[key] = c
    return _CENSUS[key]


def size_counts(name, N, R, K=32, chs=None):
    """(components per size, winners per size) as arrays of 33 counts over the channels `chs` (all) of a member"""
    comp = np.zeros(33, np.int64); win = np.zeros(33, np.int64)
    for ch in (channels(N) if chs is None else chs):
        c = census(name, N, R, ch, K)
        comp += np.bincount(np.concatenate(c["sizes"]), minlength=33)
        win += np.bincount(c["winner"], minlength=33)
    return comp, win


def by_key(counts):
    """33 per-size counts -> the keys of solver_stats()["tasks_by_size"]: "2" .. "8" and "9+" """
    out = {str(s): int(counts[s]) for s in range(2, 9)}
    out["9+"] = int(counts[9:].sum())
    return out
