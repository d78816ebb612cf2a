"""Designed devices for the candidate search (csrc/qd_tile.h, csrc/qd_pixel.h), one source for both tiers:
tests/test_search_cases_cpu.py runs them through the host build of the per-pixel search, tests/test_gpu_search_adversarial.py
through the device code.  The scenes of the other search tests come from the device sampler, where float64 energies never
tie, floors stay small and a tile rarely leaves the fast path; the scenes here are built by hand so that they do.

A scene is a parameter / state block of the product's sampler with the search-relevant part overwritten:

    cdd_inv[:N,:N] = 0.25 I + r (J - I)      (ufac / uinv: its reversed Cholesky factor)
    cgd[:N]        = [I 0],  vgm = I,  origin = 0      ->  v' = the virtual plunger voltages themselves
    window         = (R - 1) * step / 2      ->  linspace(v - w, v + w, R) has the exact step `step` for every R

With r, gate_v and step dyadic every energy of the 4^N scan is an exact float64 in any summation order, so equal energies
are equal bit for bit and the (E, index) rule decides.  The sensor row of cdd_inv / cgd, the barrier model and the noise
block stay the sampled ones; `cbg` is zeroed where the plungers sit at 3e4 V (the couplings would overflow).

`make(name, N, R)` builds a family member, `MEMBERS` lists the members both tiers run, `brute_force` is a plain NumPy
scan of all 4^N candidates for checking that the families are what they claim to be (N <= 5), `lowest_energies` the
same energies without the indices for any N."""
import numpy as np

import helpers as H
import qd_oracle as O
from qadapt_hip.layout import layout

BIAS = 0x7FFF                      # QD_FL_BIAS of csrc/qd_tile.h: the largest floor of the packed min / max reduction
KS = (32, 16, 8)                   # kept-set sizes of the three kernel instantiations


def _gates(N, base):
    """the first N of a repeating dyadic pattern"""
    return np.array([base[i % len(base)] for i in range(N)], dtype=np.float64)


def _dyadic(N, R):
    """r = 0, equal dyadic voltages: the energy is a sum of per-dot squares, ties in every pixel"""
    return dict(r=0.0, gate=np.full(N, 1.5), step=1 / 8)


def _dyadic_mixed(N, R):
    """r = 0, a different dyadic voltage per dot (the 6- and 8-dot member: with equal voltages 2^(N-2) states would tie)"""
    return dict(r=0.0, gate=_gates(N, (1.5, 1.25, 2.0, 0.75, 1.125, 2.5, 0.25, 1.75)), step=1 / 8)


def _exchange(N, R):
    """r = 1/16 (1/32 from 6 dots on), equal voltages: ties from the dot-exchange symmetry of the unswept dots and of the diagonal"""
    return dict(r=1 / 16 if N < 6 else 1 / 32, gate=np.full(N, 1.5), step=1 / 8 if N < 6 else 1 / 16)


def _high_floor(N, R):
    """every dot near 40000.5: no floor fits the packed reduction; generic offsets, so that tiles complete"""
    off = _gates(N, (0.13, 0.37, -0.21, 0.29, -0.08, 0.41, 0.02, -0.33))
    return dict(r=0.03, gate=40000.5 + off, step=0.7 * 2 / 32, zero_cbg=True)


def _straddle(N, R):
    """gate 32768 = 0x8000, r = 0: floors 0x7FFE..0x8002, packable and unpackable lanes in one tile, ties everywhere"""
    return dict(r=0.0, gate=np.full(N, 32768.0), step=1 / 8, zero_cbg=True)


def _one_dot_high(N, R):
    """the last dot (never swept in channel 0) above 0x7FFF, the others small; generic offsets"""
    g = _gates(N, (1.63, 2.17, 0.79, 1.31, 2.42, 0.58, 1.87, 1.12))
    g[N - 1] = 40000.3
    return dict(r=0.03, gate=g, step=0.7 * 2 / 32, zero_cbg=True)


def _depleted(N, R):
    """dot 0 occupied, dot 1 negative, dot 2 at exactly 0, dot 3 at -0.0, then alternating; channel 0 sweeps an occupied
    and a depleted dot through 0, channel 2 sweeps the two zeros.  v' = -0.0 needs a product that underflows: the chain
    fma(cgd[3][j], v_ext[j], acc) starts from +0.0 and (+0.0) + (-0.0) = +0.0, so a voltage of -0.0 alone does not give it;
    cgd[3][N] = -2^-1074 times the sensor voltage 0.25 rounds to -0.0, and the barrier columns of that row are zeros signed against the barrier voltages (products of -0.0)."""
    g = _gates(N, (1.5, -0.75, 0.0, 0.0, 2.25, -1.5, 0.5, -0.25))
    return dict(r=1 / 16, gate=g, step=1 / 8, minus_zero_dot=3)


def _wide_window(N, R):
    """Up to 5 dots half an electron per pixel: a full tile spans 3.5 electrons in the two swept dots, so a tile's floors
    differ by 3 or by 4 (> 3: no candidate is valid in every pixel, hand-over `ranges`) depending on where it starts, and by 0
    where both swept dots are depleted (the lower left of the image).  From 6 dots on a quarter electron per pixel: every tile
    passes the range test, and the states below a tile's threshold outgrow the frontier (832) or the superset (383)."""
    return dict(r=1 / 16, gate=_gates(N, (0.5, 0.25, 1.5, 1.25, 0.75, 2.0, 1.0, 1.75)), step=1 / 2 if N < 6 else 1 / 4)


def _soft_mode(N, R):
    """r = -0.99 * 0.25 / (N - 1), where 0.25 I + r (J - I) all but loses the uniform mode: moving an electron between dots
    costs little next to adding one, the threshold of a tile lies far above its ground energy in units of the stiff
    directions, and at 8 dots some tiles outgrow the frontier"""
    return dict(r=-0.99 * 0.25 / (N - 1), gate=_gates(N, (2.3, 1.9, 2.6, 2.1, 1.7, 2.4, 2.0, 2.2)), step=0.7 * 2 / 32)


FAMILIES = {"dyadic": _dyadic, "dyadic_mixed": _dyadic_mixed, "exchange": _exchange, "high_floor": _high_floor,
            "straddle": _straddle, "one_dot_high": _one_dot_high, "depleted": _depleted, "wide_window": _wide_window,
            "soft_mode": _soft_mode}

# every energy is an exact float64: the NumPy scan equals the canonical arithmetic bit for bit
EXACT = ("dyadic", "dyadic_mixed", "exchange", "straddle", "depleted")
# at least 10 % of the pixels tie exactly at the boundary of the kept set, for K = 8, 16 and 32
TIE_FAMILIES = ("dyadic", "dyadic_mixed", "exchange", "straddle")

# (family, N, R): the smallest shapes that reach the tile kernel (N >= 4, R >= 32); R = 33 has one-pixel-wide edge tiles,
# 36 four-pixel-wide ones, 32 and 40 none
MEMBERS = [("dyadic", 4, 33), ("dyadic", 4, 36), ("exchange", 4, 33), ("exchange", 4, 40), ("straddle", 4, 33),
           ("straddle", 5, 32), ("high_floor", 4, 33), ("high_floor", 6, 32), ("one_dot_high", 4, 36), ("depleted", 4, 33),
           ("depleted", 5, 36), ("wide_window", 4, 36), ("wide_window", 4, 33), ("wide_window", 6, 36), ("soft_mode", 8, 32),
           ("dyadic_mixed", 6, 36), ("dyadic_mixed", 8, 32), ("exchange", 8, 32)]

_SEED = 4242
_BLOCKS = {}


def sampled(N):
    """the sampled block every member of size N starts from (and the ordinary neighbour of the GPU tier): read-only"""
    if N not in _BLOCKS:
        eb = H.sample_blocks(N, [_SEED + N, _SEED + 100 + N])
        par, st = np.ascontiguousarray(eb.params), np.ascontiguousarray(eb.state)
        par.setflags(write=False); st.setflags(write=False)
        _BLOCKS[N] = (par, st)
    return _BLOCKS[N]


def cdd_inv_block(N, r):
    return 0.25 * np.eye(N) + r * (np.ones((N, N)) - np.eye(N))


def make(name, N, R, tc_base=None):
    """(par, st) of family `name` with N dots, to be rendered at resolution R.  tc_base None keeps the sampled one."""
    return build(FAMILIES[name](N, R), N, R, tc_base=tc_base)


def build(spec, N, R, tc_base=None):
    """the recipe of the module docstring for one spec, dict(r, gate, step[, zero_cbg, minus_zero_dot]): tests/gs_cases.py
    builds its own families on it"""
    L = layout(N); G = N + 1; V = 2 * N
    par, st = (a[0].copy() for a in sampled(N))
    A = par[L.cdd_inv:L.cdd_inv + G * G].reshape(G, G).copy()
    A[:N, :N] = cdd_inv_block(N, spec["r"])
    par[L.cdd_inv:L.cdd_inv + G * G] = A.reshape(-1)
    U = np.linalg.cholesky(A[:N, :N][::-1, ::-1])[::-1, ::-1]                    # A = U U^T, U upper
    par[L.ufac:L.ufac + N * N] = U.reshape(-1); par[L.uinv:L.uinv + N] = 1 / np.diag(U)
    cgd = par[L.cgd:L.cgd + G * V].reshape(G, V).copy()
    cgd[:N] = 0.0; cgd[:N, :N] = np.eye(N)
    st[L.s_sensor_gt] = 0.25
    if "minus_zero_dot" in spec:
        i = spec["minus_zero_dot"]
        cgd[i, N] = -np.ldexp(1.0, -1074)
        cgd[i, G:] = np.copysign(0.0, -st[L.s_barrier_v:L.s_barrier_v + N - 1])               # zeros whose products are -0.0
    par[L.cgd:L.cgd + G * V] = cgd.reshape(-1)
    if spec.get("zero_cbg"):
        par[L.cbg:L.cbg + (N - 1) * G] = 0.0
    par[L.origin:L.origin + G] = 0.0
    par[L.scal + 2] = (R - 1) * spec["step"] / 2
    par[L.scal + 4] = 0.0
    if tc_base is not None:
        par[L.scal] = tc_base
    st[L.s_vgm:L.s_vgm + G * G] = np.eye(G).reshape(-1)
    st[L.s_gate_v:L.s_gate_v + N] = spec["gate"]
    return par, st


def v_dash(N, par, st, ch, R):
    """(P, N) v' of every pixel of channel `ch` in NumPy (exact for the dyadic families) and the continuous minimiser"""
    dev = H.dev_view(N, par); sv = H.state_view(N, st)
    vg = O.sweep_voltages(sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, ch, -dev.window, dev.window, R)
    v_ext = np.concatenate([vg, np.broadcast_to(sv.barrier_v, (R * R, N - 1))], axis=1)
    vd = v_ext @ dev.cgd_full[:N].T
    return vd, O.continuous_ground_state(v_ext, dev.cdd_inv_full, dev.cgd_full, N)


def brute_force(N, par, st, ch, R, floors):
    """All 4^N candidates c = floors + delta, delta in {-1, 0, 1, 2}^N with dot 0 the most significant base-4 digit, of every
    pixel in plain NumPy: (E, order) with E (P, 4^N) the energies sorted by (E, index), c < 0 at +inf, and order the candidate
    indices in that order.  For checking the families' conditions (N <= 5), not the kernels."""
    assert N <= 5
    L = layout(N); G = N + 1
    A = par[L.cdd_inv:L.cdd_inv + G * G].reshape(G, G)[:N, :N]
    vd, _ = v_dash(N, par, st, ch, R)
    idx = np.arange(4 ** N)
    delta = np.stack([(idx >> (2 * (N - 1 - i))) & 3 for i in range(N)], axis=1) - 1           # (4^N, N)
    c = floors[:, None, :] + delta[None]                                                     # (P, 4^N, N)
    d = c - vd[:, None, :]
    E = np.einsum("pki,ij,pkj->pk", d, A, d)
    E[(c < 0).any(axis=2)] = np.inf
    order = np.argsort(E, axis=1, kind="stable")                                             # stable: ties by index
    return np.take_along_axis(E, order, axis=1), order


def lowest_energies(N, par, st, ch, R, floors, k):
    """(P, k) the k lowest energies of the 4^N candidates of every pixel, sorted, for any N: the scan split into the two swept
    dots (16 choices per pixel) and the unswept ones (4^(N-2) choices, the same in every pixel), with the closed form
    E = (a - r) sum d^2 + r (sum d)^2 of A = a I + r (J - I).  Exact, hence equal to the canonical energies, in the EXACT
    families; no candidate indices, so ties are counted but not ordered."""
    L = layout(N); G = N + 1
    A = par[L.cdd_inv:L.cdd_inv + G * G].reshape(G, G)[:N, :N]
    a, r = A[0, 0], A[0, 1]
    assert np.array_equal(A, cdd_inv_block(N, r) + (a - 0.25) * np.eye(N))
    vd, _ = v_dash(N, par, st, ch, R)
    sw = [ch, ch + 1]; un = [i for i in range(N) if i not in sw]
    assert (floors[:, un] == floors[0, un]).all() and (vd[:, un] == vd[0, un]).all()
    dl = np.arange(-1, 3)
    cu = floors[0, un][None, :] + np.stack(np.meshgrid(*[dl] * len(un), indexing="ij"), axis=-1).reshape(-1, len(un))
    du = cu - vd[0, un]
    s2u = (du * du).sum(axis=1); s1u = du.sum(axis=1)
    s2u = np.where((cu < 0).any(axis=1), np.inf, s2u)
    cs = floors[:, None, sw] + np.stack(np.meshgrid(dl, dl, indexing="ij"), axis=-1).reshape(-1, 2)[None]      # (P, 16, 2)
    ds = cs - vd[:, None, sw]
    s2s = np.where((cs < 0).any(axis=2), np.inf, (ds * ds).sum(axis=2)); s1s = ds.sum(axis=2)
    out = np.empty((floors.shape[0], k))
    for p0 in range(0, floors.shape[0], 64):
        s1 = s1s[p0:p0 + 64, :, None] + s1u[None, None, :]
        E = ((a - r) * (s2s[p0:p0 + 64, :, None] + s2u[None, None, :]) + r * (s1 * s1)).reshape(s1.shape[0], -1)
        out[p0:p0 + 64] = np.sort(np.partition(E, k - 1, axis=1)[:, :k], axis=1)
    return out


def states_of(floors, order, k):
    """(P, k, N) the first k states of `order`"""
    N = floors.shape[1]
    o = order[:, :k]
    delta = np.stack([(o >> (2 * (N - 1 - i))) & 3 for i in range(N)], axis=2) - 1
    return (floors[:, None, :] + delta).astype(np.int32)
