"""Adversarial inputs of the exact-percentile kernels (qd_k_percentile cached / uncached, the grid-wide qd_k_sel_* select),
shared by test_pct_cases_cpu.py and test_gpu_percentile_adversarial.py, and the host restatement of the kernels' rank and
interpolation arithmetic.  The simulator's signals are smooth and positive, with nearly equal leading key bytes; these are
not: ties that end on either side of a rank, negative keys, signed zeros and denormals, infinities, one NaN, sizes below a
block, one past a multiple of 1024 and on both sides of the 32 768 boundary between the two single-block kernels."""
import functools
import math

import numpy as np

SIZES = (1, 2, 3, 63, 64, 65, 200, 201, 202, 401, 1023, 1024, 1025, 4097, 20000, 32767, 32768, 32769, 40001, 80000)
PCTS = (0.5, 99.5)
TIE_OFFSETS = (-1, 0, 1, 2)
SEED = 60221

# families whose percentiles or normalised image involve inf - inf or inf / inf: percentiles are still compared (NaN = NaN),
# the image rule is not (qd_norm maps inf / inf to 0 where numpy keeps NaN, and nothing in the reference defines it)
NON_FINITE = ("one_inf_each", "many_inf", "nan_last", "huge")


def ranks(n, pc):
    """(ip, in, g) of the numpy 'linear' method as the kernels form them: (n-1)*q, floor, clamp"""
    virt = float(n - 1) * (pc / 100.0)
    prev = math.floor(virt)
    ip = min(max(int(prev), 0), n - 1)
    return ip, min(ip + 1, n - 1), virt - prev


def tie_count(n, which, d):
    """number of copies of the LOWER value so that its run ends at sorted index ip + d (clamped to [0, n])"""
    return min(max(ranks(n, PCTS[which])[0] + d + 1, 0), n)


@functools.lru_cache(maxsize=None)
def families(n):
    """((name, float64 array of n values), ...), the same on every call"""
    rng = np.random.default_rng([SEED, n])
    out = []

    def add(name, z):
        z = np.ascontiguousarray(z, dtype=np.float64)
        assert z.shape == (n,)
        z.setflags(write=False)
        out.append((name, z))

    add("const", np.full(n, 0.25))
    add("const_neg", np.full(n, -3.5))
    z = np.full(n, 1.0); z[rng.integers(n)] = 2.0; add("one_high", z)
    z = np.full(n, 1.0); z[rng.integers(n)] = -2.0; add("one_low", z)
    for which, tag, (lo, hi) in ((0, "lo", (0.0, 1.0)), (1, "hi", (1.0, 3.0))):
        for d in TIE_OFFSETS:
            z = np.full(n, hi); z[:tie_count(n, which, d)] = lo; rng.shuffle(z)
            add(f"two_valued_{tag}{d:+d}", z)
    add("signs", rng.normal(0, 1, n) * 10.0 ** rng.integers(-300, 300, n))
    add("denormals", rng.integers(-50, 50, n).astype(np.float64) * 5e-324)
    z = rng.normal(0, 1, n); z[rng.random(n) < 0.3] = 0.0; z[rng.random(n) < 0.1] = -0.0; add("zeros_pm", z)
    add("few_levels", rng.integers(0, 3, n).astype(np.float64))
    add("ulp_cluster", 1.0 + rng.integers(0, 8, n) * 2.0 ** -52)
    z = rng.normal(0, 1, n); z[rng.integers(n)] = np.inf; z[rng.integers(n)] = -np.inf; add("one_inf_each", z)
    z = rng.normal(0, 1, n); m = max(1, n // 50); z[:m] = np.inf; z[m:2 * m] = -np.inf; rng.shuffle(z); add("many_inf", z)
    z = rng.normal(0, 1, n); z[-1] = np.nan; add("nan_last", z)
    add("sorted", np.sort(rng.normal(0, 1, n)))
    add("reversed", np.sort(rng.normal(0, 1, n))[::-1])
    add("huge", rng.choice([1.7e308, -1.7e308, 1e308], n))
    return tuple(out)


def family(n, name):
    return dict(families(n))[name]


def keys(z):
    """qd_key: order-preserving 64-bit keys (-0.0 below +0.0, -inf lowest)"""
    u = np.ascontiguousarray(z, np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def lerp(a, b, t):
    """qd_lerp"""
    with np.errstate(all="ignore"):
        a, b = np.float64(a), np.float64(b)
        d = b - a
        r = a + d * t
        if t >= 0.5:
            r = b - d * (1.0 - t)
    return r


def kernel_percentiles(z):
    """What the three kernels compute, restated on the host: values ordered by their keys, ranks as `ranks`, qd_lerp;
    NaN anywhere gives (NaN, NaN)."""
    z = np.ascontiguousarray(z, np.float64)
    if np.isnan(z).any():
        return np.array([np.nan, np.nan])
    s = z[np.argsort(keys(z), kind="stable")]
    out = []
    for pc in PCTS:
        ip, inn, g = ranks(z.size, pc)
        out.append(lerp(s[ip], s[inn], g))
    return np.array(out)


def numpy_percentiles(z):
    with np.errstate(all="ignore"):
        return np.array([np.percentile(z, pc) for pc in PCTS])


def same_percentiles(name, got, ref):
    """The comparison of both test tiers: bit patterns; `==` for the +-0.0 family (numpy's partition does not order the two
    zeros, the kernels' keys do); NaN matches NaN."""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    for a, b in zip(got, ref):
        if np.isnan(b):
            if not np.isnan(a):
                return False
        elif name == "zeros_pm":
            if not a == b:
                return False
        elif np.float64(a).view(np.uint64) != np.float64(b).view(np.uint64):
            return False
    return True
