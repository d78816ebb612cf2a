"""Probe scans with the stochastic stages, CPU tier: one row of the latching walk (csrc/qd_latch.h: qd_latch_row, compiled
for the host in tests/hosttest_latch) against the NumPy restatement of the whole walk, bit for bit; the prototype, export
and argument checks of qd_probe_ex; and the `noise` keyword of `env.array._get_obs` on a stub backend.  No GPU needed."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import helpers as H
import qd_noise_oracle as NO
import test_probe as TP
from qadapt_hip import device_model as DM
from qadapt_hip.layout import layout

ROOT = H.ROOT
_HOST = None


def _hosttest():
    global _HOST
    if _HOST is None:
        hdir = os.path.join(ROOT, "tests", "hosttest_latch")
        subprocess.check_call(["make", "-s", "-C", hdir, "libqdsim_hosttest_latch.so"])
        _HOST = ctypes.CDLL(os.path.join(hdir, "libqdsim_hosttest_latch.so"))
    return _HOST


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _fma(a, b, c):
    """round(a * b + c) with one rounding, as fma(): Fraction arithmetic is exact and float() rounds correctly."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def _scene(N, R, rng):
    """(P, N) occupations along the raster: every pixel differs from its left neighbour in 0, 1, 2 or 3 dots (as many as
    N has), by whole carriers; some equal dots are moved by 1e-9, below the isclose tolerance.  Returns the occupations and
    how often a neighbour pair differs in k dots."""
    P = R * R
    occ = np.zeros((P, N))
    kinds = np.zeros(4, int)
    cur = rng.integers(0, 3, N).astype(float)
    for p in range(P):
        k = int(rng.integers(0, min(3, N) + 1))
        dots = rng.choice(N, size=k, replace=False)
        cur = cur.copy()
        cur[dots] += rng.choice([-1.0, 1.0], size=k)
        if p % R:
            kinds[k] += 1
        occ[p] = cur + (1e-9 * rng.random(N)) * (rng.random(N) < 0.3)
    return occ, kinds


@pytest.mark.parametrize("N", [2, 4, 8])
def test_latch_row_equals_the_walk_bit_for_bit(N):
    """R = 6, probabilities 0, 1 and 0.5, two serials (one with the top bit set, as side questions use): the rows latched
    one by one, in reverse order, equal oracle/qd_noise_oracle.py::latch_walk over the whole image as 64-bit patterns, and
    the sensor constant of every held pixel is c0 + 2 * fma-chain(A[N][i], held_i - own_i), that of every other pixel
    untouched."""
    host = _hosttest()
    R, ch, seed, gid = 6, N - 2, 0x1234ABCD5678, 1000 + N
    L, G, P = layout(N), N + 1, R * R
    rng = np.random.default_rng(40 + N)
    occ, kinds = _scene(N, R, rng)
    assert kinds[1] > 0 and kinds[2] > 0 and (kinds[3] > 0 or N < 3), kinds
    z = rng.normal(0, 1, P)
    dp = ctypes.POINTER(ctypes.c_double)
    held_at_half = 0
    for prob in (0.0, 1.0, 0.5):
        par = rng.normal(0, 0.3, L.size)
        par[L.pleads:L.pleads + N] = prob
        par[L.pinter:L.pinter + N * N] = prob
        A = par[L.cdd_inv + N * G:L.cdd_inv + N * G + N]
        for serial in (7, (1 << 63) | 3):
            s = NO.Stream(seed, gid, serial)
            ref = NO.latch_walk(s, ch, occ, R, par[L.pleads:L.pleads + N], par[L.pinter:L.pinter + N * N].reshape(N, N))
            got, zg = occ.copy(), z.copy()
            for row in reversed(range(R)):                        # rows are independent: any order
                rc = host.qdhl_latch_row(N, par.ctypes.data_as(dp), got.ctypes.data_as(dp), zg.ctypes.data_as(dp), row, R, ch,
                                         ctypes.c_uint32(s.k0), ctypes.c_uint32(s.ser_lo), ctypes.c_uint32(s.ser_hi),
                                         ctypes.c_uint32(s.k1))
                assert rc == 0
            assert np.array_equal(_bits(got), _bits(ref)), (N, prob, serial)
            held = (ref != occ).any(axis=1)
            assert not held.reshape(R, R)[:, 0].any()             # a row starts clean
            want = z.copy()
            for p in np.nonzero(held)[0]:
                corr = 0.0
                for i in range(N):
                    corr = _fma(A[i], ref[p, i] - occ[p, i], corr)
                want[p] = z[p] + 2.0 * corr
            assert np.array_equal(_bits(zg), _bits(want)), (N, prob, serial)
            if prob == 1.0:
                assert not held.any()
            if prob == 0.0:
                assert held.any()
            if prob == 0.5:
                held_at_half += int(held.sum())
    assert held_at_half > 0
    assert host.qdhl_latch_row(N, par.ctypes.data_as(dp), got.ctypes.data_as(dp), zg.ctypes.data_as(dp), R, R, ch, 0, 0, 0, 0) == 1


def test_latch_row_draws_differ_between_serials_and_streams():
    """Probability 0.5: another serial or another global env id holds other pixels (the draws are really keyed by them)."""
    host = _hosttest()
    N, R, ch = 4, 6, 1
    L = layout(N)
    rng = np.random.default_rng(5)
    occ, _ = _scene(N, R, rng)
    par = rng.normal(0, 0.3, L.size)
    par[L.pleads:L.pleads + N] = 0.5
    par[L.pinter:L.pinter + N * N] = 0.5
    dp = ctypes.POINTER(ctypes.c_double)
    outs = []
    for gid, serial in ((3, 9), (3, 10), (4, 9)):
        s = NO.Stream(77, gid, serial)
        got, zg = occ.copy(), np.zeros(R * R)
        for row in range(R):
            assert host.qdhl_latch_row(N, par.ctypes.data_as(dp), got.ctypes.data_as(dp), zg.ctypes.data_as(dp), row, R, ch,
                                       ctypes.c_uint32(s.k0), ctypes.c_uint32(s.ser_lo), ctypes.c_uint32(s.ser_hi),
                                       ctypes.c_uint32(s.k1)) == 0
        outs.append(got)
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2])


# ------------------------------------------------------------------ C ABI without a GPU
def _built_lib():
    from qadapt_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail(f"{_lib.LIB_PATH} is missing: run __graft_entry__.build() before the tests (no test compiles it)")
    return _lib, _lib.lib()


def test_probe_ex_symbol_and_prototype():
    _lib, L = _built_lib()
    assert "qd_probe_ex" in _lib.EXPORTS and hasattr(L, "qd_probe_ex")
    at = L.qd_probe_ex.argtypes
    assert len(at) == 12 and at[2] is ctypes.c_int and L.qd_probe_ex.restype is ctypes.c_int
    assert at[10]._type_ is _lib.QdProbeOpts
    assert at[:10] == L.qd_probe.argtypes[:10]                  # the ten data arguments of qd_probe, unchanged
    f = dict(_lib.QdProbeOpts._fields_)
    assert list(f) == ["struct_size", "noise_flags", "serial", "stream_base", "occ_dst"]
    assert f["serial"] is ctypes.c_uint64 and f["stream_base"] is ctypes.c_int64 and ctypes.sizeof(_lib.QdProbeOpts) == 32
    hdr = open(os.path.join(ROOT, "include", "qdsim.h")).read()
    assert "int qd_probe_ex(qd_handle* h, const int32_t* env_of_query_dev, int nq, const double* gate_v_dev," in hdr
    assert "} qd_probe_opts;" in hdr and "stochastic probes are not built" not in hdr
    # a null handle is an argument error, not a crash, with or without options
    assert L.qd_probe_ex(None, None, 1, None, None, None, None, None, None, None, None, None) == _lib.QD_ERR_ARG
    opts = _lib.QdProbeOpts(struct_size=ctypes.sizeof(_lib.QdProbeOpts))
    assert L.qd_probe_ex(None, None, 1, None, None, None, None, None, None, None, ctypes.byref(opts), None) == _lib.QD_ERR_ARG


def test_probe_ex_argument_checks_need_no_device():
    """As tests/test_probe.py: without a GPU qd_create fails with QD_ERR_HIP and still hands out the partial handle, which is
    all the argument checks need; every call below returns before anything touches the device."""
    _lib, L = _built_lib()
    from qadapt_hip.vec_env import make_qd_config
    cfg = make_qd_config(DM.load_yaml(None, "env_config.yaml"), DM.load_yaml(None, "qarray_config.yaml"), 4, 8, 2)
    h = ctypes.c_void_p()
    L.qd_create(ctypes.byref(cfg), 0, ctypes.byref(h))
    if not h:
        pytest.fail("qd_create handed out no handle")
    try:
        one = ctypes.c_void_p(64)                                # never dereferenced
        size = ctypes.sizeof(_lib.QdProbeOpts)
        call = lambda nq, o, ids=one: L.qd_probe_ex(h, ids, nq, one, one, None, None, None, None, None,      # noqa: E731
                                                    None if o is None else ctypes.byref(o), None)
        for bad in (0, size - 8, size + 8):
            assert call(1, _lib.QdProbeOpts(struct_size=bad)) == _lib.QD_ERR_ARG
            assert b"struct_size" in L.qd_last_error(h)
        for flags in (8, 7 | 16, -1):
            assert call(1, _lib.QdProbeOpts(struct_size=size, noise_flags=flags)) == _lib.QD_ERR_ARG
            assert b"noise_flags" in L.qd_last_error(h)
        # qd_probe's own checks come first and still hold with options
        ok = _lib.QdProbeOpts(struct_size=size, noise_flags=7, serial=(1 << 63) | 5, stream_base=1000)
        assert call(1, ok, ids=None) == _lib.QD_ERR_ARG and b"env_of_query" in L.qd_last_error(h)
        assert call(-1, ok) == _lib.QD_ERR_ARG and b"nq < 0" in L.qd_last_error(h)
        assert call(0, ok) == 0 and call(0, None) == 0           # nq == 0 does nothing
        # the options are checked even when there is nothing to render
        assert call(0, _lib.QdProbeOpts(struct_size=size, noise_flags=8)) == _lib.QD_ERR_ARG
    finally:
        L.qd_destroy(h)


# ------------------------------------------------------------------ the array facade on a stub backend
class KwStub(TP.StubBackend):
    """Records the keywords beyond the five of the deterministic probe."""

    def probe(self, env_ids, gate_voltages, barrier_voltages, sensor_voltage=None, window=None, normalised=False, **kw):
        out = super().probe(env_ids, gate_voltages, barrier_voltages, sensor_voltage, window, normalised)
        self.probes[-1]["extra"] = kw
        return out


def test_get_obs_passes_noise_on_only_when_asked(tmp_path):
    import yaml
    from qadapt_hip.env import QuantumDeviceEnv
    N, R = 4, 6
    cfg = DM.load_yaml(None, "env_config.yaml")
    cfg["capacitance_model"]["update_method"] = None
    cfg["simulator"].update(num_dots=N, resolution=R)
    p = tmp_path / "env.yaml"
    p.write_text(yaml.safe_dump(cfg))
    # a backend whose probe knows nothing of the new keyword still serves the default call
    old = QuantumDeviceEnv(config_path=str(p), backend=TP.StubBackend(N, R))
    old.array._get_obs(np.zeros(N), np.zeros(N - 1))
    old.array._get_obs(np.zeros(N), np.zeros(N - 1), noise=False)
    assert len(old._b.probes) == 2
    with pytest.raises(TypeError, match="noise"):
        old.array._get_obs(np.zeros(N), np.zeros(N - 1), noise=True)
    env = QuantumDeviceEnv(config_path=str(p), backend=KwStub(N, R))
    a = env.array
    a._get_obs(np.zeros(N), np.zeros(N - 1), sensor_voltage=0.5)
    assert env._b.probes[-1]["extra"] == {} and env._b.probes[-1]["sensor_voltage"] == 0.5
    a._get_obs(np.zeros(N), np.zeros(N - 1), noise=False)
    assert env._b.probes[-1]["extra"] == {}
    obs = a._get_obs(np.zeros(N), np.zeros(N - 1), noise=True)
    assert env._b.probes[-1]["extra"] == {"noise": True}
    assert obs["image"].shape == (R, R, N - 1) and env.current_step == 0


def test_probe_keywords_of_the_maps_and_the_vec_env():
    """The signatures the issue names, without a device: probe's four keywords with their defaults, the maps' `noise`."""
    import inspect
    from qadapt_hip import device_map as M
    from qadapt_hip.vec_env import VecQuantumDeviceEnv
    sig = inspect.signature(VecQuantumDeviceEnv.probe).parameters
    assert [sig[k].default for k in ("noise", "serial", "stream_base", "occupations")] == [None, None, None, False]
    for f in (M.map_device_range, M.map_full_device_range):
        assert inspect.signature(f).parameters["noise"].default is None
