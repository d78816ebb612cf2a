"""latched_model.num_charge_states (K, qarray_config.yaml:129): the option checks, the qd_config a handle is built
from, and the truncation argument the kernels rely on (no GPU needed)."""
import ctypes

import numpy as np
import pytest

import qd_oracle as O
import helpers as H
from qadapt_hip import _lib
from qadapt_hip import device_model as DM


def _qconfig(k):
    q = DM.load_yaml(None, "qarray_config.yaml")
    q["simulator"]["latched_model"]["num_charge_states"] = k
    return q


@pytest.mark.parametrize("k", [1, 8, 16, 31, 32])
def test_kept_state_counts_up_to_32_are_accepted(k):
    assert DM.check_solver_options(_qconfig(k)) == k


@pytest.mark.parametrize("k", [0, 33, 64, -1, 8.5, "16x"])
def test_other_kept_state_counts_are_refused(k):
    with pytest.raises(NotImplementedError, match="32"):
        DM.check_solver_options(_qconfig(k))


def test_use_sparse_is_still_refused_whatever_k():
    q = _qconfig(16)
    q["simulator"]["latched_model"]["use_sparse"] = True
    with pytest.raises(NotImplementedError, match="use_sparse"):
        DM.check_solver_options(q)


def test_qd_config_field_keeps_the_reserved_slot():
    """num_charge_states took the place of reserved0: same offset, same struct size, so zeroed callers get K = 32."""
    f = _lib.QdConfig
    assert f.num_charge_states.offset == f.cnn_outputs.offset + 4
    assert f.delta_max.offset == f.num_charge_states.offset + 4
    assert ctypes.sizeof(f) == 184
    assert f().num_charge_states == 0


@pytest.mark.parametrize("k,expect", [(None, 32), (32, 32), (16, 16), (8, 8), (20, 20), (1, 1)])
def test_qd_config_carries_k(k, expect):
    from qadapt_hip.vec_env import make_qd_config
    q = DM.load_yaml(None, "qarray_config.yaml")
    if k is not None:
        q["simulator"]["latched_model"]["num_charge_states"] = k
    e = DM.load_yaml(None, "env_config.yaml")
    cfg = make_qd_config(e, q, 8, 64, 4, seed=5)
    assert cfg.num_charge_states == expect
    assert cfg.struct_size == ctypes.sizeof(_lib.QdConfig)
    assert (cfg.n_dot, cfg.resolution, cfg.batch) == (8, 64, 4)


def test_qd_config_refuses_k_out_of_range():
    from qadapt_hip.vec_env import make_qd_config
    e = DM.load_yaml(None, "env_config.yaml")
    with pytest.raises(NotImplementedError, match="32"):
        make_qd_config(e, _qconfig(33), 4, 16, 2)


def _pixels(N, seeds, R=4):
    """v_ext of R x R pixels of channel 0 for devices drawn by the product's sampler, near and far from their
    ground truth."""
    eb = H.sample_blocks(N, seeds)
    rng = np.random.default_rng(N)
    out = []
    for e in range(len(seeds)):
        dev = H.dev_view(N, eb.params[e])
        sv = H.state_view(N, H.place(N, eb.state[e], ("near", "mid", "far")[e % 3], rng))
        vg = O.sweep_voltages(sv.vgm, dev.origin, sv.gate_v, sv.sensor_gt, 0, -dev.window, dev.window, R)
        vb = np.broadcast_to(np.asarray(sv.barrier_v, float), (R * R, N - 1))
        out.append((dev, np.concatenate([vg, vb], axis=1)))
    return out


@pytest.mark.parametrize("N", [2, 4, 6])
def test_first_k_of_the_32_list_is_the_literal_k_scan(N):
    """The kernels keep KC in {8, 16, 32} >= K states and hand over the first K of the (E, index)-sorted list: that is
    the reference's chunked k = K scan, padding included (K = 24 > 4^2 for two dots)."""
    for dev, v_ext in _pixels(N, [11, 12, 13]):
        full, _ = O.candidate_states(v_ext, dev.cdd_inv_full, dev.cgd_full, N, k=32)
        for K in (1, 8, 16, 24):
            lit, _ = O.candidate_states_literal(v_ext, dev.cdd_inv_full, dev.cgd_full, N, k=K)
            assert np.array_equal(full[:, :K], lit), (N, K)
            fast, _ = O.candidate_states(v_ext, dev.cdd_inv_full, dev.cgd_full, N, k=K)
            assert np.array_equal(fast, lit), (N, K)
