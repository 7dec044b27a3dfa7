"""Host-side checks of the running observation normaliser (include/ses.h: ses_obs_norm_bind): the merge and the
reduction order of the numpy restatement (tests/obs_norm_np.py) that the GPU tests hold the kernels to, the network module's
buffers, the builder's key and the configs.  No kernel is launched here."""
import copy
import os

import numpy as np
import pytest
import torch
import yaml

import obs_norm_np as on

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
U = 2.0 ** -53


def data_sets(n=10007):
    """name -> float32[n] (observations are float32): mean 0 / std 1, mean 100 / std 0.01, a constant"""
    rng = np.random.default_rng(5)
    return {"unit": rng.standard_normal(n).astype(np.float32),
            "offset": (100.0 + 0.01 * rng.standard_normal(n)).astype(np.float32),
            "constant": np.full(n, 0.3, np.float32)}


def merged_in_two(x, cut):
    """the statistics of x merged as two batches x[:cut], x[cut:] from the fresh state: (stats[1, 3], affine[2, 1])"""
    stats, affine = on.fresh(1)
    for part in (x[:cut], x[cut:]):
        stats, affine = on.merge(stats, affine, on.partials_of(part))
    return stats, affine


@pytest.mark.parametrize("name", ["unit", "offset", "constant"])
def test_merge_agrees_with_two_pass_mean_and_variance(name):
    """Two merged batches against the two-pass mean and M2 of the concatenation in longdouble, within 4 n u sum x^2 on M2 and
    that times 1 / n on the mean, u = 2^-53.
    Where the bound comes from: every input is a float32, so each x and each x^2 is exact in float64.  S1 and S2 are sums of
    n terms in a fixed order: |err(S2)| <= (n - 1) u sum x^2, |err(S1)| <= (n - 1) u sum |x|.  M2b = S2 - S1 * (S1 / n_b) adds
    three roundings of quantities bounded by sum x^2 (S1^2 / n_b <= sum x^2, Cauchy-Schwarz), and the error of S1 enters
    through 2 |S1| / n_b * err(S1) <= 2 (n - 1) u sum x^2 (|S1| sum |x| <= n_b sum x^2).  Merging two such batches adds a
    handful of roundings of terms that are themselves bounded by sum x^2: |err(M2)| <= (3 (n - 1) + c) u sum x^2 with c a small
    constant, which 4 n u sum x^2 covers for n >= 16.  The mean is S1 / n up to a few roundings: |err(mean)| <= (1 + 5 / n) u
    sum |x|, inside 4 u sum x^2 for data with sum |x| (1 + 5 / n) <= 4 sum x^2 -- the three sets here (asserted below)."""
    x = data_sets()[name]
    n = len(x)
    stats, affine = merged_in_two(x, 6000)
    xl = x.astype(np.longdouble)
    mean_ref = xl.sum() / n
    M2_ref = ((xl - mean_ref) ** 2).sum()
    sum_sq = float((xl * xl).sum())
    sum_abs = float(np.abs(xl).sum())
    tol_M2 = 4.0 * n * U * sum_sq
    tol_mean = tol_M2 / n
    assert sum_abs * (1.0 + 5.0 / n) <= 4.0 * sum_sq
    print(name, "n", n, "M2 err", float(abs(stats[0, 2] - M2_ref)), "tol", tol_M2, "mean err", float(abs(stats[0, 1] - mean_ref)), "tol",
          tol_mean)
    assert stats[0, 0] == n
    assert abs(stats[0, 2] - M2_ref) <= tol_M2
    assert abs(stats[0, 1] - mean_ref) <= tol_mean
    assert affine[0, 0] == np.float32(stats[0, 1])
    if name == "constant":
        assert affine[1, 0] == 0.0                                      # a component that never varies: ARS's std = inf
    else:
        std = np.sqrt(stats[0, 2] / (n - 1))
        assert affine[1, 0] == np.float32(1.0 / std) and affine[1, 0] > 0.0


def test_merge_edge_cases():
    # an empty batch leaves the state bit-identical, the affine included
    stats, affine = merged_in_two(data_sets()["unit"], 100)
    empty = np.zeros((3, 40), np.float64)
    s2, a2 = on.merge(stats, affine, empty)
    assert s2.tobytes() == stats.tobytes() and a2.tobytes() == affine.tobytes()
    assert on.merge_component(5.0, 1.0, 2.0, 0.0, 0.0, 0.0) is None
    # the first merge from the fresh state gives mean == S1 / n_b exactly
    x = data_sets()["offset"][:777]
    p = on.partials_of(x)
    S1, nb = on.reduce_envs(p[1]), on.reduce_envs(p[0])
    stats, affine = on.merge(*on.fresh(1), p)
    assert nb == 777.0 and stats[0, 0] == 777.0
    assert stats[0, 1] == S1 / nb
    # a constant component: scale 0, shift the constant
    stats, affine = on.merge(*on.fresh(1), on.partials_of(np.full(50, 0.25, np.float32)))
    assert affine[1, 0] == 0.0 and affine[0, 0] == np.float32(0.25) and stats[0, 2] == 0.0
    # one observation in all: N = 1, std = 1 by definition
    stats, affine = on.merge(*on.fresh(1), on.partials_of(np.array([3.0], np.float32)))
    assert stats[0, 0] == 1.0 and affine[1, 0] == 1.0 and affine[0, 0] == 3.0
    # std just below / above the floor of 1e-7
    for std, zero in ((0.99e-7, True), (1.01e-7, False)):
        M2 = np.float64(std) ** 2 * 9.0                                 # N = 8 + 2 = 10, the batch two observations of 0
        n_, mean_, M2_, shift, scale = on.merge_component(8.0, 0.0, M2, 2.0, 0.0, 0.0)
        assert (scale == 0.0) == zero, (std, scale)


def literal_reduction(x):
    """the order of the contract written out as a double loop, separately from obs_norm_np.reduce_envs"""
    lane = [np.float64(0.0)] * 256
    for l in range(256):
        e = l
        while e < len(x):
            lane[l] = lane[l] + np.float64(x[e])
            e += 256
    s = 128
    while s >= 1:
        for l in range(s):
            lane[l] = lane[l] + lane[l + s]
        s //= 2
    return lane[0]


@pytest.mark.parametrize("n_env", [1, 21, 255, 256, 257, 270])
def test_reduction_order(n_env):
    rng = np.random.default_rng(n_env)
    x = rng.standard_normal(n_env) * 10.0 ** rng.integers(-6, 7, n_env)     # magnitudes apart: the order shows in the bits
    got, want = on.reduce_envs(x), literal_reduction(x)
    assert np.float64(got).tobytes() == np.float64(want).tobytes()
    if n_env >= 255:
        assert got != np.sum(x[::-1]) or got != np.cumsum(x)[-1]          # (the data does tell orders apart)


# ---- the network module ---------------------------------------------------------------------------------------------------
REFERENCE_KEYS_MLP = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]


def test_module_buffers():
    from networks.neural_network import GymEnvModel
    plain = GymEnvModel(9, 2, False, False)
    assert list(plain.state_dict()) == REFERENCE_KEYS_MLP
    m = GymEnvModel(9, 2, False, False, obs_normalizer=True)
    keys = list(m.state_dict())                                         # (a module's own buffers come before its children's entries)
    assert [k for k in keys if k in REFERENCE_KEYS_MLP] == REFERENCE_KEYS_MLP
    assert sorted(set(keys) - set(REFERENCE_KEYS_MLP)) == ["obs_norm_scale", "obs_norm_shift", "obs_norm_stats"] and len(keys) == 7
    assert m.obs_norm_shift.dtype == torch.float32 and tuple(m.obs_norm_shift.shape) == (9,) and not m.obs_norm_shift.any()
    assert m.obs_norm_scale.dtype == torch.float32 and tuple(m.obs_norm_scale.shape) == (9,) and (m.obs_norm_scale == 1).all()
    assert m.obs_norm_stats.dtype == torch.float64 and tuple(m.obs_norm_stats.shape) == (9, 3) and not m.obs_norm_stats.any()
    # buffers are not parameters
    assert m.param_count() == plain.param_count() == 386
    assert len(m.get_param_list()) == len(plain.get_param_list()) == 4
    vec = np.arange(386, dtype=np.float32)
    assert np.array_equal(m.load_flat(vec).flat(), vec)
    affine = np.stack([np.linspace(-1, 1, 9), np.linspace(0.5, 3, 9)]).astype(np.float32)
    stats = np.arange(27, dtype=np.float64).reshape(9, 3)
    m.set_obs_norm(affine, stats)
    m.zero_init()
    assert not m.flat().any()
    assert np.array_equal(m.obs_norm_affine(), affine) and np.array_equal(m.obs_norm_stats.numpy(), stats)   # zero_init leaves them
    c = copy.deepcopy(m)
    assert np.array_equal(c.obs_norm_affine(), affine) and np.array_equal(c.obs_norm_stats.numpy(), stats)
    # a normalised checkpoint does not load into a plain module, and a plain one not into a normalised module
    with pytest.raises(RuntimeError):
        plain.load_state_dict(m.state_dict())
    with pytest.raises(RuntimeError):
        m.load_state_dict(plain.state_dict())
    m2 = GymEnvModel(9, 2, False, False, obs_normalizer=True)
    m2.load_state_dict(m.state_dict())
    assert np.array_equal(m2.obs_norm_affine(), affine) and m2.obs_norm_stats.dtype == torch.float64
    with pytest.raises(ValueError):
        GymEnvModel(9, 2, False, True, obs_normalizer=True)


# ---- builder and configs ----------------------------------------------------------------------------------------------------
def net_cfg(**kw):
    cfg = dict(name="gym_model", num_state=3, num_action=1, discrete_action=False, gru=False)
    cfg.update(kw)
    return cfg


def test_builder_reads_the_key():
    import builder
    assert not builder.build_network(net_cfg()).obs_normalizer
    assert not builder.build_network(net_cfg(obs_normalizer=False), "Pendulum-v1").obs_normalizer
    assert builder.build_network(net_cfg(obs_normalizer=True), "Pendulum-v1").obs_normalizer
    assert len(builder.OBS_NORMALIZER_ENVS) == 8
    with pytest.raises(ValueError, match="gru"):
        builder.build_network(net_cfg(obs_normalizer=True, gru=True), "Pendulum-v1")
    with pytest.raises(ValueError, match="CartPole-v1"):
        builder.build_network(net_cfg(obs_normalizer=True, num_state=4, num_action=2, discrete_action=True), "CartPole-v1")


@pytest.mark.skipif(torch.cuda.is_available(), reason="build_loop creates device handles on a GPU box; the GPU suite covers it there")
def test_build_loop_refuses_before_touching_a_device():
    import builder
    cfg = {"env": {"name": "CartPole-v1", "max_step": 500, "pomdp": False},
           "network": net_cfg(obs_normalizer=True, num_state=4, num_action=2, discrete_action=True),
           "strategy": {"name": "openai_es", "init_sigma": 0.1, "sigma_decay": 0.999, "learning_rate": 0.05, "offspring_num": 16}}
    with pytest.raises(ValueError, match="CartPole-v1"):
        builder.build_loop(cfg, 1, 1, 1, False, 1)


@pytest.mark.parametrize("new, base", [("reacher_ars_v2.yaml", "reacher_ars.yaml"), ("pendulum_swingup_ars_v2.yaml", "pendulum_swingup_ars.yaml"),
                                       ("reacher_openai_norm.yaml", "reacher.yaml")])
def test_configs_are_the_base_config_plus_the_key(new, base):
    import builder
    cfg = yaml.load(open(os.path.join(SRC, "conf", new)), Loader=yaml.FullLoader)
    ref = yaml.load(open(os.path.join(SRC, "conf", base)), Loader=yaml.FullLoader)
    assert cfg["network"].pop("obs_normalizer") is True
    assert cfg == ref
    cfg["network"]["obs_normalizer"] = True
    net = builder.build_network(cfg["network"], cfg["env"]["name"])
    assert net.obs_normalizer and cfg["env"]["name"] in builder.OBS_NORMALIZER_ENVS
    strategy = builder.build_strategy(cfg["strategy"])
    assert type(strategy).__name__ == cfg["strategy"]["name"]


def test_sweep_runs_normalised_configs_sequentially():
    """--concurrent R: a config with the key gets no batch key, so its trials run one after the other"""
    src = open(os.path.join(SRC, "sweep_main.py")).read()
    assert 'config.get("network", {}).get("obs_normalizer", False)' in src
