"""LunarLander-v2 without a GPU: the Python rollout the GPU tests compare against (tests/lander_discrete_np.py) is held to the
C oracle where the two overlap, its discrete inputs are shown to reach every action and both ways an episode ends, and the host
surface (names, configs, the head / name pairing) is in place."""
import os

import numpy as np
import pytest
import yaml

import lander_discrete_np as ld
from oracle import c_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")


@pytest.mark.parametrize("gru,pomdp", [(False, False), (False, True), (True, False), (True, True)])
def test_harness_in_continuous_mode_equals_the_c_oracle(gru, pomdp):
    n, E, max_step = 20, 3, 120
    theta, init = ld.population(gru, pomdp, n, E)
    mask = ld.POMDP_MASK if pomdp else 0
    fit, ret, steps, _ = ld.rollout(theta, init, E, max_step, gru, mask, discrete=False)
    o_fit, o_ret, o_steps = co.rollout_lander(theta, init, E, max_step, gru=gru, obs_mask=mask)
    assert np.array_equal(steps, o_steps)
    assert np.array_equal(ret.view(np.uint64), o_ret.view(np.uint64))
    assert np.array_equal(fit.view(np.uint32), o_fit.view(np.uint32))


@pytest.mark.parametrize("E", [3, 5])
@pytest.mark.parametrize("gru,pomdp", [(False, False), (False, True), (True, False), (True, True)])
def test_discrete_inputs_exercise_every_path(gru, pomdp, E):
    _theta, _init, fit, ret, steps, hist = ld.reference(gru, pomdp, E)
    share = hist / hist.sum()
    early = (steps < 120).mean()
    print(f"gru={gru} pomdp={pomdp} E={E}: action shares {share.round(3)}, ended before the cap {early:.3f}, "
          f"lowest return {ret.min():.1f}, distinct fitness {len(set(fit.tolist()))}")
    assert hist.sum() == steps.sum()
    assert share.min() >= 0.05, share
    assert 0.50 <= early <= 0.97, early
    assert ret.min() < -100.0
    assert len(set(fit.tolist())) == 22


@pytest.mark.parametrize("gru", [False, True])
def test_zero_theta_never_fires_an_engine(gru):
    """all-equal logits: the first maximum wins, which is action 0, the no-op"""
    theta = np.zeros(co.param_count(8, 4, gru), np.float32)
    init = co.init_states_uniform(11, 2, 50, 1, 2, 16, False, 0.0, 1.0)
    sim = co.LanderSim()
    for e in range(2):
        trace = []
        ld.episode(sim, theta, init[0, e], 120, gru, 0, True, trace)
        assert trace and all(a == 0 for a, _ in trace)


def test_names_configs_and_the_head_pairing():
    from envs.gym_wrapper import SUPPORTED
    from ses import HipES, SesError
    from ses.device import ENV_IDS
    import builder
    assert SUPPORTED["LunarLander-v2"] == dict(num_state=8, num_action=4, discrete=True, time_limit=1000)
    assert ENV_IDS["LunarLander-v2"] == ENV_IDS["LunarLanderContinuous-v2"]
    for name, gru, pomdp, strategy in (("lunarlander_v2", False, False, "simple_evolution"),
                                       ("lunarlander_v2_openai", True, True, "openai_es")):
        cfg = yaml.load(open(os.path.join(SRC, "conf", name + ".yaml")), Loader=yaml.FullLoader)
        assert cfg["env"] == {"name": "LunarLander-v2", "max_step": 300, "pomdp": pomdp}
        assert cfg["strategy"]["name"] == strategy
        env = builder.build_env(cfg["env"])
        assert (env.name, env.horizon, env.pomdp, env.variant) == ("LunarLander-v2", 300, pomdp, "box2d-restated")
        net = builder.build_network(cfg["network"])
        assert (net.num_state, net.num_action, net.discrete_action, net.use_gru) == (8, 4, True, gru)
        assert net.param_count() == co.param_count(8, 4, gru)
    # a name that contradicts the head is refused on the host, before any device is asked for
    with pytest.raises(SesError, match="LunarLander-v2 takes discrete_action=True"):
        HipES("LunarLander-v2", 8, 4, False, False)
    with pytest.raises(SesError, match="LunarLanderContinuous-v2 takes discrete_action=False"):
        HipES("LunarLanderContinuous-v2", 8, 4, True, True)
