"""Walker2DBulletEnv-v0 on the HIP path (csrc/ses_walker2d.hip) against the host build of the same env text (tests/walker2d_host.py), bit
for bit: the step-wise env, the fused MLP rollout at every lanes-per-env setting and with the envs per wave forced, the GRU rollout,
the device loop against per-generation calls, the wrapper's playback, and the refusals.

The horizon of the rollout tests is 60 steps.  Episode 1 of every offspring starts from the zero init row, from which the zero
policy is still standing at step 60 (it falls at 67); episode 0 starts from a row of the full range, from which it falls after
34 - 44 steps; random policies fall within 4 - 40.  So the zero population's 14 episodes hold both capped and early-ended ones;
the fixtures assert it on the host."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import walker2d_host as wh
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = wh.NAME
T = 60


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def handle(gru=False, E=1, max_step=T):
    from ses import HipES
    return HipES(NAME, wh.S, wh.A, False, gru, max_step=max_step, eval_ep_num=E)


def init_rows(seed, n, E):
    """[n, E, 6] rows of the env's init stream; episode 1 of every offspring starts from the zero row (module docstring)"""
    init = co.init_states_uniform(seed, 0, 0, n, E, wh.INIT_W, False, -0.1, 0.1)
    init[:, 1, :] = 0.0
    return init


@pytest.fixture(scope="module")
def mlp_reference():
    """theta = zeros and theta ~ N(0, 1), 7 offspring x 2 episodes: the host's (fitness, returns, lengths), computed once"""
    P = co.param_count(wh.S, wh.A, False)
    init = init_rows(3, 7, 2)
    thetas = {"zeros": np.zeros((7, P), np.float32), "normal": np.random.default_rng(3).standard_normal((7, P)).astype(np.float32)}
    want = {k: wh.rollout(th, init, 2, T) for k, th in thetas.items()}
    steps = want["zeros"][2]
    assert (steps == T).any() and (steps < T).any(), steps                  # capped and early-ended episodes among the 14
    assert (want["normal"][2] < T).all() and len(np.unique(want["normal"][1])) == 14
    return init, thetas, want


def test_stepwise_env_equals_the_host_build():
    es = handle()
    n = 5
    assert es.env_state_bytes() == wh.lib().w2d_state_size() and es.env_obs_width() == 22 and es.init_dim == 6
    init = es.init_states_uniform(9, 0, 0, n)[:, 0].contiguous()
    want_init = co.init_states_uniform(9, 0, 0, n, 1, 6, False, -0.1, 0.1)[:, 0]
    assert np.array_equal(bits(init.cpu().numpy()), bits(want_init))
    state, obs = es.env_reset(init)
    sims = [wh.Walker2dSim() for _ in range(n)]
    w_obs = np.stack([s.reset(want_init[i]) for i, s in enumerate(sims)])
    assert np.array_equal(bits(obs.cpu().numpy()), bits(w_obs))
    rng = np.random.default_rng(9)
    first_done = [None] * n
    feet_differ = 0
    for t in range(40):
        a = rng.uniform(-1.0, 1.0, (n, 6)).astype(np.float32)
        a[0] *= 0.01                                                        # one env stays up for 30 steps or more, four thrash and fall
        a[1, 3:] = 0.0                                                      # one env is driven on its right leg only
        obs, reward, done = es.env_step_generic(state, dev(a))
        w = [s.step(a[i]) for i, s in enumerate(sims)]
        assert np.array_equal(bits(obs.cpu().numpy()), bits(np.stack([x[0] for x in w]))), t
        assert np.array_equal(bits(reward.cpu().numpy()), bits(np.array([x[1] for x in w], np.float32))), t
        assert np.array_equal(done.cpu().numpy() != 0, np.array([x[2] for x in w])), t
        first_done = [t + 1 if (f is None and x[2]) else f for f, x in zip(first_done, w)]
        feet_differ += sum(int(x[0][20] != x[0][21]) for x in w)
    # (the comparison runs on through and past the falls)
    assert feet_differ > 0                                                  # the second foot's contact path was compared, not two equal flags
    assert all(f is not None and f < 25 for f in first_done[1:]) and (first_done[0] is None or first_done[0] > 25), first_done
    es.close()


SHAPES = [("box2d_lanes_per_env", lpe) for lpe in (1, 2, 4, 8, 16, 32, 64)] + [("box2d_envs_per_wave", 1), ("box2d_envs_per_wave", 3), (None, 0)]


@pytest.mark.parametrize("knob,value", SHAPES, ids=[f"{k}={v}" for k, v in SHAPES])
def test_mlp_rollout_equals_the_host_build(mlp_reference, knob, value):
    """7 offspring x 2 episodes = 14 envs: an odd count, so the last lane group of the last wave shadows."""
    init, thetas, want = mlp_reference
    es = handle(False, 2)
    if knob:
        es.set_tuning(knob, value)
    for key, theta in thetas.items():
        fit, ep_ret, ep_steps = es.rollout(dev(theta), dev(init), want_episodes=True)
        w_fit, w_ret, w_steps = want[key]
        assert np.array_equal(ep_steps.cpu().numpy(), w_steps), (key, ep_steps.cpu().numpy(), w_steps)
        assert np.array_equal(bits(ep_ret.cpu().numpy()), bits(w_ret)), key
        assert np.array_equal(bits(fit.cpu().numpy()), bits(w_fit)), key
    es.close()


def test_gru_rollout_equals_the_host_build():
    P = co.param_count(wh.S, wh.A, True)
    rng = np.random.default_rng(0)
    theta = np.concatenate([np.zeros((1, P), np.float32), (rng.standard_normal((4, P)) * 0.3).astype(np.float32)])
    init = init_rows(0, 5, 2)
    w_fit, w_ret, w_steps = wh.rollout(theta, init, 2, T, gru=True)
    assert (w_steps == T).any() and (w_steps < T).any(), w_steps
    es = handle(True, 2)
    fit, ep_ret, ep_steps = es.rollout(dev(theta), dev(init), want_episodes=True)
    assert np.array_equal(ep_steps.cpu().numpy(), w_steps), (ep_steps.cpu().numpy(), w_steps)
    assert np.array_equal(bits(ep_ret.cpu().numpy()), bits(w_ret))
    assert np.array_equal(bits(fit.cpu().numpy()), bits(w_fit))
    es.close()


def test_device_loop_equals_three_per_generation_calls(tmp_path, monkeypatch):
    """openai_es, 8 offspring, three generations through ses_run_generations and generation by generation: identical histories,
    populations and elites."""
    import builder
    monkeypatch.chdir(tmp_path)
    cfg = {"env": {"name": NAME, "max_step": T, "pomdp": False, "seed": 3},
           "network": {"name": "gym_model", "num_state": 22, "num_action": 6, "discrete_action": False, "gru": False},
           "strategy": {"name": "openai_es", "init_sigma": 0.2, "sigma_decay": 0.999, "learning_rate": 0.05, "offspring_num": 8, "seed": 1}}
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SES_BATCH_GENERATIONS", mode)
        loop = builder.build_loop(cfg, 3, 1, 2, False, 10 ** 9)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            pop = loop.run()
        assert "pybullet-restated" in out.getvalue()
        runs[mode] = (list(loop.history), pop.theta.cpu().numpy(), loop.offspring_strategy.get_elite_model().flat())
    (h0, t0, m0), (h1, t1, m1) = runs["0"], runs["1"]
    assert len(h0) == 3 and h0 == h1
    assert np.array_equal(bits(t0), bits(t1)) and np.array_equal(bits(m0), bits(m1))


def test_wrapper_playback_equals_the_host_build_and_the_fused_rollout():
    from envs.gym_wrapper import GymWrapper
    from learning_strategies.evolution.loop import RolloutWorker
    from networks.neural_network import GymEnvModel
    env = GymWrapper(NAME, T)
    es = handle(False, 1, T)
    want_init = co.init_states_uniform(0, 0, 0, 1, 1, 6, False, -0.1, 0.1)[0, 0]
    sim = wh.Walker2dSim()
    obs = env.reset()["0"]["state"]
    assert np.array_equal(bits(obs), bits(sim.reset(want_init)))
    rng = np.random.default_rng(2)
    for t in range(T):
        a = (rng.uniform(-1.0, 1.0, 6) * 0.02).astype(np.float32)
        tr, r, done, _ = env.step({"0": a})
        w_obs, w_r, w_done = sim.step(a)
        assert np.array_equal(bits(tr["0"]["state"]), bits(w_obs)) and np.float32(r) == w_r, t
        assert done == (w_done or t + 1 >= T), t
        if done:
            break
    assert t > 20
    net = GymEnvModel(22, 6, False, False)
    net.load_flat((np.random.default_rng(6).standard_normal(co.param_count(22, 6, False)) * 0.1).astype(np.float32))
    k = env._episode
    got = RolloutWorker((env, {"0": net}, 1))
    init = es.init_states_uniform(0, k, 0, 1)
    fit, _, _ = es.rollout(dev(net.flat()[None, :]), init, want_episodes=True)
    assert got == float(fit[0].item())
    w_fit, _, _ = wh.rollout(net.flat()[None, :], init.cpu().numpy(), 1, T)
    assert np.float32(got) == w_fit[0]
    with pytest.raises(NotImplementedError, match="CartPole"):               # no scene: the message names the envs that have one
        env.render()
    es.close()
    env.close()


def test_refusals_are_by_name():
    from envs.gym_wrapper import GymWrapper
    from ses import HipES, SesError
    from ses._lib import MODE_FIXED_LENGTH
    for bad, word in ((dict(num_state=21), "num_state"), (dict(num_state=23), "num_state"), (dict(num_action=5), "num_action"),
                      (dict(discrete_action=True), "discrete_action"), (dict(pomdp=True), "pomdp"), (dict(physics64=True), "physics64")):
        kw = dict(num_state=22, num_action=6, discrete_action=False, gru=False, max_step=10, eval_ep_num=1)
        kw.update(bad)
        with pytest.raises(SesError, match="Walker2DBulletEnv-v0.*" + word):
            HipES(NAME, **kw)
    with pytest.raises(AssertionError):
        GymWrapper(NAME, None, pomdp=True)
    for gru in (False, True):
        es = handle(gru)
        theta = dev(np.zeros((2, co.param_count(22, 6, gru)), np.float32))
        init = es.init_states_uniform(1, 0, 0, 1, shared=True)[0].contiguous()
        with pytest.raises(SesError, match="Walker2DBulletEnv-v0 has no fixed-length mode"):
            es.rollout(theta, init, mode=MODE_FIXED_LENGTH)
        es.close()
