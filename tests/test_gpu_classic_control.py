"""Acrobot-v1 and MountainCar-v0 on the HIP path (csrc/ses_f64_envs.hip), held bit for bit to the independent numpy float64
restatement in tests/classic_control_np.py: single transitions (ses_env_step_generic) on random and crafted states, fused
MLP / GRU rollouts against a host loop of that env plus the oracle's policy forward, the reference's playback loop on the
wrappers, and the training loop on both of its paths."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import classic_control_np as cc
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("Acrobot-v1", "MountainCar-v0")
# max_step below the TimeLimit; (observation, gain) that the hand-built policies push with (Acrobot: torque along dtheta2,
# pumps energy into the chain; MountainCar: push along the velocity)
CASE = {"Acrobot-v1": dict(T=300, feat=(5, 8.0)), "MountainCar-v0": dict(T=180, feat=(1, 2000.0))}
LANES = (0, 1, 2, 4, 8, 16, 32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def handle(name, gru=False, E=1, T=None, lanes=0):
    from ses import HipES
    e = cc.ENVS[name]
    return HipES(name, e["S"], e["A"], True, gru, max_step=T or CASE[name]["T"], eval_ep_num=E, lanes_per_env=lanes)


# ---- single transitions ------------------------------------------------------------------------------------------------------
def crafted_states(name):
    pi = np.pi
    if name == "Acrobot-v1":
        rows = []
        edges = [pi, -pi, np.nextafter(pi, 4.0), np.nextafter(-pi, -4.0), np.nextafter(pi, 0.0), np.nextafter(-pi, 0.0)]
        for t in edges:                                                 # theta at +-pi, on both sides of the wrap
            for w in (0.0, 3.0, -3.0):
                rows += [(t, 0.0, w, 0.0), (0.0, t, 0.0, w), (t, t, w, -w)]
        v1, v2 = 4 * pi, 9 * pi                                        # the velocity bounds, at and beyond
        for w1, w2 in ((v1, 0.0), (-v1, 0.0), (0.0, v2), (0.0, -v2), (v1 * 1.5, v2 * 1.5), (-v1 * 1.5, -v2 * 1.5),
                       (np.nextafter(v1, 99.0), np.nextafter(v2, 99.0)), (v1 - 0.01, v2 - 0.01)):
            rows += [(0.3, -0.2, w1, w2), (2.0, 1.0, w1, -w2)]
        for d1 in np.linspace(-0.3, 0.3, 13):                          # straddling -cos th1 - cos(th2 + th1) = 1
            for d2 in np.linspace(-0.4, 0.4, 9):
                rows.append((pi + d1, pi / 2 + d2, 0.0, 0.0))
                rows.append((pi + d1, -pi / 2 + d2, 0.5, -0.5))
        return np.array(rows, np.float64)
    rows = [(-1.2, -0.07), (-1.2, -0.01), (-1.2, 0.0), (-1.19, -0.02), (-1.2, 0.001), (-1.1999, -0.0005),   # the left wall
            (0.0, 0.07), (0.0, -0.07), (0.0, 0.0699), (-0.5, 0.08), (-0.5, -0.08), (0.1, np.nextafter(0.07, 1.0)),   # speed clip
            (0.49, 0.01), (0.49, 0.0099), (0.5, 0.0), (0.5, -0.001), (0.499, 0.001), (0.5, 0.0025), (0.6, 0.07),     # p crossing 0.5
            (0.45, 0.05), (0.55, -0.06)]
    return np.array(rows, np.float64)


def random_states(name, n, rng):
    if name == "Acrobot-v1":
        lim = np.array([np.pi + 0.5, np.pi + 0.5, 4 * np.pi * 1.2, 9 * np.pi * 1.2])
        return rng.uniform(-1.0, 1.0, (n, 4)) * lim
    return np.stack([rng.uniform(-1.25, 0.65, n), rng.uniform(-0.08, 0.08, n)], axis=1)


def step_and_compare(es, name, states, action):
    n = states.shape[0]
    blob = dev(np.ascontiguousarray(states).view(np.uint8).reshape(n, -1))
    obs, reward, done = es.env_step_generic(blob, dev(action.astype(np.int32)))
    ns, w_obs, w_r, w_d = cc.ENVS[name]["step"](states.T, action)
    got_state = blob.cpu().numpy().view(np.float64).reshape(n, -1)
    assert np.array_equal(bits(got_state), bits(ns.T.copy())), (name, np.argwhere(bits(got_state) != bits(ns.T.copy()))[:5])
    assert np.array_equal(bits(obs.cpu().numpy()), bits(w_obs))
    assert np.array_equal(bits(reward.cpu().numpy()), bits(w_r))
    assert np.array_equal(done.cpu().numpy().astype(bool), w_d)
    return w_d


@pytest.mark.parametrize("name", NAMES)
def test_reset_is_the_widened_init_row(name):
    es = handle(name)
    e = cc.ENVS[name]
    init = es.init_states_uniform(5, 2, 0, 300)[:, 0].contiguous()
    assert es.init_range == e["init_range"] and es.init_dim == e["init_dim"]
    want_init = co.init_states_uniform(5, 2, 0, 300, 1, e["init_dim"], False, *e["init_range"])[:, 0]
    assert np.array_equal(bits(init.cpu().numpy()), bits(want_init))
    state, obs = es.env_reset(init)
    assert es.env_state_bytes() == 8 * e["state_dim"] and es.env_obs_width() == e["S"]
    s = e["reset"](want_init)
    assert np.array_equal(bits(state.cpu().numpy().view(np.float64)), bits(s.T.copy()))
    assert np.array_equal(bits(obs.cpu().numpy()), bits(e["obs"](s)))
    es.close()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", [1, 4133])
def test_transitions_are_bit_exact(name, n):
    es = handle(name)
    rng = np.random.default_rng(n)
    edges = crafted_states(name)
    if n == 1:
        sets = [edges[i:i + 1] for i in range(0, len(edges), max(1, len(edges) // 12))]
    else:
        sets = [np.concatenate([edges, random_states(name, n - len(edges), rng)])]
    dones = []
    for states in sets:
        for a in range(3):
            dones.append(step_and_compare(es, name, states, np.full(states.shape[0], a)))
        dones.append(step_and_compare(es, name, states, rng.integers(0, 3, states.shape[0])))
    if n > 1:
        d = np.concatenate(dones)
        assert d.any() and not d.all()                                  # both sides of the terminal condition are hit
        # several steps in a row from the same states: the state carried in the blob is the float64 one
        states = sets[0]
        for t in range(20):
            ns, _, _, _ = cc.ENVS[name]["step"](states.T, np.full(n, t % 3))
            step_and_compare(es, name, states, np.full(n, t % 3))
            states = ns.T.copy()
    es.close()


# ---- fused rollouts ------------------------------------------------------------------------------------------------------------
def hand_built(name, gru, rng, noise):
    """A policy that finishes early: logit 2 - logit 0 follows tanh(gain * obs[f]) (through the GRU's n gate with z shut)."""
    e = cc.ENVS[name]
    S, A = e["S"], e["A"]
    f, gain = CASE[name]["feat"]
    th = np.zeros(co.param_count(S, A, gru), np.float32)
    th[f] = gain                                                        # fc1 unit 0 <- obs[f]
    off = 32 * S + 32
    if gru:
        wih, whh = off, off + 96 * 32
        bih, bhh = whh + 96 * 32, whh + 96 * 32 + 96
        th[bih + 32] = -30.0                                            # z of unit 0 shut: h' = n
        th[wih + 64 * 32] = 5.0                                         # n of unit 0 <- a_0
        off = bhh + 96
    th[off + 2 * 32] = 3.0
    th[off] = -3.0
    return th + (rng.standard_normal(th.shape) * noise).astype(np.float32)


def population(name, gru, n, rng):
    P = co.param_count(cc.ENVS[name]["S"], 3, gru)
    rows = []
    for i in range(n):
        if i % 4 == 3:                                                  # a random policy in every fourth row
            rows.append((rng.standard_normal(P) * rng.choice([0.1, 0.5, 1.5])).astype(np.float32))
        else:
            rows.append(hand_built(name, gru, rng, 0.0 if i == 0 else 0.02))
    return np.stack(rows)


def oracle_rollout(name, gru, theta, init, E, T):
    S = cc.ENVS[name]["S"]

    def policy(th, obs, h):
        action, _, _, hn = co.policy_forward(S, 3, True, gru, th, obs, h)
        return action, hn

    return cc.rollout(name, theta, init, E, T, policy)


_ORACLE = {}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("gru", [False, True], ids=["mlp", "gru"])
@pytest.mark.parametrize("E", [1, 5, 8])
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "own"])
@pytest.mark.parametrize("n", [1, 63, 1000])
def test_fused_rollout_is_bit_exact(name, gru, E, shared, n):
    """Every accepted lanes_per_env (MLP; 0 = the library's choice) against one host loop of the checker env + the oracle's
    policy forward: per-episode return, length and fitness bit for bit."""
    T = CASE[name]["T"]
    rng = np.random.default_rng(n * 100 + E * 10 + int(gru) * 2 + int(shared))
    theta = population(name, gru, n, rng)
    es = handle(name, gru, E, T)
    init = es.init_states_uniform(11, 3, 40, 1 if shared else n, shared=shared)
    init_dev = init[0].contiguous() if shared else init
    w_fit, w_ret, w_steps = oracle_rollout(name, gru, theta, init.cpu().numpy(), E, T)
    assert (w_steps < T).mean() >= 0.25, (w_steps < T).mean()          # the env's own termination, not only the cap
    es.close()
    for lanes in (LANES if not gru else (0,)):
        es = handle(name, gru, E, T, lanes)
        fit, ep_ret, ep_steps = es.rollout(dev(theta), init_dev, want_episodes=True)
        assert np.array_equal(ep_steps.cpu().numpy(), w_steps), lanes
        assert np.array_equal(bits(ep_ret.cpu().numpy()), bits(w_ret)), lanes
        assert np.array_equal(bits(fit.cpu().numpy()), bits(w_fit)), lanes
        es.close()


@pytest.mark.parametrize("name", NAMES)
def test_fixed_length_mode_is_refused(name):
    from ses import SesError
    from ses._lib import MODE_FIXED_LENGTH
    es = handle(name)
    theta = dev(population(name, False, 2, np.random.default_rng(0)))
    init = es.init_states_uniform(1, 0, 0, 1, shared=True)[0].contiguous()
    with pytest.raises(SesError):
        es.rollout(theta, init, mode=MODE_FIXED_LENGTH)
    es.close()


# ---- playback and training --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["acrobot", "mountaincar"])
def test_the_reference_playback_loop_runs_on_the_wrappers(name):
    """The reference's test.py loop over the wrapper (one transition per launch) against the fused rollout kernel fed the
    same reset rows: identical episode lengths and returns."""
    import yaml
    import builder
    from test_gpu_envs import playback
    cfg = yaml.load(open(os.path.join(ROOT, "simple-es_amd", "conf", name + ".yaml")), Loader=yaml.FullLoader)
    env = builder.build_env(cfg["env"])
    net = builder.build_network(cfg["network"])
    net.load_flat(hand_built(env.name, False, np.random.default_rng(1), 0.05))
    episodes = 3
    got = playback(env, net, episodes)
    es = handle(env.name, False, 1, env.horizon)
    for k, (ret, steps) in enumerate(got):
        init = es.init_states_uniform(0, k, 0, 1)
        _, ep_ret, ep_steps = es.rollout(dev(net.flat()[None, :]), init, want_episodes=True)
        assert int(ep_steps[0, 0]) == steps and float(ep_ret[0, 0]) == ret, (k, got, ep_ret, ep_steps)
    assert any(steps < env.horizon for _, steps in got)
    es.close()
    env.close()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("strategy", ["openai_es", "simple_evolution"])
def test_training_loop_paths_agree(tmp_path, monkeypatch, name, strategy):
    """Three generations per-generation (SES_BATCH_GENERATIONS=0) and through ses_run_generations: identical populations."""
    import builder
    monkeypatch.chdir(tmp_path)
    e = cc.ENVS[name]
    cfg = {"env": {"name": name, "max_step": CASE[name]["T"], "pomdp": False, "seed": 3},
           "network": {"name": "gym_model", "num_state": e["S"], "num_action": 3, "discrete_action": True, "gru": False},
           "strategy": {"name": strategy, "init_sigma": 0.5, "sigma_decay": 0.99, "learning_rate": 0.05, "elite_num": 5,
                        "offspring_num": 48, "seed": 1}}
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SES_BATCH_GENERATIONS", mode)
        loop = builder.build_loop(cfg, 3, 1, 2, False, 10 ** 9)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            pop = loop.run()
        assert "classic-control-restated" in out.getvalue()
        runs[mode] = (list(loop.history), pop.theta.cpu().numpy(), loop.offspring_strategy.get_elite_model().flat())
    (h0, t0, m0), (h1, t1, m1) = runs["0"], runs["1"]
    assert len(h0) == 3 and h0 == h1
    assert np.array_equal(bits(t0), bits(t1)) and np.array_equal(bits(m0), bits(m1))
