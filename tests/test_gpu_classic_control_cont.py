"""Pendulum-v1 and MountainCarContinuous-v0 on the HIP path (csrc/ses_f64_envs.hip), held bit for bit to the independent
numpy float64 restatement in tests/classic_control_cont_np.py: single transitions (ses_env_step_generic) on random and crafted
states and actions, fused MLP / GRU rollouts against a host loop of that env plus the oracle's policy forward (its tanh
`act`), the reference's playback loop on the wrappers, and the training loop on both of its paths."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import classic_control_cont_np as ccc
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("Pendulum-v1", "MountainCarContinuous-v0")
# max_step of the rollout tests; (observation, gain) of the hand-built policies a = tanh(gain * obs[f]): Pendulum pushes along
# the angular velocity (pumps energy, drives the speed into the +-8 clip), MountainCarContinuous along the velocity (reaches
# the goal in ~80 steps)
CASE = {"Pendulum-v1": dict(T=150, feat=(2, 4.0)), "MountainCarContinuous-v0": dict(T=300, feat=(1, 2000.0))}
LANES = (0, 1, 2, 4, 8, 16, 32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def handle(name, gru=False, E=1, T=None, lanes=0):
    from ses import HipES
    e = ccc.ENVS[name]
    return HipES(name, e["S"], 1, False, gru, max_step=T or CASE[name]["T"], eval_ep_num=E, lanes_per_env=lanes)


# ---- single transitions ------------------------------------------------------------------------------------------------------
def crafted(name):
    """(states float64[m, 2], actions float32[m]): every crafted state with every crafted action"""
    pi = np.pi
    if name == "Pendulum-v1":
        ths = []
        for k in range(-13, 14):                                       # th + pi at and on both sides of multiples of 2 pi
            t = 2 * pi * k - pi
            ths += [t, np.nextafter(t, 100.0), np.nextafter(t, -100.0), t + 1e-9, t - 1e-9]
        ths += [0.0, -0.0, pi, -pi, 0.5 * pi, -0.5 * pi, 1.0, -1.0, -2.5, -7.0, -40.0, 40.0, 65.0, -65.0, 83.9, -83.9, 84.0, -84.0]
        ws = [0.0, -0.0, 8.0, -8.0, 7.99, -7.99, np.nextafter(8.0, 9.0), np.nextafter(-8.0, -9.0), 9.5, -9.5, 1.0, -3.0]
        acts = [0.0, -0.0, 1.0, -1.0, 2.0, -2.0, np.nextafter(np.float32(2.0), np.float32(3.0)),
                np.nextafter(np.float32(-2.0), np.float32(-3.0)), 2.5, -2.5, 7.0, -7.0, 0.3, -1.7]
        states = np.array([(t, w) for t in ths for w in ws], np.float64)
    else:
        states = np.array([(-1.2, -0.07), (-1.2, -0.01), (-1.2, 0.0), (-1.19, -0.02), (-1.2, 0.001), (-1.1999, -0.0005),   # the left wall
                           (-1.15, -0.07), (-1.25, -0.03),
                           (0.0, 0.07), (0.0, -0.07), (0.0, 0.0699), (-0.5, 0.08), (-0.5, -0.08), (0.1, np.nextafter(0.07, 1.0)),  # speed clip
                           (0.44, 0.01), (0.44, 0.0099), (0.45, 0.0), (0.45, -0.001), (0.449, 0.001), (0.4499, 0.0001),           # p crossing 0.45
                           (0.46, -0.0005), (0.47, -0.03), (0.43, 0.03), (0.5, -0.06), (0.448, 0.002),
                           (0.59, 0.07), (0.6, 0.07), (0.6, -0.07), (0.58, 0.03), (0.65, 0.01)], np.float64)                   # p clipped at 0.6
        acts = [0.0, -0.0, 1.0, -1.0, np.nextafter(np.float32(1.0), np.float32(2.0)), np.nextafter(np.float32(-1.0), np.float32(-2.0)),
                1.5, -1.5, 4.0, -4.0, 0.5, -0.25]
    acts = np.array(acts, np.float32)
    return np.repeat(states, len(acts), axis=0), np.tile(acts, len(states))


def random_cases(name, n, rng):
    if name == "Pendulum-v1":
        states = np.stack([rng.uniform(-84.0, 84.0, n), rng.uniform(-9.0, 9.0, n)], axis=1)
        return states, rng.uniform(-2.6, 2.6, n).astype(np.float32)
    # MountainCarContinuous keeps its state float32-representable; arbitrary float64 states are legal blobs too: half of each
    states = np.stack([rng.uniform(-1.25, 0.65, n), rng.uniform(-0.08, 0.08, n)], axis=1)
    half = n // 2
    states[:half] = states[:half].astype(np.float32).astype(np.float64)
    return states, rng.uniform(-1.4, 1.4, n).astype(np.float32)


def step_and_compare(es, name, states, action):
    n = states.shape[0]
    blob = dev(np.ascontiguousarray(states).view(np.uint8).reshape(n, -1))
    obs, reward, done = es.env_step_generic(blob, dev(action.astype(np.float32).reshape(n, 1)))
    ns, w_obs, w_r, w_d = ccc.ENVS[name]["step"](states.T, action)
    got_state = blob.cpu().numpy().view(np.float64).reshape(n, -1)
    assert np.array_equal(bits(got_state), bits(ns.T.copy())), (name, np.argwhere(bits(got_state) != bits(ns.T.copy()))[:5])
    assert np.array_equal(bits(obs.cpu().numpy()), bits(w_obs))
    got_r = reward.cpu().numpy()
    want_r = w_r.astype(np.float32)                                     # the step-wise ABI carries (float)reward
    assert np.array_equal(bits(got_r), bits(want_r)), (name, np.argwhere(bits(got_r) != bits(want_r))[:5])
    assert np.array_equal(done.cpu().numpy().astype(bool), w_d)
    return ns.T.copy(), w_d


@pytest.mark.parametrize("name", NAMES)
def test_reset_is_the_widened_init_row(name):
    es = handle(name)
    e = ccc.ENVS[name]
    init = es.init_states_uniform(5, 2, 0, 300)[:, 0].contiguous()
    assert es.init_range == e["init_range"] and es.init_dim == e["init_dim"]
    want_init = co.init_states_uniform(5, 2, 0, 300, 1, e["init_dim"], False, *e["init_range"])[:, 0]
    assert np.array_equal(bits(init.cpu().numpy()), bits(want_init))
    state, obs = es.env_reset(init)
    assert es.env_state_bytes() == 16 and es.env_obs_width() == e["S"]
    s = e["reset"](want_init)
    assert np.array_equal(bits(state.cpu().numpy().view(np.float64)), bits(s.T.copy()))
    assert np.array_equal(bits(obs.cpu().numpy()), bits(e["obs"](s)))
    es.close()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n", [1, 4133])
def test_transitions_are_bit_exact(name, n):
    es = handle(name)
    rng = np.random.default_rng(n)
    c_states, c_acts = crafted(name)
    if n == 1:
        idx = np.arange(0, len(c_states), max(1, len(c_states) // 40))
        sets = [(c_states[i:i + 1], c_acts[i:i + 1]) for i in idx]
    else:
        sets = []
        for lo in range(0, len(c_states), n // 2):                      # the crafted cases, each batch filled up with random ones
            cs, ca = c_states[lo:lo + n // 2], c_acts[lo:lo + n // 2]
            rs, ra = random_cases(name, n - len(cs), rng)
            sets.append((np.concatenate([cs, rs]), np.concatenate([ca, ra])))
    dones = []
    for states, acts in sets:
        assert states.shape[0] == n
        dones.append(step_and_compare(es, name, states, acts)[1])
    if n > 1:
        d = np.concatenate(dones)
        if name == "Pendulum-v1":
            assert not d.any()                                          # the env never terminates
        else:
            assert d.any() and not d.all()                              # both outcomes of done occur in the batch
        # 20 steps in a row through the blob: the state carried is the float64 one (MountainCarContinuous: float32-rounded)
        states, acts = sets[0]
        for t in range(20):
            a = np.roll(acts, t)
            states, _ = step_and_compare(es, name, states, a)
    es.close()


# ---- fused rollouts ------------------------------------------------------------------------------------------------------------
def hand_built(name, gru, rng, noise):
    """a = tanh(logit), logit = 3 * tanh(gain * obs[f]) (through the GRU's n gate with z shut)."""
    e = ccc.ENVS[name]
    S = e["S"]
    f, gain = CASE[name]["feat"]
    th = np.zeros(co.param_count(S, 1, gru), np.float32)
    th[f] = gain                                                        # fc1 unit 0 <- obs[f]
    off = 32 * S + 32
    if gru:
        wih, whh = off, off + 96 * 32
        bih, bhh = whh + 96 * 32, whh + 96 * 32 + 96
        th[bih + 32] = -30.0                                            # z of unit 0 shut: h' = n
        th[wih + 64 * 32] = 5.0                                         # n of unit 0 <- a_0
        off = bhh + 96
    th[off] = 3.0                                                       # the one output <- unit 0
    return th + (rng.standard_normal(th.shape) * noise).astype(np.float32)


def population(name, gru, n, rng):
    P = co.param_count(ccc.ENVS[name]["S"], 1, gru)
    rows = []
    for i in range(n):
        if i % 4 == 3:                                                  # a random policy in every fourth row
            rows.append((rng.standard_normal(P) * rng.choice([0.1, 0.5, 1.5])).astype(np.float32))
        else:
            rows.append(hand_built(name, gru, rng, 0.0 if i == 0 else 0.02))
    return np.stack(rows)


def oracle_rollout(name, gru, theta, init, E, T, trace=None):
    """trace: a list that receives every step's action array (one float32 per env still running)"""
    S = ccc.ENVS[name]["S"]

    def policy(th, obs, h):
        _, _, act, hn = co.policy_forward(S, 1, False, gru, th, obs, h)
        if trace is not None:
            trace.append(act[:, 0].copy())
        return act, hn

    return ccc.rollout(name, theta, init, E, T, policy)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("gru", [False, True], ids=["mlp", "gru"])
@pytest.mark.parametrize("E", [1, 5, 8])
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "own"])
@pytest.mark.parametrize("n", [1, 63, 1000])
def test_fused_rollout_is_bit_exact(name, gru, E, shared, n):
    """Every accepted lanes_per_env (MLP; 0 = the library's choice) against one host loop of the checker env + the oracle's
    policy forward: per-episode return (float64 bits), length and fitness bit for bit."""
    T = CASE[name]["T"]
    rng = np.random.default_rng(n * 100 + E * 10 + int(gru) * 2 + int(shared))
    theta = population(name, gru, n, rng)
    es = handle(name, gru, E, T)
    init = es.init_states_uniform(11, 3, 40, 1 if shared else n, shared=shared)
    init_dev = init[0].contiguous() if shared else init
    trace = []
    w_fit, w_ret, w_steps = oracle_rollout(name, gru, theta, init.cpu().numpy(), E, T, trace)
    if name == "Pendulum-v1":
        assert (w_steps == T).all()                                     # every episode has exactly max_step steps
        assert (w_ret < 0).all()
        # The random rows' returns differ from one another -- except where two policies saturate the tanh head (the table
        # returns exactly +-1 there: scale-1.5 rows do) into the SAME action sequence from the same shared reset: those
        # episodes are the same trajectory and tie legitimately, like the saturated hand-built rows.  So: equal returns only
        # with bit-equal action sequences.
        acts = np.stack(trace).reshape(T, n, E)[:, 3::4, :].reshape(T, -1)
        rnd = w_ret[3::4].reshape(-1)
        if rnd.size:
            order = np.argsort(rnd, kind="stable")
            for i, j in zip(order[:-1], order[1:]):
                if rnd[i] == rnd[j]:
                    assert shared and np.array_equal(bits(acts[:, i]), bits(acts[:, j])), (i, j, rnd[i])
            assert len(np.unique(rnd)) >= 0.9 * rnd.size                # and such ties are rare
    else:
        early = (w_steps < T).mean()                                    # the env's own termination, not only the cap ...
        assert early >= 0.25, early
        if n >= 4:                                                      # ... and the cap too, wherever the population has random rows
            assert 1.0 - early >= 0.10, early                           # (n = 1 is the one hand-built policy: it always reaches the goal)
    es.close()
    for lanes in (LANES if not gru else (0,)):
        es = handle(name, gru, E, T, lanes)
        fit, ep_ret, ep_steps = es.rollout(dev(theta), init_dev, want_episodes=True)
        assert np.array_equal(ep_steps.cpu().numpy(), w_steps), lanes
        assert np.array_equal(bits(ep_ret.cpu().numpy()), bits(w_ret)), lanes
        assert np.array_equal(bits(fit.cpu().numpy()), bits(w_fit)), lanes
        es.close()


def test_pendulum_generic_kernel_agrees():
    """The generic observe / step kernel (ses_set_tuning pendulum_generic_step = 1, the A/B partner of the one-sincos kernel)
    returns the same bits."""
    name, E, T = "Pendulum-v1", 5, 150
    theta = population(name, False, 200, np.random.default_rng(7))
    out = {}
    for generic in (0, 1):
        for lanes in (1, 4, 16):
            es = handle(name, False, E, T, lanes)
            es.set_tuning("pendulum_generic_step", generic)
            init = es.init_states_uniform(2, 1, 0, 200)
            fit, ep_ret, ep_steps = es.rollout(dev(theta), init, want_episodes=True)
            out[generic, lanes] = (bits(fit.cpu().numpy()), bits(ep_ret.cpu().numpy()), ep_steps.cpu().numpy())
            es.close()
    for key, val in out.items():
        for a, b in zip(val, out[0, 1]):
            assert np.array_equal(a, b), key


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
@pytest.mark.parametrize("name", ["pendulum", "mountaincar_continuous"])
def test_the_reference_playback_loop_runs_on_the_wrappers(name):
    """The reference's test.py loop over the wrapper (one transition per launch) against the fused rollout kernel fed the
    same reset rows: equal episode lengths; returns within 2^-23 * sum |r_t|.  Derived, not measured: playback adds the
    float32-rounded rewards of the step-wise ABI, each within 2^-24 |r_t| of the float64 reward the kernel adds, and the
    float64 summation error is orders below that.  sum |r_t| is bounded from the env: Pendulum's rewards are all <= 0, so it
    is |return|; MountainCarContinuous' is at most 100 + 0.1 * steps (|a| <= 1 from the tanh head)."""
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
        want = float(ep_ret[0, 0])
        sum_abs = abs(want) if env.name == "Pendulum-v1" else 100.0 + 0.1 * steps
        print(name, k, "steps", steps, "playback", ret, "fused", want, "bound", 2.0 ** -23 * sum_abs)
        assert int(ep_steps[0, 0]) == steps, (k, got, ep_steps)
        assert abs(float(ret) - want) <= 2.0 ** -23 * sum_abs, (k, ret, want)
    if env.name == "Pendulum-v1":
        assert all(steps == env.horizon for _, steps in got)
    else:
        assert any(steps < env.horizon for _, steps in got)
    es.close()
    env.close()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("strategy", ["openai_es", "simple_evolution"])
def test_training_loop_paths_agree(tmp_path, monkeypatch, name, strategy):
    """Three generations per-generation (SES_BATCH_GENERATIONS=0) and through ses_run_generations: identical populations."""
    import builder
    monkeypatch.chdir(tmp_path)
    e = ccc.ENVS[name]
    cfg = {"env": {"name": name, "max_step": CASE[name]["T"], "pomdp": False, "seed": 3},
           "network": {"name": "gym_model", "num_state": e["S"], "num_action": 1, "discrete_action": False, "gru": False},
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
