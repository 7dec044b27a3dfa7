"""The inverted-pendulum family modelled on pybullet_envs on the HIP path (csrc/ses_f64_envs.hip), held bit for bit to the
independent numpy float64 restatement in tests/pendula_np.py: resets, single transitions (ses_env_step_generic) on crafted and
random states and actions, fused MLP / GRU rollouts against a host loop of that env plus the oracle's policy forward (its tanh
`act`), the two forms of the MLP rollout against each other, the refusals, the reference's playback loop on the wrappers, the
training loop on both of its paths, and learning on conf/inverted_pendulum.yaml."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch
import yaml

import pendula_np as pn
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BALANCE, SWINGUP, DOUBLE = "InvertedPendulumBulletEnv-v0", "InvertedPendulumSwingupBulletEnv-v0", "InvertedDoublePendulumBulletEnv-v0"
NAMES = (BALANCE, SWINGUP, DOUBLE)
CONF = {BALANCE: "inverted_pendulum", SWINGUP: "pendulum_swingup", DOUBLE: "double_pendulum"}
STATE_BYTES = {BALANCE: 32, SWINGUP: 32, DOUBLE: 48}
T = 150                                                                 # max_step of the rollout tests
LANES = (0, 1, 2, 4, 8, 16, 32)
# The hand-built policies a = tanh(4 tanh(g . obs / 4)) (linear for small g . obs, saturating at +-1), the gains chosen on the CPU
# with the restatement alone.  "hold": the linear-quadratic regulator of the upright equilibrium (Q = diag(1, 0.1, 10, 0.1[, 10,
# 0.1]), R = 10 on the restatement's own linearisation), written on the observation with sin theta for theta -- it keeps the
# single and the double pendulum up from every reset for the 150 steps.  "pump": push along the angular velocity -- it feeds
# energy into the pole, fells a balanced one within ~30 steps and drives the swing-up cart into the rail.
HOLD = {BALANCE: {0: 0.28, 1: 0.41, 3: 4.35, 4: 0.75}, SWINGUP: {0: 0.28, 1: 0.41, 3: 4.35, 4: 0.75},
        DOUBLE: {0: -0.24, 1: -0.40, 4: -2.18, 5: -1.35, 7: -10.42, 8: -1.39}}
PUMP = {BALANCE: {4: 3.0}, SWINGUP: {4: 3.0}, DOUBLE: {5: 3.0}}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def handle(name, gru=False, E=1, max_step=T, lanes=0):
    from ses import HipES
    return HipES(name, pn.ENVS[name]["S"], 1, False, gru, max_step=max_step, eval_ep_num=E, lanes_per_env=lanes)


# ---- single transitions ------------------------------------------------------------------------------------------------------
def flip_pair(name, make, lo, hi):
    """The adjacent doubles (p, q) between lo and hi at which the restatement's `done` after one step from make(.) with a = 0
    flips: bisection on the outcome, so that the crafted states sit AT and BESIDE the threshold of the state they enter."""
    step = pn.ENVS[name]["step"]

    def done(p):
        return bool(step(np.array(make(p), np.float64).reshape(-1, 1), np.zeros(1, np.float32))[3][0])

    d_lo = done(lo)
    assert d_lo != done(hi)
    while True:
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            return lo, hi
        lo, hi = (mid, hi) if done(mid) == d_lo else (lo, mid)


def around(p, q):
    return [p, q, np.nextafter(p, -np.inf), np.nextafter(q, np.inf)]


def crafted(name):
    """(states float64[m, state_dim], actions float32[m]): every crafted state with every crafted action"""
    hp = 0.5 * np.pi
    one = np.float32(1.0)
    acts = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(one, np.float32(2.0)), np.nextafter(-one, np.float32(-2.0)), 4.0, -4.0, 0.3],
                    np.float32)
    rails = [(sx * x, v) for sx in (1.0, -1.0) for x in (1.0, np.nextafter(1.0, 0.0), 0.999, 1.2)
             for v in (0.5, -0.5, 0.0, -0.0, 3.0, -3.0, 1e-3)]
    quad = []
    for k in range(-50, 51):                                            # theta near the multiples of pi / 2 up to |theta| ~ 80
        t = k * hp
        quad += [t, np.nextafter(t, 100.0), np.nextafter(t, -100.0), t + 1e-9, t - 1e-9, t + 0.25 * np.pi, np.nextafter(t + 0.25 * np.pi, 100.0)]
    quad += [80.0, -80.0, 79.3, -79.3, 40.0, -65.0]
    if name != DOUBLE:
        states = [(x, v, 0.05, 0.1) for x, v in rails]
        if name == SWINGUP:
            states += [(x, v, 3.0, -1.0) for x, v in rails]
        for sgn in (1.0, -1.0):                                         # theta at and beside +-0.2, before and after the step
            states += [(0.0, 0.0, th, 0.0) for th in around(*flip_pair(BALANCE, lambda p: (0.0, 0.0, sgn * p, 0.0), 0.1, 0.3))]
            states += [(0.1, -0.2, th, w) for th in around(sgn * 0.2, sgn * np.nextafter(0.2, 1.0)) for w in (0.0, 0.5, -0.5)]
        states += [(0.2, 0.1, th, w) for th in quad for w in (0.0, 2.5, -7.0)]
    else:
        states = [(x, v, 0.05, 0.1, -0.03, 0.2) for x, v in rails]
        for sgn in (1.0, -1.0):                                         # y2 + 0.3 at and beside 1 after the step, by theta1 and by theta2
            states += [(0.0, 0.0, th, 0.0, 0.0, 0.0) for th in around(*flip_pair(name, lambda p: (0.0, 0.0, sgn * p, 0.0, 0.0, 0.0), 0.3, 0.9))]
            states += [(0.0, 0.0, 0.1, 0.0, th, 0.0) for th in around(*flip_pair(name, lambda p: (0.0, 0.0, 0.1, 0.0, sgn * p, 0.0), 0.2, 2.0))]
            states += [(0.3, 0.5, sgn * th, w, 0.1, -w) for th in (0.67, 0.68, 0.69, 0.7) for w in (0.0, 1.0, -1.0)]
        states += [(0.2, 0.1, th, 1.0, th2, -2.0) for th in quad[::3] for th2 in (0.0, hp, -np.pi, 0.3, 33.0)]
        states += [(0.2, 0.1, 0.4, 1.0, th2, w) for th2 in quad for w in (0.0, 6.0)]
    states = np.array(states, np.float64)
    return np.repeat(states, len(acts), axis=0), np.tile(acts, len(states))


def random_cases(name, n, rng):
    sd = pn.ENVS[name]["state_dim"]
    cols = [rng.uniform(-1.05, 1.05, n), rng.uniform(-4.0, 4.0, n)]
    for k in range((sd - 2) // 2):
        th = rng.uniform(-80.0, 80.0, n)
        near = rng.random(n) < 0.5                                      # half of them near upright: both outcomes of done
        th[near] = rng.uniform(-0.3, 0.3, n)[near] if sd == 4 else rng.uniform(-0.9, 0.9, n)[near]
        cols += [th, rng.uniform(-10.0, 10.0, n)]
    return np.stack(cols, axis=1), rng.uniform(-1.4, 1.4, n).astype(np.float32)


def step_and_compare(es, name, states, action):
    n = states.shape[0]
    blob = dev(np.ascontiguousarray(states).view(np.uint8).reshape(n, -1))
    obs, reward, done = es.env_step_generic(blob, dev(action.astype(np.float32).reshape(n, 1)))
    ns, w_obs, w_r, w_d = pn.ENVS[name]["step"](states.T, action)
    got_state = blob.cpu().numpy().view(np.float64).reshape(n, -1)
    assert np.array_equal(bits(got_state), bits(ns.T.copy())), (name, np.argwhere(bits(got_state) != bits(ns.T.copy()))[:5])
    assert np.array_equal(bits(obs.cpu().numpy()), bits(w_obs)), (name, np.argwhere(bits(obs.cpu().numpy()) != bits(w_obs))[:5])
    got_r = reward.cpu().numpy()
    want_r = w_r.astype(np.float32)                                     # the step-wise ABI carries (float)reward
    assert np.array_equal(bits(got_r), bits(want_r)), (name, np.argwhere(bits(got_r) != bits(want_r))[:5])
    assert np.array_equal(done.cpu().numpy().astype(bool), w_d)
    return ns.T.copy(), w_d


@pytest.mark.parametrize("name", NAMES)
def test_reset_is_the_widened_init_row(name):
    es = handle(name)
    e = pn.ENVS[name]
    init = es.init_states_uniform(5, 2, 0, 300)[:, 0].contiguous()
    assert es.init_range == e["init_range"] and es.init_dim == e["init_dim"]
    want_init = co.init_states_uniform(5, 2, 0, 300, 1, e["init_dim"], False, *e["init_range"])[:, 0]
    assert np.array_equal(bits(init.cpu().numpy()), bits(want_init))
    state, obs = es.env_reset(init)
    assert es.env_state_bytes() == STATE_BYTES[name] and es.env_obs_width() == e["S"]
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
        if name == SWINGUP:
            assert not d.any()                                          # the env never terminates
        else:
            assert d.any() and not d.all()                              # both outcomes of done occur in the batch
        states, acts = sets[0]                                          # 20 steps in a row through the blob
        for t in range(20):
            states, _ = step_and_compare(es, name, states, np.roll(acts, t))
    es.close()


# ---- fused rollouts ------------------------------------------------------------------------------------------------------------
def hand_built(name, gru, gains, rng, noise):
    """a = tanh(logit), logit = 4 u, u = tanh(g . obs / 4) in fc1 unit 0 (through the GRU's n gate with z shut: logit = 4 tanh(u))."""
    S = pn.ENVS[name]["S"]
    th = np.zeros(co.param_count(S, 1, gru), np.float32)
    for f, g in gains.items():
        th[f] = g / 4.0                                                 # fc1 unit 0 <- obs[f]
    off = 32 * S + 32
    if gru:
        wih, whh = off, off + 96 * 32
        bih, bhh = whh + 96 * 32, whh + 96 * 32 + 96
        th[bih + 32] = -30.0                                            # z of unit 0 shut: h' = n
        th[wih + 64 * 32] = 1.0                                         # n of unit 0 <- a_0
        off = bhh + 96
    th[off] = 4.0                                                       # the one output <- unit 0
    return th + (rng.standard_normal(th.shape) * noise).astype(np.float32)


def population(name, gru, n, rng):
    """hold, pump, hold, random, ... : a random policy in every fourth row, the pole pumped in every fourth, held up in the rest"""
    P = co.param_count(pn.ENVS[name]["S"], 1, gru)
    rows = []
    for i in range(n):
        if i % 4 == 3:
            rows.append((rng.standard_normal(P) * rng.choice([0.1, 0.5, 1.5])).astype(np.float32))
        else:
            rows.append(hand_built(name, gru, PUMP[name] if i % 4 == 1 else HOLD[name], rng, 0.0 if i < 2 else 0.01))
    return np.stack(rows)


def oracle_rollout(name, gru, theta, init, E, max_step, on_step=None):
    S = pn.ENVS[name]["S"]

    def policy(th, obs, h):
        _, _, act, hn = co.policy_forward(S, 1, False, gru, th, obs, h)
        return act, hn

    return pn.rollout(name, theta, init, E, max_step, policy, on_step)


def check_population(name, n, w_steps, touched):
    """The conditions on the restatement's own output that make the comparison worth something."""
    if name == SWINGUP:
        assert (w_steps == T).all()                                     # every episode has exactly max_step steps
        if n >= 2:
            assert touched[0] > 0                                       # and some cart ran into a rail (n = 1 is the one hold policy)
    elif n >= 4:
        early = (w_steps < T).mean()                                    # the env's own termination, not only the cap ...
        assert early >= 0.25, early
        assert 1.0 - early >= 0.10, early                               # ... and the cap too


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("gru", [False, True], ids=["mlp", "gru"])
@pytest.mark.parametrize("E", [1, 5, 8])
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "own"])
@pytest.mark.parametrize("n", [1, 63, 1000])
def test_fused_rollout_is_bit_exact(name, gru, E, shared, n):
    """Every accepted lanes_per_env (MLP; 0 = the library's choice) against one host loop of the checker env + the oracle's
    policy forward: per-episode return (float64 bits), length and fitness bit for bit."""
    rng = np.random.default_rng(n * 100 + E * 10 + int(gru) * 2 + int(shared))
    theta = population(name, gru, n, rng)
    es = handle(name, gru, E)
    init = es.init_states_uniform(11, 3, 40, 1 if shared else n, shared=shared)
    init_dev = init[0].contiguous() if shared else init
    es.close()
    touched = [0]

    def on_step(live, ns):
        touched[0] += int((np.abs(ns[0]) == 1.0).sum())

    w_fit, w_ret, w_steps = oracle_rollout(name, gru, theta, init.cpu().numpy(), E, T, on_step)
    check_population(name, n, w_steps, touched)
    for lanes in (LANES if not gru else (0,)):
        es = handle(name, gru, E, T, lanes)
        fit, ep_ret, ep_steps = es.rollout(dev(theta), init_dev, want_episodes=True)
        assert np.array_equal(ep_steps.cpu().numpy(), w_steps), lanes
        assert np.array_equal(bits(ep_ret.cpu().numpy()), bits(w_ret)), lanes
        assert np.array_equal(bits(fit.cpu().numpy()), bits(w_fit)), lanes
        es.close()


@pytest.mark.parametrize("name", NAMES)
def test_generic_step_form_agrees(name):
    """The generic observe / step form (ses_set_tuning pendula_generic_step = 1, the A/B partner of the one-trig form) returns
    the same bits."""
    E = 5
    theta = population(name, False, 200, np.random.default_rng(7))
    out = {}
    for generic in (0, 1):
        for lanes in (1, 4, 16):
            es = handle(name, False, E, T, lanes)
            es.set_tuning("pendula_generic_step", generic)
            init = es.init_states_uniform(2, 1, 0, 200)
            fit, ep_ret, ep_steps = es.rollout(dev(theta), init, want_episodes=True)
            out[generic, lanes] = (bits(fit.cpu().numpy()), bits(ep_ret.cpu().numpy()), ep_steps.cpu().numpy())
            es.close()
    for key, val in out.items():
        for a, b in zip(val, out[0, 1]):
            assert np.array_equal(a, b), key
    steps = out[0, 1][2]
    assert (steps == T).all() if name == SWINGUP else ((steps < T).any() and (steps == T).any())


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("name", NAMES)
def test_ses_create_refuses_each_wrong_field(name):
    from ses import HipES, SesError
    S = pn.ENVS[name]["S"]
    HipES(name, S, 1, False, False, max_step=10, eval_ep_num=1).close()
    HipES(name, S, 1, False, True, max_step=10, eval_ep_num=1).close()
    for bad in (dict(num_state=S + 1), dict(num_state=14 - S), dict(num_action=2), dict(discrete_action=True), dict(pomdp=True),
                dict(physics64=True)):
        kw = dict(num_state=S, num_action=1, discrete_action=False, gru=False, max_step=10, eval_ep_num=1)
        kw.update(bad)
        with pytest.raises(SesError):
            HipES(name, **kw)


# ---- playback and training --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_reference_playback_loop_runs_on_the_wrappers(name):
    """The reference's test.py loop over the wrapper (one transition per launch) against the fused rollout kernel fed the
    same reset rows: equal episode lengths; returns within 2^-23 * sum |r_t|.  Derived, not measured: playback adds the
    float32-rounded rewards of the step-wise ABI, each within 2^-24 |r_t| of the float64 reward the kernel adds, and the
    float64 summation error is orders below that.  sum |r_t| is bounded from the env: |r_t| <= 1 for balance (1) and swing-up
    (a cosine), so it is at most the number of steps; the double pendulum's reward lies in (10 - 0.01 * 1.9^2 - 2^2, 10], so
    it is at most 10 per step."""
    import builder
    from test_gpu_envs import playback
    cfg = yaml.load(open(os.path.join(ROOT, "simple-es_amd", "conf", CONF[name] + ".yaml")), Loader=yaml.FullLoader)
    cfg["env"]["max_step"] = 300
    env = builder.build_env(cfg["env"])
    net = builder.build_network(cfg["network"])
    episodes = 3
    # episodes 0 and 2: the hold policy; episode 1: the regulator with its sign turned, which throws the pole over within 20 steps
    nets = [hand_built(name, False, HOLD[name] if k != 1 else {f: -g for f, g in HOLD[name].items()}, np.random.default_rng(k), 0.01)
            for k in range(episodes)]
    es = handle(name, False, 1, env.horizon)
    lengths = []
    for k in range(episodes):
        net.load_flat(nets[k])
        (ret, steps), = playback(env, net, 1)
        init = es.init_states_uniform(0, k, 0, 1)
        _, ep_ret, ep_steps = es.rollout(dev(net.flat()[None, :]), init, want_episodes=True)
        want = float(ep_ret[0, 0])
        sum_abs = (10.0 if name == DOUBLE else 1.0) * steps
        print(name, k, "steps", steps, "playback", ret, "fused", want, "bound", 2.0 ** -23 * sum_abs)
        assert int(ep_steps[0, 0]) == steps, (k, steps, ep_steps)
        assert abs(float(ret) - want) <= 2.0 ** -23 * sum_abs, (k, ret, want)
        lengths.append(steps)
    if name == SWINGUP:
        assert all(s == env.horizon for s in lengths)
    else:
        assert lengths[0] == env.horizon and lengths[1] < 30            # held up to the cap; thrown over
    es.close()
    env.close()


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("strategy", ["openai_es", "sep_cma_es"])
def test_training_loop_paths_agree(tmp_path, monkeypatch, name, strategy):
    """Three generations per-generation (SES_BATCH_GENERATIONS=0) and through ses_run_generations: identical populations."""
    import builder
    monkeypatch.chdir(tmp_path)
    e = pn.ENVS[name]
    cfg = {"env": {"name": name, "max_step": T, "pomdp": False, "seed": 3},
           "network": {"name": "gym_model", "num_state": e["S"], "num_action": 1, "discrete_action": False, "gru": False},
           "strategy": {"name": strategy, "init_sigma": 0.5, "sigma_decay": 0.99, "learning_rate": 0.05, "offspring_num": 48, "seed": 1}}
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


LEARNING_GENERATIONS = 26   # twice the 13 the recorded run needed (profiles/pendula_learning.txt: best 1000 in generation 12, seed 0)


def test_inverted_pendulum_config_learns_to_balance(tmp_path, monkeypatch):
    """conf/inverted_pendulum.yaml reaches a best return of 1000 -- the TimeLimit, i.e. the env's maximum: every one of the
    five episodes of some offspring balanced to the cap -- within twice the generations the recorded run needed."""
    import builder
    monkeypatch.chdir(tmp_path)
    cfg = yaml.load(open(os.path.join(ROOT, "simple-es_amd", "conf", "inverted_pendulum.yaml")), Loader=yaml.FullLoader)
    cfg["strategy"]["seed"] = 0
    cfg["env"]["seed"] = 0
    loop = builder.build_loop(cfg, LEARNING_GENERATIONS, 1, 5, False, 10 ** 9)
    with contextlib.redirect_stdout(io.StringIO()):
        loop.run()
    best = [b for b, _ in loop.history]
    print("best per generation", best)
    assert max(best) == 1000.0, best
