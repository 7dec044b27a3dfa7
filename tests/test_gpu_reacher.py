"""ReacherBulletEnv-v0 on the HIP path (csrc/ses_f64_envs.hip), held bit for bit to the independent numpy float64 restatement in
tests/reacher_np.py: the reset, single transitions (ses_env_step_generic) on crafted and random states and actions, fused MLP /
GRU rollouts against a host loop of that env plus the oracle's policy forward (its tanh `act`, both outputs), the two forms of
the MLP rollout against each other, the refusals, the reference's playback loop on the wrapper, the training loop on both of
its paths, and learning on conf/reacher.yaml."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch
import yaml

import reacher_np as rn
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ReacherBulletEnv-v0"
T = 150                                                                 # max_step of the rollout tests: the env's horizon
LANES = (0, 1, 2, 4, 8, 16, 32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def handle(gru=False, E=1, max_step=T, lanes=0):
    from ses import HipES
    return HipES(NAME, rn.S, rn.A, False, gru, max_step=max_step, eval_ep_num=E, lanes_per_env=lanes)


# ---- single transitions ------------------------------------------------------------------------------------------------------
def with_pot(states):
    """float64[m, 6] (th, w1, g, w2, tx, ty) -> float64[m, 7]: the potential of the state appended, as a reset or a step leaves it"""
    s = np.concatenate([np.asarray(states, np.float64), np.zeros((len(states), 1))], axis=1).T.copy()
    s[6] = rn.potential(s, rn.trig(s))
    return s.T.copy()


def beside(x):
    return [x, np.nextafter(x, np.inf), np.nextafter(x, -np.inf)]


def crafted():
    """(states float64[m, 7], actions float32[m, 2])"""
    hp = 0.5 * np.pi
    one = np.float32(1.0)
    vals = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(one, np.float32(2.0)), np.nextafter(-one, np.float32(-2.0)), 4.0, -4.0, 0.3], np.float32)
    acts = np.array([(a, b) for a in vals for b in vals], np.float32)     # both slots independently: 81 pairs
    few = acts[[0, 10, 20, 38, 51, 66, 80]]
    states = []
    # g at and beside +-3 with rates of both signs (and outside, as a caller's blob may be)
    for sgn in (1.0, -1.0):
        for g in beside(sgn * 3.0) + [sgn * 2.999, sgn * 3.2]:
            states += [(0.4, 0.7, g, w2, 0.1, -0.05) for w2 in (0.5, -0.5, 0.0, -0.0, 6.0, -6.0, 1e-3)]
    # |g| at and beside 0.99, 1, 1.01 (the stuck-joint band of the state ENTERED: rate 0 keeps g, a small rate crosses the edge)
    for sgn in (1.0, -1.0):
        for edge in (0.99, 1.0, 1.01):
            for g in beside(sgn * edge):
                states += [(-1.0, 0.0, g, 0.0, 0.05, 0.2), (-1.0, 0.3, g, 1e-7, 0.05, 0.2), (-1.0, 0.3, g, -1e-7, 0.05, 0.2)]
    base = len(states)
    # th and g at and beside the multiples of pi / 2, up to |80| (g beyond the limit is clipped by the step; its trig is still read)
    for k in range(-50, 51):
        t = k * hp
        for x in beside(t) + [t + 1e-9, t + 0.25 * np.pi]:
            states.append((x, 1.0, 0.3, -2.0, 0.1, 0.1))
            states.append((0.4, 1.0, x, 0.5, 0.1, 0.1))
    states += [(80.0, 0.0, -80.0, 0.0, 0.0, 0.0), (-79.3, 2.0, 79.3, -1.0, 0.2, -0.2), (40.0, 0.0, -65.0, 0.0, 0.0, 0.0)]
    states = with_pot(states)
    # the fingertip exactly on the target: distance 0 in the state left (pot = -0) ...
    on = []
    for th, g in ((0.0, 0.0), (0.3, 1.2), (-2.0, -0.5), (1.0, 3.0)):
        s = with_pot([(th, 0.0, g, 0.0, 0.0, 0.0)]).T.copy()
        dx, dy = rn.to_target(s, rn.trig(s))
        on.append((th, 0.0, g, 0.0, dx[0], dy[0]))                        # target := fingertip
        on.append((th, 0.5, g, -0.5, dx[0], dy[0]))
    on = with_pot(on)
    dx, dy = rn.to_target(on.T.copy(), rn.trig(on.T.copy()))
    assert (dx[::2] == 0.0).all() and (dy[::2] == 0.0).all() and (on[::2, 6] == 0.0).all()   # ... and, at rest and idle, in the one entered
    out_s = [np.repeat(states[:base], len(acts), axis=0), np.repeat(states[base:], len(few), axis=0), np.repeat(on, len(acts), axis=0)]
    out_a = [np.tile(acts, (base, 1)), np.tile(few, (len(states) - base, 1)), np.tile(acts, (len(on), 1))]
    return np.concatenate(out_s), np.concatenate(out_a)


def random_cases(n, rng):
    g = rng.uniform(-3.0, 3.0, n)
    near = rng.random(n) < 0.3
    g[near] = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.98, 1.02, n))[near]
    edge = rng.random(n) < 0.2
    g[edge] = (rng.choice([-1.0, 1.0], n) * rng.uniform(2.9, 3.0, n))[edge]
    cols = [rng.uniform(-80.0, 80.0, n), rng.uniform(-10.0, 10.0, n), g, rng.uniform(-10.0, 10.0, n), rng.uniform(-0.27, 0.27, n),
            rng.uniform(-0.27, 0.27, n)]
    return with_pot(np.stack(cols, axis=1)), rng.uniform(-1.4, 1.4, (n, 2)).astype(np.float32)


def step_and_compare(es, states, action):
    n = states.shape[0]
    blob = dev(np.ascontiguousarray(states).view(np.uint8).reshape(n, -1))
    obs, reward, done = es.env_step_generic(blob, dev(action.astype(np.float32).reshape(n, 2)))
    ns, w_obs, w_r, w_d = rn.step(states.T, action)
    got_state = blob.cpu().numpy().view(np.float64).reshape(n, -1)
    assert np.array_equal(bits(got_state), bits(ns.T.copy())), np.argwhere(bits(got_state) != bits(ns.T.copy()))[:5]
    assert np.array_equal(bits(obs.cpu().numpy()), bits(w_obs)), np.argwhere(bits(obs.cpu().numpy()) != bits(w_obs))[:5]
    got_r = reward.cpu().numpy()
    want_r = w_r.astype(np.float32)                                     # the step-wise ABI carries (float)reward
    assert np.array_equal(bits(got_r), bits(want_r)), np.argwhere(bits(got_r) != bits(want_r))[:5]
    assert not done.cpu().numpy().any() and not w_d.any()               # the env never terminates
    return ns.T.copy()


def test_reset_is_the_widened_init_row():
    es = handle()
    init = es.init_states_uniform(5, 2, 0, 300)[:, 0].contiguous()
    assert es.init_range == rn.INIT_RANGE and es.init_dim == rn.INIT_DIM
    want_init = co.init_states_uniform(5, 2, 0, 300, 1, rn.INIT_DIM, False, *rn.INIT_RANGE)[:, 0]
    assert np.array_equal(bits(init.cpu().numpy()), bits(want_init))
    state, obs = es.env_reset(init)
    assert es.env_state_bytes() == 56 and es.env_obs_width() == 9
    s = rn.reset(want_init)
    assert np.array_equal(bits(state.cpu().numpy().view(np.float64)), bits(s.T.copy()))
    assert np.array_equal(bits(obs.cpu().numpy()), bits(rn.obs_of(s)))
    es.close()


@pytest.mark.parametrize("n", [1, 4133])
def test_transitions_are_bit_exact(n):
    es = handle()
    rng = np.random.default_rng(n)
    c_states, c_acts = crafted()
    if n == 1:
        idx = np.arange(0, len(c_states), max(1, len(c_states) // 60))
        sets = [(c_states[i:i + 1], c_acts[i:i + 1]) for i in idx]
    else:
        sets = []
        for lo in range(0, len(c_states), n // 2):                      # the crafted cases, each batch filled up with random ones
            cs, ca = c_states[lo:lo + n // 2], c_acts[lo:lo + n // 2]
            rs, ra = random_cases(n - len(cs), rng)
            sets.append((np.concatenate([cs, rs]), np.concatenate([ca, ra])))
    seen_limit = seen_stuck = seen_free = 0
    for states, acts in sets:
        assert states.shape[0] == n
        ns = step_and_compare(es, states, acts)
        seen_limit += int((np.abs(ns[:, 2]) == 3.0).sum())
        stuck = np.abs(np.abs(ns[:, 2]) - 1.0) < 0.01
        seen_stuck += int(stuck.sum())
        seen_free += int((~stuck).sum())
    if n > 1:
        assert seen_limit > 100 and seen_stuck > 100 and seen_free > 100   # every branch of the step occurs in the batches
        states, acts = sets[0]                                          # 20 steps in a row through the blob
        for t in range(20):
            states = step_and_compare(es, states, np.roll(acts, t, axis=0))
    es.close()


# ---- fused rollouts ------------------------------------------------------------------------------------------------------------
def population(gru, n, rng):
    """row 0: the zero policy (idle); then random policies of three scales -- the large ones saturate both actions and drive the
    elbow into its limit, the small ones barely move"""
    P = co.param_count(rn.S, rn.A, gru)
    rows = [np.zeros(P, np.float32)]
    for i in range(1, n):
        rows.append((rng.standard_normal(P) * (0.1, 0.5, 1.5)[i % 3]).astype(np.float32))
    return np.stack(rows[:n])


def oracle_rollout(gru, theta, init, E, max_step, on_step=None):
    def policy(th, obs, h):
        _, _, act, hn = co.policy_forward(rn.S, rn.A, False, gru, th, obs, h)
        return act, hn

    return rn.rollout(theta, init, E, max_step, policy, on_step)


@pytest.mark.parametrize("gru", [False, True], ids=["mlp", "gru"])
@pytest.mark.parametrize("E", [1, 5, 8])
@pytest.mark.parametrize("shared", [True, False], ids=["shared", "own"])
@pytest.mark.parametrize("n", [1, 63, 1000])
def test_fused_rollout_is_bit_exact(gru, E, shared, n):
    """Every accepted lanes_per_env (MLP; 0 = the library's choice) against one host loop of the checker env + the oracle's
    policy forward: per-episode return (float64 bits), length and fitness bit for bit."""
    rng = np.random.default_rng(n * 100 + E * 10 + int(gru) * 2 + int(shared))
    theta = population(gru, n, rng)
    es = handle(gru, E)
    init = es.init_states_uniform(11, 3, 40, 1 if shared else n, shared=shared)
    init_dev = init[0].contiguous() if shared else init
    es.close()
    touched = [0, 0]

    def on_step(ns):
        touched[0] += int((np.abs(ns[2]) == 3.0).sum())
        touched[1] += int((np.abs(np.abs(ns[2]) - 1.0) < 0.01).sum())

    w_fit, w_ret, w_steps = oracle_rollout(gru, theta, init.cpu().numpy(), E, T, on_step)
    # conditions on the restatement's own output that make the comparison worth something
    assert (w_steps == T).all()
    if n >= 63:
        assert touched[0] > 0 and touched[1] > 0                        # elbows at the limit, joints in the stuck band
        assert len(np.unique(w_ret)) > w_ret.size // 2
    for lanes in (LANES if not gru else (0,)):
        es = handle(gru, E, T, lanes)
        fit, ep_ret, ep_steps = es.rollout(dev(theta), init_dev, want_episodes=True)
        assert np.array_equal(ep_steps.cpu().numpy(), w_steps), lanes
        assert np.array_equal(bits(ep_ret.cpu().numpy()), bits(w_ret)), lanes
        assert np.array_equal(bits(fit.cpu().numpy()), bits(w_fit)), lanes
        es.close()


def test_generic_step_form_agrees():
    """The generic observe / step form (ses_set_tuning reacher_generic_step = 1, the A/B partner of the one-trig form) returns
    the same bits."""
    E = 5
    theta = population(False, 200, np.random.default_rng(7))
    out = {}
    for generic in (0, 1):
        for lanes in (1, 2, 4, 16, 32):
            es = handle(False, E, T, lanes)
            es.set_tuning("reacher_generic_step", generic)
            init = es.init_states_uniform(2, 1, 0, 200)
            fit, ep_ret, ep_steps = es.rollout(dev(theta), init, want_episodes=True)
            out[generic, lanes] = (bits(fit.cpu().numpy()), bits(ep_ret.cpu().numpy()), ep_steps.cpu().numpy())
            es.close()
    for key, val in out.items():
        for a, b in zip(val, out[0, 1]):
            assert np.array_equal(a, b), key
    assert (out[0, 1][2] == T).all() and len(np.unique(out[0, 1][1])) > 500


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_fixed_length_mode_is_refused():
    from ses import SesError
    from ses._lib import MODE_FIXED_LENGTH
    for gru in (False, True):
        es = handle(gru)
        theta = dev(population(gru, 2, np.random.default_rng(0)))
        init = es.init_states_uniform(1, 0, 0, 1, shared=True)[0].contiguous()
        with pytest.raises(SesError, match="Reacher has no fixed-length mode"):
            es.rollout(theta, init, mode=MODE_FIXED_LENGTH)
        es.close()


def test_ses_create_refuses_each_wrong_field():
    from ses import HipES, SesError
    HipES(NAME, 9, 2, False, False, max_step=10, eval_ep_num=1).close()
    HipES(NAME, 9, 2, False, True, max_step=10, eval_ep_num=1).close()
    for bad, word in ((dict(num_state=10), "num_state"), (dict(num_state=5), "num_state"), (dict(num_action=1), "num_action"),
                      (dict(discrete_action=True), "discrete_action"), (dict(pomdp=True), "pomdp"), (dict(physics64=True), "physics64")):
        kw = dict(num_state=9, num_action=2, discrete_action=False, gru=False, max_step=10, eval_ep_num=1)
        kw.update(bad)
        with pytest.raises(SesError, match="ReacherBulletEnv-v0.*" + word):
            HipES(NAME, **kw)


# ---- playback and training --------------------------------------------------------------------------------------------------------
def test_the_reference_playback_loop_runs_on_the_wrapper():
    """The reference's test.py loop over the wrapper (one transition per launch) against the fused rollout kernel fed the
    same reset rows: equal episode lengths; returns within 2^-23 * sum |r_t|.  Derived, not measured: playback adds the
    float32-rounded rewards of the step-wise ABI, each within 2^-24 |r_t| of the float64 reward the kernel adds, and the
    float64 summation error is orders below that.  sum |r_t| is taken from the restatement's own rollout of the same policy
    (the reward has no bound as simple as the pendula's |r| <= 1), never from the device."""
    import builder
    from test_gpu_envs import playback
    cfg = yaml.load(open(os.path.join(ROOT, "simple-es_amd", "conf", "reacher.yaml")), Loader=yaml.FullLoader)
    env = builder.build_env(cfg["env"])
    net = builder.build_network(cfg["network"])
    assert env.horizon == T
    es = handle(False, 1, env.horizon)
    rng = np.random.default_rng(5)
    for k in range(3):
        flat = (rng.standard_normal(co.param_count(9, 2, False)) * (0.0, 0.5, 1.5)[k]).astype(np.float32)
        net.load_flat(flat)
        (ret, steps), = playback(env, net, 1)
        init = es.init_states_uniform(0, k, 0, 1)
        _, ep_ret, ep_steps = es.rollout(dev(net.flat()[None, :]), init, want_episodes=True)
        rewards = []

        def policy(th, obs, h):
            return co.policy_forward(9, 2, False, False, th, obs, h)[2], None

        s = rn.reset(init.cpu().numpy().reshape(1, 4))
        obs, total = rn.obs_of(s), 0.0
        for _ in range(T):
            s, obs, r, _ = rn.step(s, policy(flat[None, :], obs, None)[0])
            rewards.append(r[0])
            total = total + r[0]
        sum_abs = float(np.abs(rewards).sum())
        want = float(ep_ret[0, 0])
        print(k, "steps", steps, "playback", ret, "fused", want, "bound", 2.0 ** -23 * sum_abs)
        assert want == total
        assert int(ep_steps[0, 0]) == steps == T
        assert abs(float(ret) - want) <= 2.0 ** -23 * sum_abs, (k, ret, want)
        if k == 0:
            assert sum_abs in (0.0, 15.0) or abs(sum_abs - 15.0) < 1e-9     # the idle policy
    es.close()
    env.close()


@pytest.mark.parametrize("strategy", ["openai_es", "sep_cma_es"])
def test_training_loop_paths_agree(tmp_path, monkeypatch, strategy):
    """Three generations per-generation (SES_BATCH_GENERATIONS=0) and through ses_run_generations: identical populations."""
    import builder
    monkeypatch.chdir(tmp_path)
    cfg = {"env": {"name": NAME, "max_step": T, "pomdp": False, "seed": 3},
           "network": {"name": "gym_model", "num_state": 9, "num_action": 2, "discrete_action": False, "gru": False},
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


# ---- the scene ----------------------------------------------------------------------------------------------------------------------
def scene_np(state):
    """float64[7] -> (prims, count): the scene of DESIGN.md 19 restated on render_np's Scene: the shoulder in the centre of a 400 x
    400 canvas, 500 px per metre; FILL, the target disc, the two links as capsules, the fingertip disc.  The device computes it in
    float64 with the env's own sin / cos, so the integers are EQUAL, not within one unit."""
    import render_np as rp
    s = np.asarray(state, np.float64).reshape(7, 1)
    st, ct, _, _, sb, cb = (float(v[0]) for v in rn.trig(s))
    tx, ty = float(s[4, 0]), float(s[5, 0])
    ex, ey = rn.L1 * ct, rn.L1 * st
    fx, fy = ex + rn.L2 * cb, ey + rn.L2 * sb
    sc = rp.Scene(400, 400)
    X, Y = (lambda x: sc.ux(200.0 + 500.0 * x)), (lambda y: sc.uy(200.0 + 500.0 * y))
    sc.emit(rp.FILL, rp.WHITE)
    sc.emit(rp.DISC, rp.RED, X(tx), Y(ty), 96)
    sc.emit(rp.CAPSULE, rp.POLE, X(0.0), Y(0.0), X(ex), Y(ey), 56)
    sc.emit(rp.CAPSULE, rp.AXLE, X(ex), Y(ey), X(fx), Y(fy), 56)
    sc.emit(rp.DISC, rp.AGENT, X(fx), Y(fy), 80)
    return sc.result()


def test_scene_is_byte_equal_to_the_restatement():
    import render_np as rp
    es = handle()
    assert es.render_size() == (400, 400)
    rng = np.random.default_rng(3)
    states, _ = random_cases(21, rng)
    crafted_states = with_pot([(0.0, 0.0, 0.0, 0.0, 0.2, 0.1),             # straight along +x, target up and to the right
                               (0.5 * np.pi, 0.0, 0.0, 0.0, 0.0, 0.21),      # straight up, the fingertip on the target
                               (np.pi, 0.0, 3.0, 0.0, -0.27, -0.27),         # folded at the limit, target in the corner
                               (-0.5 * np.pi, 0.0, -3.0, 0.0, 0.27, 0.27),
                               (80.0, 1.0, -1.0, 1.0, 0.0, 0.0),
                               (0.3, 0.0, 1.5, 0.0, 0.5, 0.0),               # a target a caller put outside the canvas: dropped
                               (0.3, 0.0, 1.5, 0.0, 0.41, 0.0)])             # .. partly outside: kept
    states = np.concatenate([crafted_states, states])
    n = len(states)
    blob = dev(np.ascontiguousarray(states).view(np.uint8).reshape(n, 56))
    prims, counts = es.render_scene(blob)
    want = [scene_np(s) for s in states]
    w_prims, w_counts = np.stack([w[0] for w in want]), np.array([w[1] for w in want], np.int32)
    assert np.array_equal(counts.cpu().numpy(), w_counts) and w_counts[5] == 4 and (np.delete(w_counts, 5) == 5).all()
    got = prims.cpu().numpy()
    for i in range(n):
        assert np.array_equal(got[i, :w_counts[i]], w_prims[i, :w_counts[i]]), (i, got[i, :5], w_prims[i, :5])
    frames = es.render(blob).cpu().numpy()
    assert frames.shape == (n, 400, 400) and frames.dtype == np.uint8
    assert np.array_equal(frames, rp.rasterise(w_prims, w_counts, 400, 400))
    # semantics, independent of both: y is up, x to the right, 500 px per metre round (200, 200)
    assert frames[0][200, 200 + 25] == rp.POLE and frames[0][200, 200 + 80] == rp.AXLE and frames[0][200, 200 + 105] == rp.AGENT
    assert frames[0][200 - 50, 200 + 100] == rp.RED and frames[0][5, 5] == rp.WHITE
    assert frames[1][200 - 105, 200] == rp.AGENT and (frames[1] == rp.RED).sum() > 0     # the fingertip disc (5 px) inside the target's (6 px)
    assert frames[2][399 - 64, 64] == rp.RED
    es.close()


def test_wrapper_render_is_the_device_frame_in_rgb():
    from envs.gym_wrapper import GymWrapper
    from ses.render import palette
    env = GymWrapper(NAME)
    with pytest.raises(RuntimeError) as e:
        env.render()
    assert not isinstance(e.value, NotImplementedError)
    env.reset()
    env.step({"0": np.array([0.5, -0.5], np.float32)})
    rgb = env.render()
    assert rgb.shape == (400, 400, 3) and rgb.dtype == np.uint8
    blob = env.state_blob()
    assert np.array_equal(rgb, palette()[env._device().render(blob)[0].cpu().numpy()])
    want = scene_np(blob.cpu().numpy().view(np.float64).reshape(7))
    import render_np as rp
    assert np.array_equal(rgb, palette()[rp.rasterise(want[0][None], [want[1]], 400, 400)[0]])
    assert len(np.unique(rgb.reshape(-1, 3), axis=0)) == 5
    env.close()


# ---- learning -------------------------------------------------------------------------------------------------------------------------
# profiles/reacher_learning.txt (conf/reacher.yaml, 300 generations, seed 0): the population mean starts at -17.4, ends at +2.407 (the
# mean of the last ten generations; idle = 0) and first passes half of that, 1.2035, in generation 148 -- 149 generations.
RECORDED_FINAL_MEAN = 2.407
LEARNING_GENERATIONS = 2 * 149


def test_reacher_config_learns(tmp_path, monkeypatch):
    """conf/reacher.yaml brings the population mean above half of the recorded run's final value within twice the generations the
    recorded run needed (the run is deterministic: same seed, bit-exact kernels)."""
    import builder
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("SES_BATCH_GENERATIONS", "0")                    # generation by generation: every fitness vector can be read
    cfg = yaml.load(open(os.path.join(ROOT, "simple-es_amd", "conf", "reacher.yaml")), Loader=yaml.FullLoader)
    cfg["strategy"]["seed"] = 0
    cfg["env"]["seed"] = 0
    loop = builder.build_loop(cfg, LEARNING_GENERATIONS, 1, 5, False, 10 ** 9)
    means = []
    rollout = loop.rollout

    def recording(population):
        fitness = rollout(population)
        means.append(fitness.mean())
        return fitness

    loop.rollout = recording
    with contextlib.redirect_stdout(io.StringIO()):
        loop.run()
    means = [float(m) for m in means]
    print("population mean every 20th generation", [round(m, 3) for m in means[::20]], "max", max(means))
    assert len(means) == LEARNING_GENERATIONS and means[0] < -10.0
    assert max(means) > 0.5 * RECORDED_FINAL_MEAN, max(means)
