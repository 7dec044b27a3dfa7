"""BipedalWalkerHardcore-v3 on the HIP path (csrc/ses_walker_hardcore.hip) against the host build of the same env text
(tests/walker_hardcore_host.py), bit for bit: the step-wise env from reset and from states placed on every kind of obstacle edge, the
fused MLP rollout at every lanes-per-env setting with the envs per wave forced, both init forms and the plan's default shape, the GRU
rollout and ses_policy_forward at gru = 1, the device loop against per-generation calls, the wrapper's playback, and the refusals.

The rollout inputs are the 20 trained walker policies of tests/golden/g10_box2d_mlp.npz (rows 12 - 31 of walker_theta) x its 3 init
rows at 250 steps: on BipedalWalker-v3 59 of those 60 pairs carry the hull past x = 9.8 m by step 138, and the first obstacle starts at
9.33 m; the fixture asserts on the host build that at least 30 pairs put a leg on an obstacle edge (57 do)."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch

import walker_hardcore_host as hh
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = hh.NAME
H, STEP = float(hh.TERRAIN_HEIGHT), float(hh.STEP)
T = 250


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def handle(gru=False, E=1, max_step=T):
    from ses import HipES
    return HipES(NAME, hh.S, hh.A, False, gru, max_step=max_step, eval_ep_num=E)


def _step_both(es, state, sims, actions):
    """every row of actions [T, n, 4] on the device blobs and on the host sims: observations, rewards and dones equal bit for bit,
    through and past the ends of episodes; returns how many envs ended"""
    ended = np.zeros(len(sims), bool)
    for t, a in enumerate(actions):
        obs, reward, done = es.env_step_generic(state, dev(a))
        w = [s.step(a[i]) for i, s in enumerate(sims)]
        assert np.array_equal(bits(obs.cpu().numpy()), bits(np.stack([x[0] for x in w]))), t
        assert np.array_equal(bits(reward.cpu().numpy()), bits(np.array([x[1] for x in w], np.float32))), t
        assert np.array_equal(done.cpu().numpy() != 0, np.array([x[2] for x in w])), t
        ended |= np.array([x[2] for x in w])
    return int(ended.sum())


def test_stepwise_env_from_reset_equals_the_host_build():
    es = handle()
    n = 8
    assert es.env_state_bytes() == hh.lib().bwh_blob_size() and es.env_obs_width() == 24 and es.init_dim == 4
    init = es.init_states_uniform(9, 0, 0, n)[:, 0].contiguous()
    want_init = co.init_states_uniform(9, 0, 0, n, 1, 4, False, 0.0, 1.0)[:, 0]
    assert np.array_equal(bits(init.cpu().numpy()), bits(want_init))
    state, obs = es.env_reset(init)
    sims = [hh.HardcoreSim() for _ in range(n)]
    w_obs = np.stack([s.reset(want_init[i]) for i, s in enumerate(sims)])
    assert np.array_equal(bits(obs.cpu().numpy()), bits(w_obs))
    # the terrain rows the device generated: heights, riser counts and edge columns, byte for byte
    row_bytes = 4 * hh.lib().bwh_row_floats()
    got_rows = state.cpu().numpy()[:, -row_bytes:]
    for i, s in enumerate(sims):
        assert np.array_equal(got_rows[i], s.blob()[-row_bytes:]), i
    actions = np.random.default_rng(9).uniform(-1.0, 1.0, (40, n, 4)).astype(np.float32)
    actions[:, 0] *= 0.05                                                   # one env stays up, the others thrash
    _step_both(es, state, sims, actions)
    es.close()


def _placements():
    """host sims moved onto a stump's left riser, a stump top, a pit's lip, a pit floor and a stair riser: (label, sim)"""
    out = []

    def place(label, key, x, height):
        sim = hh.HardcoreSim()
        sim.reset(hh.init_row(key))
        sim.shift(x - float(sim.debug()["bodies"][0, 0]), height - H + 0.02)
        out.append((label, sim))

    wanted = {"stump": None, "pit": None, "stairs": None}
    for key in range(1, 200):
        row, kind = hh.row_generate(key)
        yl = row[:hh.COLS]
        if wanted["stump"] is None and (kind == hh.KIND_STUMP).any():
            c = int(np.flatnonzero(kind == hh.KIND_STUMP)[0])
            wanted["stump"] = (key, c, float(yl[c]), float(yl[c - 1]))
        if wanted["pit"] is None and (kind == hh.KIND_PIT_FLOOR).any():
            c = int(np.flatnonzero(kind == hh.KIND_PIT_FLOOR)[0])
            wanted["pit"] = (key, c, float(yl[c]), float(yl[c - 1]))
        if wanted["stairs"] is None and (kind == hh.KIND_TREAD).any():
            c = int(np.flatnonzero(kind == hh.KIND_TREAD)[0])
            wanted["stairs"] = (key, c, float(yl[c]), float(yl[c - 1]))
        if all(wanted.values()):
            break
    key, c, top, ground = wanted["stump"]
    place("stump riser", key, c * STEP, top)                               # the feet straddle the riser, level with the top
    place("stump top", key, (c + 0.5) * STEP, top)
    key, c, floor, lip = wanted["pit"]
    place("pit lip", key, c * STEP + 0.05, lip)                            # astride the lip's edge: one foot over the opening
    place("pit floor", key, (c + 1.0) * STEP, floor)
    key, c, tread, before = wanted["stairs"]
    place("stair riser", key, c * STEP + 0.05, max(tread, before))
    return out


def test_stepwise_env_on_every_obstacle_edge_equals_the_host_build():
    """states the host build made, uploaded as the device's: the smallest inputs that put every edge kind into the manifolds"""
    placed = _placements()
    sims = [s for _, s in placed]
    es = handle()
    state = dev(np.stack([s.blob() for s in sims]))
    assert state.shape == (5, es.env_state_bytes())
    rng = np.random.default_rng(4)
    actions = (rng.uniform(-1.0, 1.0, (40, 5, 4)) * 0.3).astype(np.float32)
    touched = np.zeros(5, bool)
    ended = 0
    for t0 in range(0, 40, 10):                                             # (the host's manifolds are looked at between the blocks)
        ended = max(ended, _step_both(es, state, sims, actions[t0:t0 + 10]))
        touched |= np.array([s.on_obstacle() for s in sims])
        if t0 == 0:
            first = [s.manifolds() for s in sims]
    assert touched.all(), [(label, bool(tch)) for (label, _), tch in zip(placed, touched)]
    # risers themselves were in the manifolds: an edge whose two ends share their abscissa
    on_riser = 0
    for s, (flags, edges) in zip(sims, first):
        e = hh.row_edges(s.terrain()[0])
        on_riser += sum(int(e[k, 0] == e[k, 2]) for k in edges[flags == 1])
    assert on_riser > 0
    es.close()


@pytest.fixture(scope="module")
def mlp_reference():
    """the 20 trained walker policies x the 3 golden init rows, 250 steps, on the host build, once: shared init rows and one row set
    per offspring (the same rows, rotated by the offspring's number)"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "g10_box2d_mlp.npz"))
    theta, init = np.ascontiguousarray(g["walker_theta"][12:32]), np.ascontiguousarray(g["walker_init"])
    assert theta.shape == (20, co.param_count(24, 4, False)) and init.shape == (3, 4)
    touched = np.zeros((20, 3), bool)
    shared = hh.rollout(theta, init, 3, T, touched=touched)
    print("pairs with a leg manifold on an obstacle edge within 250 steps:", int(touched.sum()), "of 60")
    assert touched.sum() >= 30
    steps = shared[2]
    assert (steps == T).any() and (steps < T).any()
    init_per = np.stack([np.roll(init, i, axis=0) for i in range(20)])
    per = hh.rollout(theta, init_per, 3, T)
    for i in range(20):                                                     # the rotation only moves episodes around
        assert np.array_equal(bits(per[1][i]), bits(np.roll(shared[1][i], i)))
    return theta, init, init_per, shared, per


def _check(es, theta, init, want):
    fit, ep_ret, ep_steps = es.rollout(dev(theta), dev(init), want_episodes=True)
    w_fit, w_ret, w_steps = want
    assert np.array_equal(ep_steps.cpu().numpy(), w_steps), (ep_steps.cpu().numpy(), w_steps)
    assert np.array_equal(bits(ep_ret.cpu().numpy()), bits(w_ret))
    assert np.array_equal(bits(fit.cpu().numpy()), bits(w_fit))


# every lanes-per-env setting with 1, 3 and the most envs per wave it admits (3 does not fit 64 or 32 lanes per env)
SHAPES = sorted({(lpe, min(epw, 64 // lpe)) for lpe in (1, 2, 4, 8, 16, 32, 64) for epw in (1, 3, 64)})


@pytest.mark.parametrize("lpe,epw", SHAPES, ids=[f"lpe{l}-epw{e}" for l, e in SHAPES])
def test_mlp_rollout_at_a_forced_shape_equals_the_host_build(mlp_reference, lpe, epw):
    """60 envs: with 3 envs per wave the waves are full, with the most per wave the last lane groups of the last wave shadow"""
    theta, init, _, shared, _ = mlp_reference
    es = handle(False, 3)
    es.set_tuning("box2d_lanes_per_env", lpe)
    es.set_tuning("box2d_envs_per_wave", epw)
    _check(es, theta, init, shared)
    es.close()


@pytest.mark.parametrize("form", ["shared", "per_offspring"])
def test_mlp_rollout_at_the_plans_shape_equals_the_host_build(mlp_reference, form):
    theta, init, init_per, shared, per = mlp_reference
    es = handle(False, 3)
    if form == "shared":
        _check(es, theta, init, shared)
    else:
        _check(es, theta, init_per, per)
        es.set_tuning("box2d_lanes_per_env", 2)                             # ... and at a shape with several envs per wave
        _check(es, theta[:19], init_per[:19], tuple(x[:19] for x in per))   # 57 envs: the last wave is not full
    es.close()


@pytest.mark.parametrize("E", [1, 2, 3, 4, 5])
def test_gru_rollout_equals_the_host_build(E):
    P = co.param_count(24, 4, True)
    rng = np.random.default_rng(E)
    theta = (rng.standard_normal((6, P)) * 0.3).astype(np.float32)
    init = co.init_states_uniform(E, 0, 0, 6, E, 4, False, 0.0, 1.0)
    want = hh.rollout(theta, init, E, 60, gru=True)
    es = handle(True, E, 60)
    _check(es, theta, init, want)
    es.close()


def test_gru_rollout_over_obstacles_equals_the_host_build():
    """Random GRU policies fall on the start pad within 60 steps, so the cases above never put an obstacle edge under the lockstep
    body.  These four random-weight policies (found by a search over 750 on the host build) get their second episode to the first
    obstacle within 400 steps: the eight-slot contact path under k_bwh_gru_ls, two episodes of unequal length in one wave."""
    P = co.param_count(24, 4, True)
    theta = np.concatenate([(np.random.default_rng(1000 + seed).standard_normal((1, P)) * scale).astype(np.float32)
                            for scale, seed in ((0.6, 75), (1.0, 27), (1.0, 51), (1.0, 177))])
    init = co.init_states_uniform(7, 0, 0, 1, 2, 4, False, 0.0, 1.0)[0]
    touched = np.zeros((4, 2), bool)
    want = hh.rollout(theta, init, 2, 400, gru=True, touched=touched)
    print("GRU (policy, episode) pairs with a leg manifold on an obstacle edge:", int(touched.sum()), "of 8")
    assert touched[:, 1].all(), touched
    es = handle(True, 2, 400)
    _check(es, theta, init, want)
    es.close()


def test_policy_forward_gru_equals_the_oracle():
    P = co.param_count(24, 4, True)
    rng = np.random.default_rng(0)
    n = 37
    theta = (rng.standard_normal((n, P)) * 0.3).astype(np.float32)
    obs = rng.standard_normal((n, 24)).astype(np.float32)
    hid = (rng.standard_normal((n, co.HIDDEN)) * 0.5).astype(np.float32)
    w_action, w_logits, w_act, w_h = co.policy_forward(24, 4, False, True, theta, obs, hid.copy())
    es = handle(True, 1, 60)
    h = dev(hid)
    _, logits, act = es.policy_forward(dev(theta), dev(obs), h)
    assert np.array_equal(bits(logits.cpu().numpy()), bits(w_logits))
    assert np.array_equal(bits(act.cpu().numpy()), bits(w_act))
    assert np.array_equal(bits(h.cpu().numpy()), bits(w_h))
    es.close()


def test_device_loop_equals_three_per_generation_calls(tmp_path, monkeypatch):
    """openai_es, 8 offspring, three generations of 40 steps through ses_run_generations and generation by generation: identical
    histories, populations and elites."""
    import builder
    monkeypatch.chdir(tmp_path)
    cfg = {"env": {"name": NAME, "max_step": 40, "pomdp": False, "seed": 3},
           "network": {"name": "gym_model", "num_state": 24, "num_action": 4, "discrete_action": False, "gru": False},
           "strategy": {"name": "openai_es", "init_sigma": 0.2, "sigma_decay": 0.999, "learning_rate": 0.05, "offspring_num": 8, "seed": 1}}
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SES_BATCH_GENERATIONS", mode)
        loop = builder.build_loop(cfg, 3, 1, 2, False, 10 ** 9)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            pop = loop.run()
        assert "box2d-restated" in out.getvalue()
        runs[mode] = (list(loop.history), pop.theta.cpu().numpy(), loop.offspring_strategy.get_elite_model().flat())
    (h0, t0, m0), (h1, t1, m1) = runs["0"], runs["1"]
    assert len(h0) == 3 and h0 == h1
    assert np.array_equal(bits(t0), bits(t1)) and np.array_equal(bits(m0), bits(m1))


def test_wrapper_playback_equals_the_host_build_and_the_fused_rollout():
    from envs.gym_wrapper import GymWrapper
    from learning_strategies.evolution.loop import RolloutWorker
    from networks.neural_network import GymEnvModel
    Tw = 60
    env = GymWrapper(NAME, Tw)
    es = handle(False, 1, Tw)
    want_init = co.init_states_uniform(0, 0, 0, 1, 1, 4, False, 0.0, 1.0)[0, 0]
    sim = hh.HardcoreSim()
    obs = env.reset()["0"]["state"]
    assert np.array_equal(bits(obs), bits(sim.reset(want_init)))
    rng = np.random.default_rng(2)
    for t in range(Tw):
        a = (rng.uniform(-1.0, 1.0, 4) * 0.05).astype(np.float32)
        tr, r, done, _ = env.step({"0": a})
        w_obs, w_r, w_done = sim.step(a)
        assert np.array_equal(bits(tr["0"]["state"]), bits(w_obs)) and np.float32(r) == w_r, t
        assert done == (w_done or t + 1 >= Tw), t
        if done:
            break
    assert t > 20
    g = np.load(os.path.join(ROOT, "tests", "golden", "g10_box2d_mlp.npz"))
    net = GymEnvModel(24, 4, False, False)
    net.load_flat(np.ascontiguousarray(g["walker_theta"][20]))
    k = env._episode
    got = RolloutWorker((env, {"0": net}, 1))                               # the reference's loop, step by step
    init = es.init_states_uniform(0, k, 0, 1)
    fit, _, _ = es.rollout(dev(net.flat()[None, :]), init, want_episodes=True)
    assert got == float(fit[0].item())
    w_fit, _, _ = hh.rollout(net.flat()[None, :], init.cpu().numpy(), 1, Tw)
    assert np.float32(got) == w_fit[0]
    # a GRU policy through the same loop: the network's own handle has no env, so ses_policy_forward serves (24, 4) at gru = 1 by shape
    gnet = GymEnvModel(24, 4, False, True)
    gnet.load_flat((np.random.default_rng(1027).standard_normal(co.param_count(24, 4, True)) * 1.0).astype(np.float32))
    k = env._episode
    got = RolloutWorker((env, {"0": gnet}, 1))
    es_gru = handle(True, 1, Tw)
    init = es_gru.init_states_uniform(0, k, 0, 1)
    fit, _, _ = es_gru.rollout(dev(gnet.flat()[None, :]), init, want_episodes=True)
    assert got == float(fit[0].item())
    es_gru.close()
    with pytest.raises(NotImplementedError, match="CartPole.*LunarLander.*BipedalWalker-v3.*simple_spread"):      # no scene for this name
        env.render()
    es.close()
    env.close()


def test_refusals_are_by_name():
    from envs.gym_wrapper import GymWrapper
    from ses import HipES, SesError
    from ses._lib import MODE_FIXED_LENGTH
    for bad, word in ((dict(num_state=23), "num_state"), (dict(num_action=5), "num_action"), (dict(discrete_action=True), "discrete_action"),
                      (dict(pomdp=True), "pomdp"), (dict(physics64=True), "physics64")):
        kw = dict(num_state=24, num_action=4, discrete_action=False, gru=False, max_step=10, eval_ep_num=1)
        kw.update(bad)
        with pytest.raises(SesError, match="BipedalWalkerHardcore-v3.*" + word):
            HipES(NAME, **kw)
    with pytest.raises(AssertionError):
        GymWrapper(NAME, None, pomdp=True)
    for gru in (False, True):
        es = handle(gru, 1, 10)
        theta = dev(np.zeros((2, co.param_count(24, 4, gru)), np.float32))
        init = es.init_states_uniform(1, 0, 0, 1, shared=True)[0].contiguous()
        with pytest.raises(SesError, match="BipedalWalkerHardcore-v3 has no fixed-length mode"):
            es.rollout(theta, init, mode=MODE_FIXED_LENGTH)
        es.close()
