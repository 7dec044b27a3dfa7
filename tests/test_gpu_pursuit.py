"""pursuit (csrc/ses_pursuit.h, csrc/ses_pursuit.hip) on the HIP path against the numpy restatement (tests/pursuit_np.py): the
step-wise env, ses_policy_forward at (147, 5), the fused rollout with fc1 on the matrix cores and on the VALU, early termination
inside a tile, the wrapper's playback and conf/pursuit.yaml through ESLoop.  Every comparison is on bit patterns: the env is
integers and the policy is the canonical chain.  The inputs are the restatement's own (tests/test_pursuit_host.py asserts that they
reach every event of the env)."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch
import yaml

import pursuit_np as pu
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                 # (a copy: the shared references are read-only)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def handle(E=1, max_step=500):
    from ses import HipES
    return HipES("pursuit", 147, 5, True, False, max_step=max_step, eval_ep_num=E, n_agents=8)


def test_stepwise_env_matches_the_restatement():
    init, acts, obs, rews, dones, _ = pu.stepwise_reference()
    n = init.shape[0]
    assert n == 37
    es = handle()
    assert es.env_obs_width() == 8 * 147 and es.env_state_bytes() == 96 and es.init_dim == 40
    state, o = es.env_reset(dev(init))
    assert np.array_equal(bits(o.cpu().numpy().reshape(n, 8, 147)), bits(obs[0])), "reset observations differ"
    for t in range(pu.STEPWISE_CYCLES):
        o, r, d = es.env_step_generic(state, dev(acts[t]))
        assert np.array_equal(bits(o.cpu().numpy().reshape(n, 8, 147)), bits(obs[t + 1])), t
        assert np.array_equal(bits(r.cpu().numpy()), bits(rews[t])), t
        assert np.array_equal(d.cpu().numpy() != 0, dones[t]), t
    assert any(d.any() for d in dones) and not all(d.all() for d in dones)
    with pytest.raises(Exception, match="shape"):
        es.env_step_generic(state, dev(np.zeros((n, 5), np.int32)))
    es.close()


def test_reset_observations_of_crafted_rows():
    """all actors in one cell; actors on every edge and beside the block; absent evaders"""
    rows = pu.crafted_rows()
    want = pu.Pursuit(rows).observe()
    es = handle()
    _, o = es.env_reset(dev(rows))
    got = o.cpu().numpy().reshape(len(rows), 8, 147)
    assert np.array_equal(bits(got), bits(want))
    one_cell = list(pu.CRAFTED).index("one_cell")
    assert (got[one_cell, :, (3 * 7 + 3) * 3 + 1] == 8).all() and (got[one_cell, :, (3 * 7 + 3) * 3 + 2] == 30).all()
    es.close()


def test_policy_forward_at_147_inputs():
    rng = np.random.RandomState(4)
    n = 64
    theta = pu.thetas(n, 5)
    obs = pu.Pursuit(co.init_states_uniform(3, 0, 0, 8, 1, 40, False, 0.0, 1.0)[:, 0]).observe().reshape(n, 147).copy()
    obs[8:16] = rng.randn(8, 147).astype(np.float32) * 30.0
    obs[16] = 0.0
    obs[17] = 1.0
    obs[19] = 1.0e30
    obs[20, ::2] = -1.0e30
    obs[21] = np.float32(1.0e-40)                                # subnormal inputs
    # ties between logits: fc2 rows 1 and 3 equal to row 0 (logits 0 = 1 = 3), and in another policy all five rows equal
    w2 = 32 * 147 + 32
    for row, same in ((24, (1, 3)), (25, (1, 2, 3, 4)), (26, (4,))):
        for o in same:
            theta[row, w2 + 32 * o:w2 + 32 * o + 32] = theta[row, w2:w2 + 32]
            theta[row, w2 + 160 + o] = theta[row, w2 + 160]
    # a row whose fc1 accumulator is -0 throughout: b1 = -0, zero observations (every product w * (+0) added to -0 ...) -- and one
    # whose products are all -0 as well: weights >= 0, observations -0
    theta[27, 32 * 147:32 * 147 + 32] = -0.0
    obs[27] = 0.0
    theta[28, :32 * 147] = np.abs(theta[28, :32 * 147])
    theta[28, 32 * 147:32 * 147 + 32] = -0.0
    obs[28] = -0.0
    w_action, w_logits, w_act, _ = co.policy_forward(147, 5, True, False, theta, obs)
    assert w_action[25] == 0 and w_logits[24, 0] == w_logits[24, 1] == w_logits[24, 3]
    from ses import HipES
    for es in (handle(), HipES(None, 147, 5, True, False)):      # the env's handle and one without an env
        action, logits, act = es.policy_forward(dev(theta), dev(obs))
        assert np.array_equal(bits(logits.cpu().numpy()), bits(w_logits))
        assert np.array_equal(bits(act.cpu().numpy()), bits(w_act))
        assert np.array_equal(action.cpu().numpy(), w_action)
        es.close()
    assert len(set(w_action.tolist())) == 5


CASES = [(E, n) for E in pu.FUSED_E for n in pu.FUSED_N]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "E%d_n%d" % c)
def test_fused_rollout_matches_the_restatement_in_both_fc1_forms(case):
    E, n = case
    theta, init, w_fit, w_ret, w_steps, _ = pu.fused_reference(E, n)
    es = handle(E, pu.FUSED_MAX_STEP)
    got = {}
    for mfma in (1, 0):
        es.set_tuning("pursuit_fc1_mfma", mfma)
        fit, ep_ret, ep_steps = es.rollout(dev(theta), dev(init), want_episodes=True)
        got[mfma] = (ep_ret.cpu().numpy().view(np.uint64), ep_steps.cpu().numpy(), bits(fit.cpu().numpy()))
        assert np.array_equal(got[mfma][0], w_ret.view(np.uint64)), "episode returns differ from the restatement (mfma=%d)" % mfma
        assert np.array_equal(got[mfma][1], w_steps), mfma
        assert np.array_equal(got[mfma][2], bits(w_fit)), mfma
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a, b)
    es.close()


def test_knob_values_and_shared_init_rows():
    E, n = 5, 5
    theta, init, w_fit, _, _, _ = pu.fused_reference(E, n)
    es = handle(E, pu.FUSED_MAX_STEP)
    for knob in (None, -1, 0, 1):
        if knob is not None:
            es.set_tuning("pursuit_fc1_mfma", knob)
        fit = es.rollout(dev(theta), dev(init))
        assert np.array_equal(bits(fit.cpu().numpy()), bits(w_fit)), knob
    with pytest.raises(Exception, match="pursuit_fc1_mfma"):
        es.set_tuning("pursuit_fc1_mfma", 2)
    # one init row set shared by all offspring
    shared = np.array(init[2])
    want, _, _, _ = pu.rollout(theta, shared, E, pu.FUSED_MAX_STEP)
    fit = es.rollout(dev(theta), dev(shared))
    assert np.array_equal(bits(fit.cpu().numpy()), bits(want))
    es.close()


@pytest.mark.parametrize("mfma", [1, 0], ids=["mfma", "valu"])
def test_episodes_end_early_beside_tile_mates_that_run_on(mfma):
    """Boxed evaders (pursuit_np.early_inputs): of an offspring's five episodes, 0, 1 and 3 end in the first cycle in which their
    evaders stay put, while 2 (same tile as 0, 1, 3) and 4 run to max_step."""
    theta, init = pu.early_inputs()
    E, T = 5, pu.FUSED_MAX_STEP
    w_fit, w_ret, w_steps, _ = pu.rollout(theta, init, E, T)
    es = handle(E, T)
    es.set_tuning("pursuit_fc1_mfma", mfma)
    fit, ep_ret, ep_steps = es.rollout(dev(theta), dev(init), want_episodes=True)
    steps = ep_steps.cpu().numpy()
    assert (steps[:, 2] == T).all() and (steps[:, 4] == T).all()
    assert (steps[:, [0, 1, 3]] < T).sum() >= 8 and len(set(steps[:, [0, 1, 3]].ravel().tolist())) >= 4
    assert np.array_equal(steps, w_steps)
    assert np.array_equal(ep_ret.cpu().numpy().view(np.uint64), w_ret.view(np.uint64))
    assert np.array_equal(bits(fit.cpu().numpy()), bits(w_fit))
    es.close()


def test_handle_refuses_what_the_env_does_not_run():
    from ses import HipES
    ok = dict(num_state=147, num_action=5, discrete_action=True, gru=False, pomdp=False, n_agents=8, eval_ep_num=5)
    for kw, says in ((dict(gru=True), "GRU"), (dict(pomdp=True), "pomdp"), (dict(discrete_action=False), "discrete_action=1"),
                     (dict(num_state=146), "num_state=147"), (dict(num_action=4), "num_action=5"), (dict(n_agents=5), "n_agents=8"),
                     (dict(n_agents=1), "n_agents=8"), (dict(eval_ep_num=17), "eval_ep_num"), (dict(physics64=True), "physics64")):
        a = dict(ok, **kw)
        with pytest.raises(Exception, match="pursuit.*" + says):
            HipES("pursuit", a["num_state"], a["num_action"], a["discrete_action"], a["gru"], pomdp=a["pomdp"], max_step=500,
                  eval_ep_num=a["eval_ep_num"], n_agents=a["n_agents"], physics64=a.get("physics64", False))
    for E in (1, 16):
        handle(E).close()
    with pytest.raises(Exception):
        HipES(None, 147, 5, True, True)                          # the env-less (147, 5) handle is the MLP's


def test_wrapper_playback_equals_the_fused_rollout():
    """One team played through PettingzooWrapper by the reference's playback loop (a model per agent on obs[agent]["state"], the
    dict of actions stepped, r added up): every cycle's reward is the restatement's float64 team reward rounded to float, the
    episode is as long as the fused rollout's, and the two totals differ by the roundings to float only: at most 2^-24 of the sum
    of the rewards' magnitudes."""
    from envs.pettingzoo_wrapper import PettingzooWrapper
    T = 40
    theta = pu.thetas(1, 31)
    env = PettingzooWrapper("pursuit", T)
    obs = env.reset()
    rewards, done, episode_reward, ep_step = [], False, 0, 0
    while not done:
        actions = {}
        for k in env.get_agent_ids():
            s = obs[k]["state"][np.newaxis, ...]
            actions[k] = co.policy_forward(147, 5, True, False, theta, s)[0][0]
        obs, r, done, _ = env.step(actions)
        rewards.append(r)
        episode_reward += r
        ep_step += 1
    es = handle(1, T)
    init = es.init_states_uniform(0, 0, 0, 1)
    ref = pu.Pursuit(init.cpu().numpy()[0])
    want = []
    for _ in range(T):
        r, d = ref.step(pu.policy_actions(theta, ref.observe()))
        want.append(np.float32(r[0]))
        if d[0]:
            break
    assert np.array_equal(bits(np.array(rewards, np.float32)), bits(np.array(want, np.float32)))
    fit, ep_ret, ep_steps = es.rollout(dev(theta), init, want_episodes=True)
    _, w_ret, w_steps, _ = pu.rollout(theta, init.cpu().numpy(), 1, T)
    assert np.array_equal(ep_ret.cpu().numpy().view(np.uint64), w_ret.view(np.uint64))
    assert ep_step == int(ep_steps[0, 0]) == int(w_steps[0, 0])
    assert abs(episode_reward - float(ep_ret[0, 0])) <= 2.0 ** -24 * float(np.sum(np.abs(np.array(rewards, np.float64)))) + 1e-12
    es.close()


def test_wrapper_reports_done_when_the_last_evader_is_caught():
    from envs.pettingzoo_wrapper import PettingzooWrapper
    env = PettingzooWrapper("pursuit", 500)
    env.reset()
    d = env._device()
    row = pu.craft(pursuers={0: (1, 0), 1: (0, 1)}, evaders={0: (0, 0)})
    env._state, _ = d.env_reset(dev(row[None]))
    ref = pu.Pursuit(row[None])
    for t in range(60):
        _, r, done, _ = env.step({a: 4 for a in env.get_agent_ids()})
        w_r, w_d = ref.step(np.full((1, 8), 4))
        assert np.float32(r) == np.float32(w_r[0]) and done == bool(w_d[0])
        if done:
            break
    assert done and t < 59


def test_training_loop_paths_agree_and_start_from_the_restatements_fitness(tmp_path, monkeypatch):
    """Three generations of conf/pursuit.yaml at 16 offspring, 2 episodes, 20 cycles: per generation (SES_BATCH_GENERATIONS=0) and
    through ses_run_generations -- identical parents, finite numbers; the first generation's fitness is the restatement's."""
    import builder
    monkeypatch.chdir(tmp_path)
    cfg = yaml.load(open(os.path.join(SRC, "conf", "pursuit.yaml")), Loader=yaml.FullLoader)
    cfg["env"]["max_step"] = 20
    cfg["strategy"]["offspring_num"] = 16
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("SES_BATCH_GENERATIONS", mode)
        loop = builder.build_loop(cfg, 3, 1, 2, False, 10 ** 9)
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            pop = loop.run()
        assert "pettingzoo-restated" in out.getvalue()
        runs[mode] = (list(loop.history), pop.theta.cpu().numpy(), loop.offspring_strategy.get_elite_model().flat(),
                      loop.batched_generations)
    (h0, t0, m0, b0), (h1, t1, m1, b1) = runs["0"], runs["1"]
    assert len(h0) == 3 and h0 == h1 and np.isfinite(np.array(h0, np.float64)).all()
    assert np.array_equal(bits(t0), bits(t1)) and np.array_equal(bits(m0), bits(m1)) and np.isfinite(t0).all()
    assert b0 == 0 and b1 > 0
    loop = builder.build_loop(cfg, 3, 1, 2, False, 10 ** 9)
    pop = loop.offspring_strategy.init_offspring(loop.network, loop.env.get_agent_ids())
    init = loop._init_states(pop.gen, pop.shard)
    fit = loop.dev.rollout(pop.theta, init)
    w_fit, _, _, _ = pu.rollout(pop.theta.cpu().numpy(), init.cpu().numpy(), 2, 20)
    assert np.array_equal(bits(fit.cpu().numpy()), bits(w_fit))
    assert np.float32(h0[0][0]) == w_fit.max()


def test_run_generations_of_three_equals_three_calls():
    """ses_run_generations with k = 3 against three calls with k = 1 (ESLoop.generations, the device-side loop): the next
    population, the mean and the optimizer's moments bit for bit."""
    import builder
    cfg = yaml.load(open(os.path.join(SRC, "conf", "pursuit.yaml")), Loader=yaml.FullLoader)
    cfg["env"]["max_step"] = 12
    cfg["strategy"]["offspring_num"] = 16
    outs = []
    for chunks in ((3,), (1, 1, 1)):
        loop = builder.build_loop(cfg, 3, 1, 2, False, 10 ** 9)
        strat = loop.offspring_strategy
        pop = strat.init_offspring(loop.network, loop.env.get_agent_ids())
        for k in chunks:
            pop = loop.generations(pop, k)
        torch.cuda.synchronize()
        assert loop._bench_batch[1] is not None, "the run did not go through ses_run_generations"
        outs.append([x.cpu().numpy().copy() for x in (pop.theta, strat.mu_model, strat.optimizer.m, strat.optimizer.v)])
    for a, b in zip(*outs):
        assert np.array_equal(bits(a), bits(b)) and np.isfinite(a).all()
    assert not np.array_equal(outs[0][1], np.zeros_like(outs[0][1]))
