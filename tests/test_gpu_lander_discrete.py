"""LunarLander-v2 (csrc/ses_lander_discrete.hip: the lander's world step behind an argmax head) on the HIP path: every rollout
form the continuous lander runs, the int32 step-wise env and the wrapper's playback, bit for bit against a Python rollout
composed from the oracle (tests/lander_discrete_np.py); the continuous sibling next to it; conf/lunarlander_v2_openai.yaml end
to end.  22 offspring: a partly filled last wave at 2 and at 4 offspring per wave and a partly filled workgroup of four waves."""
import contextlib
import io
import os
from copy import deepcopy

import numpy as np
import pytest
import torch
import yaml

import lander_discrete_np as ld
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
N, MAX_STEP = 22, 120


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                 # (a copy: the shared references are read-only)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_rollout(gru, pomdp, E, knobs):
    from ses import HipES
    theta, init, w_fit, w_ret, w_steps, _ = ld.reference(gru, pomdp, E, N, MAX_STEP)
    es = HipES("LunarLander-v2", 8, 4, True, gru, pomdp=pomdp, max_step=MAX_STEP, eval_ep_num=E)
    for name, value in knobs.items():
        es.set_tuning(name, value)
    fit, ep_ret, ep_steps = es.rollout(dev(theta), dev(init), want_episodes=True)
    assert np.array_equal(ep_steps.cpu().numpy(), w_steps)
    assert np.array_equal(ep_ret.cpu().numpy().view(np.uint64), w_ret.view(np.uint64)), "episode returns differ from the harness"
    assert np.array_equal(bits(fit.cpu().numpy()), bits(w_fit))
    es.close()


@pytest.mark.parametrize("lpe,epw,pomdp", [(0, 0, False), (1, 0, True), (2, 0, False), (4, 0, True), (8, 0, False), (16, 0, True),
                                           (64, 0, False), (8, 5, True), (2, 20, False)])
def test_mlp_rollout_at_every_lane_count(lpe, epw, pomdp):
    """lpe: lanes per env (0 = the library's choice, 64 at this size); epw: different envs per wave (0 = 64 / lpe) -- with 5 envs on
    8 groups of 8 lanes and 20 on 32 pairs the lane groups past the last env shadow it, and the last wave is partly filled"""
    check_rollout(False, pomdp, 3, {"box2d_lanes_per_env": lpe, "box2d_envs_per_wave": epw})


GRU_FORMS = {"episode_parallel": {"gru_ep_parallel_max": 1000000},
             "sequential": {"gru_sequential": 1},
             "lockstep": {"gru_ep_parallel_max": 0, "lander_offspring_per_wave": 1},
             "lockstep_x2": {"gru_ep_parallel_max": 0, "lander_offspring_per_wave": 2},
             "lockstep_x4": {"gru_ep_parallel_max": 0, "lander_offspring_per_wave": 4}}


@pytest.mark.parametrize("E", [3, 5])
@pytest.mark.parametrize("form", list(GRU_FORMS))
def test_gru_rollout_in_every_form(form, E):
    check_rollout(True, True, E, GRU_FORMS[form])


@pytest.mark.parametrize("E,knobs", [(5, {"gru_ep_parallel_max": 0, "gru_mfma_min_e": 1}), (13, {"gru_ep_parallel_max": 0})],
                         ids=["E5_knob", "E13"])
def test_gru_rollout_on_the_matrix_cores(E, knobs):
    check_rollout(True, True, E, knobs)


@pytest.mark.parametrize("pomdp", [False, True])
def test_stepwise_env_takes_int32_actions(pomdp):
    from ses import HipES
    n, T = 70, 40
    es = HipES("LunarLander-v2", 8, 4, True, False, pomdp=pomdp, max_step=300, eval_ep_num=1)
    init = es.init_states_uniform(5, 1, 0, n)[:, 0].contiguous()
    state, obs = es.env_reset(init)
    masked = [2, 3, 5] if pomdp else []
    sims = [co.LanderSim() for _ in range(n)]
    want = np.stack([s.reset(u) for s, u in zip(sims, init.cpu().numpy())])
    want[:, masked] = 0.0
    assert np.array_equal(bits(obs.cpu().numpy()), bits(want))
    rng = np.random.RandomState(17 + int(pomdp))
    alive = np.ones(n, bool)
    for t in range(T):
        act = rng.randint(0, 4, size=n).astype(np.int32)
        o, r, d = es.env_step_generic(state, dev(act))
        o, r, d = o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()
        for i in np.flatnonzero(alive):
            wo, wr, wd = sims[i].step(*(float(x) for x in ld.ACTION_TABLE[act[i]]))
            wo[masked] = 0.0
            assert np.array_equal(bits(o[i]), bits(wo)), (t, i)
            assert bits(r[i:i + 1])[0] == bits(np.float32(wr))[0] and bool(d[i]) == wd, (t, i)
            alive[i] = alive[i] and not wd
    # a value outside 0 .. 3 acts as the no-op (include/ses.h)
    act = np.array([-1, 4, 7, -2 ** 31, 2 ** 31 - 1] * (n // 5), np.int32)
    o, r, d = es.env_step_generic(state, dev(act))
    o, r, d = o.cpu().numpy(), r.cpu().numpy(), d.cpu().numpy()
    for i in np.flatnonzero(alive):
        wo, wr, wd = sims[i].step(0.0, 0.0)
        wo[masked] = 0.0
        assert np.array_equal(bits(o[i]), bits(wo)) and bits(r[i:i + 1])[0] == bits(np.float32(wr))[0] and bool(d[i]) == wd, i
    assert alive.any()
    with pytest.raises(Exception, match="dtype"):
        es.env_step_generic(state, dev(np.zeros((n, 4), np.float32)))
    es.close()


def test_the_reference_playback_loop_plays_the_wrapper():
    """The reference's test.py loop (test.py:45-63) over GymWrapper("LunarLander-v2"): one transition per launch, the policy
    evaluated by the library's discrete head -- rewards and length equal the harness on the row the wrapper drew."""
    from envs.gym_wrapper import GymWrapper
    from networks.neural_network import GymEnvModel
    env = GymWrapper("LunarLander-v2", max_step=MAX_STEP)
    net = GymEnvModel(8, 4, True, False)
    rng = np.random.RandomState(7)
    net.load_flat((rng.randn(net.param_count()) * 0.4).astype(np.float32))
    model = deepcopy(net)
    model.eval()
    model.reset()
    obs = env.reset()
    done, rewards = False, []
    while not done:
        action = {"0": model(obs["0"]["state"][np.newaxis, ...])}
        assert action["0"].dtype == np.int64 and 0 <= int(action["0"]) <= 3
        obs, r, done, _ = env.step(action)
        rewards.append(r)
    row = env._device().init_states_uniform(0, 0, 0, 1)[0, 0].cpu().numpy()
    trace = []
    total, steps = ld.episode(co.LanderSim(), net.flat(), row, MAX_STEP, False, 0, True, trace)
    assert len(rewards) == steps
    assert np.array_equal(np.array(rewards, np.float64).view(np.uint64), np.array([r for _, r in trace], np.float64).view(np.uint64))
    assert sum(rewards) == total
    env.close()


def test_continuous_sibling_is_unchanged_next_to_a_discrete_handle():
    from ses import HipES
    theta, init, w_fit, _, _, _ = ld.reference(False, False, 3, N, MAX_STEP)
    disc = HipES("LunarLander-v2", 8, 4, True, False, max_step=MAX_STEP, eval_ep_num=3)
    d_fit = disc.rollout(dev(theta), dev(init))
    cont = HipES("LunarLanderContinuous-v2", 8, 4, False, False, max_step=MAX_STEP, eval_ep_num=3)
    fit, ep_ret, ep_steps = cont.rollout(dev(theta), dev(init), want_episodes=True)
    o_fit, o_ret, o_steps = co.rollout_lander(theta, init, 3, MAX_STEP, gru=False, obs_mask=0)
    assert np.array_equal(ep_steps.cpu().numpy(), o_steps)
    assert np.array_equal(ep_ret.cpu().numpy().view(np.uint64), o_ret.view(np.uint64))
    assert np.array_equal(bits(fit.cpu().numpy()), bits(o_fit))
    assert np.array_equal(bits(disc.rollout(dev(theta), dev(init)).cpu().numpy()), bits(w_fit))   # and the other way round
    assert np.array_equal(bits(d_fit.cpu().numpy()), bits(w_fit))
    disc.close()
    cont.close()


def test_lunarlander_v2_openai_yaml_improves(tmp_path, monkeypatch):
    """BASELINE config 3 as worded, at 512 offspring: 60 generations of 5 episodes.  Observed on one MI355X: see
    profiles/lander_discrete_learning.txt."""
    import builder
    monkeypatch.chdir(tmp_path)
    cfg = yaml.load(open(os.path.join(SRC, "conf", "lunarlander_v2_openai.yaml")), Loader=yaml.FullLoader)
    cfg["strategy"]["offspring_num"] = 512
    loop = builder.build_loop(cfg, 60, 1, 5, False, 10 ** 9)
    with contextlib.redirect_stdout(io.StringIO()):
        loop.run()
    best = [b for b, _ in loop.history]
    print("best return per generation:", " ".join(f"{b:.1f}" for b in best))
    print(f"first 5: {np.mean(best[:5]):.2f}, last 10: {np.mean(best[-10:]):.2f}")
    assert np.mean(best[-10:]) > np.mean(best[:5]) + 50, best[::5]
