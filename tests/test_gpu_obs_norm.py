"""The running observation normaliser on the device (include/ses.h: ses_obs_norm_bind / ses_obs_norm_merge) against
its numpy restatement (tests/obs_norm_np.py), bit for bit: the identity with the fresh state, the statistics, the normalised
rollout, stream order between rollouts, the merge on crafted partials, ses_run_generations, the loop with its checkpoints and
playback, and the refusals.

Shapes: 7 rows x 3 episodes = 21 envs -- at 1 lane per env 43 shadow lanes in the only wave, at 32 lanes per env 11 waves, the
last of them ragged -- and max_step 40, at every lanes-per-env and in both step forms; 90 x 3 = 270 envs once, so that some
lanes of the reduction add two terms; 1 x 1 once."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch
import yaml

import obs_norm_np as on
import pendula_np as pn
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
T = 40
N, E = 7, 3
ALL_LANES = (1, 2, 4, 8, 16, 32)
ACROBOT, MOUNTAINCAR, PENDULUM, MOUNTAINCAR_CONT = "Acrobot-v1", "MountainCar-v0", "Pendulum-v1", "MountainCarContinuous-v0"
BALANCE, SWINGUP, DOUBLE = "InvertedPendulumBulletEnv-v0", "InvertedPendulumSwingupBulletEnv-v0", "InvertedDoublePendulumBulletEnv-v0"
REACHER = "ReacherBulletEnv-v0"
# env -> the lanes per env its cases run at: every one for six envs, one each for the other two (all eight adapters are covered)
LANES = {ACROBOT: ALL_LANES, MOUNTAINCAR: ALL_LANES, PENDULUM: ALL_LANES, BALANCE: ALL_LANES, DOUBLE: ALL_LANES, REACHER: ALL_LANES,
         MOUNTAINCAR_CONT: (32,), SWINGUP: (4,)}
# env -> the tuning knob that picks its step form (0: one trig per step, 1: generic observe / step); the others have one form
FORM_KNOB = {PENDULUM: "pendulum_generic_step", BALANCE: "pendula_generic_step", SWINGUP: "pendula_generic_step",
             DOUBLE: "pendula_generic_step", REACHER: "reacher_generic_step"}
TERMINATES_EARLY = (BALANCE, DOUBLE)                                    # ~15 - 20 steps under random policies: frozen envs in every wave
NAMES = list(LANES)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, (what, bad[:4].tolist(), got.reshape(-1)[:4], want.reshape(-1)[:4])


def handle(name, lanes=0, form=None, n_ep=E, max_step=T, gru=False):
    from ses import HipES
    S, A, discrete = on.SHAPES[name]
    es = HipES(name, S, A, discrete, gru, max_step=max_step, eval_ep_num=n_ep, lanes_per_env=lanes)
    if form is not None:
        es.set_tuning(FORM_KNOB[name], form)
    return es


def variants(name):
    """(lanes per env, step form) of every kernel instance the env's cases run"""
    forms = (0, 1) if name in FORM_KNOB else (None,)
    return [(lanes, form) for lanes in LANES[name] for form in forms]


_CASE = {}


def case(name, n=N, n_ep=E, seed=3):
    """(theta float32[n, P] = randn * 0.5, init float32[n, n_ep, W], a per-offspring init), computed once"""
    key = (name, n, n_ep, seed)
    if key not in _CASE:
        S, A, _ = on.SHAPES[name]
        rng = np.random.default_rng(seed * 1000 + S * 10 + A)
        theta = (rng.standard_normal((n, co.param_count(S, A, False))) * 0.5).astype(np.float32)
        es = handle(name, n_ep=n_ep)
        init = host(es.init_states_uniform(17, seed, 5, n))
        es.close()
        _CASE[key] = (theta, init)
    return _CASE[key]


_REF = {}


def reference(name, affine, n=N, n_ep=E, seed=3, record_seen=False):
    """the restatement's rollout of case(...) under `affine`, computed once per (case, affine)"""
    key = (name, n, n_ep, seed, affine.tobytes(), record_seen)
    if key not in _REF:
        theta, init = case(name, n, n_ep, seed)
        _REF[key] = on.rollout(name, theta, init, n_ep, T, affine, record_seen)
    return _REF[key]


def run(es, theta, init):
    fit, ret, steps = es.rollout(dev(theta), dev(init), want_episodes=True)
    return host(fit), host(ret), host(steps)


def crafted_affine(S):
    """a shift of 0.75 on component 0, a scale of 0 on component 1, scales of 3.0 and 0.125 elsewhere"""
    affine = np.zeros((2, S), np.float32)
    affine[0, 0] = 0.75
    affine[1] = [3.0 if k % 2 == 0 else 0.125 for k in range(S)]
    affine[1, 1] = 0.0
    return affine


def used_stats(S):
    """the state of a run that has seen 1234 steps"""
    stats = np.zeros((S, 3), np.float64)
    stats[:, 0] = 1234.0
    stats[:, 1] = 0.05 * (np.arange(S) + 1.0)
    stats[:, 2] = 10.0 + np.arange(S)
    return stats


# ---- 1: the identity ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_fresh_state_without_update_is_the_identity(name):
    """fresh state, update off: fitness, returns and lengths bit-equal to the same handle's rollout with nothing bound; the
    state is not written"""
    theta, init = case(name)
    w_fit, w_ret, w_steps, _ = reference(name, on.fresh(on.SHAPES[name][0])[1])
    if name in TERMINATES_EARLY:
        assert (w_steps < T).mean() > 0.5
    for lanes, form in variants(name):
        es = handle(name, lanes, form)
        plain = run(es, theta, init)
        stats, affine = es.obs_norm_new()
        s0, a0 = host(stats).copy(), host(affine).copy()
        same(a0, on.fresh(es.S)[1], "obs_norm_new")
        es.obs_norm_bind(stats, affine, update=False)
        bound = run(es, theta, init)
        es.obs_norm_unbind()
        again = run(es, theta, init)
        for got, again_, want, ref, what in zip(bound, again, plain, (w_fit, w_ret, w_steps), ("fitness", "ep_return", "ep_steps")):
            same(got, want, (name, lanes, form, what))
            same(again_, want, (name, lanes, form, what, "after unbind"))
            same(want, ref, (name, lanes, form, what, "restatement"))
        same(host(stats), s0, (name, lanes, form, "stats untouched"))
        same(host(affine), a0, (name, lanes, form, "affine untouched"))
        es.close()


# ---- 2: the statistics -----------------------------------------------------------------------------------------------------------
def check_statistics(name, n, n_ep, lanes, form):
    S = on.SHAPES[name][0]
    theta, init = case(name, n, n_ep)
    fresh_stats, fresh_affine = on.fresh(S)
    w_fit, w_ret, w_steps, partials = reference(name, fresh_affine, n, n_ep)
    w_stats, w_affine = on.merge(fresh_stats, fresh_affine, partials)
    es = handle(name, lanes, form, n_ep=n_ep)
    plain = run(es, theta, init)
    stats, affine = es.obs_norm_new()
    es.obs_norm_bind(stats, affine, update=True)
    got = run(es, theta, init)
    for g, p, w, what in zip(got, plain, (w_fit, w_ret, w_steps), ("fitness", "ep_return", "ep_steps")):
        same(g, p, (name, n, lanes, form, what, "unbound"))
        same(g, w, (name, n, lanes, form, what, "restatement"))
    same(host(stats), w_stats, (name, n, lanes, form, "stats"))
    same(host(affine), w_affine, (name, n, lanes, form, "affine"))
    es.close()
    return w_stats, w_steps


@pytest.mark.parametrize("name", NAMES)
def test_statistics_from_the_fresh_state(name):
    for lanes, form in variants(name):
        w_stats, w_steps = check_statistics(name, N, E, lanes, form)
    assert (w_stats[:, 0] == w_steps.sum()).all() and w_steps.sum() > 0      # the count: steps taken, repeated per component
    if name in TERMINATES_EARLY:
        assert w_steps.sum() < 0.7 * N * E * T                              # most envs froze inside their wave


@pytest.mark.parametrize("name, n, n_ep, lanes", [(REACHER, 90, 3, 2), (PENDULUM, 90, 3, 0), (DOUBLE, 90, 3, 16),
                                                  (DOUBLE, 1, 1, 1), (REACHER, 1, 1, 32), (ACROBOT, 1, 1, 4)])
def test_statistics_at_270_envs_and_at_one(name, n, n_ep, lanes):
    """270 envs: reduction lanes 0 .. 13 add two terms; 1 x 1: one env, every other lane group shadows it"""
    check_statistics(name, n, n_ep, lanes, None)


# ---- 3: the normalised rollout ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_normalised_rollout_with_crafted_affine(name):
    """crafted shift and scales, update on, a state that is not fresh: returns, lengths, stats and affine against the
    restatement; what is accumulated is the RAW observation, not what the policy saw"""
    S = on.SHAPES[name][0]
    theta, init = case(name)
    affine0, stats0 = crafted_affine(S), used_stats(S)
    w_fit, w_ret, w_steps, partials = reference(name, affine0)
    w_stats, w_affine = on.merge(stats0, affine0, partials)
    # conditions on the restatement's own output that make the comparison worth something
    plain = reference(name, on.fresh(S)[1])
    assert not np.array_equal(bits(partials), bits(plain[3]))               # the crafted affine changes what the policies do
    seen_stats, _ = on.merge(stats0, affine0, reference(name, affine0, record_seen=True)[3])
    assert not np.array_equal(bits(seen_stats[:, 1:]), bits(w_stats[:, 1:]))   # raw and seen statistics differ on this data
    for lanes, form in variants(name):
        es = handle(name, lanes, form)
        stats, affine = dev(stats0), dev(affine0)
        es.obs_norm_bind(stats, affine, update=True)
        fit, ret, steps = run(es, theta, init)
        same(steps, w_steps, (name, lanes, form, "ep_steps"))
        same(ret, w_ret, (name, lanes, form, "ep_return"))
        same(fit, w_fit, (name, lanes, form, "fitness"))
        same(host(stats), w_stats, (name, lanes, form, "stats"))
        same(host(affine), w_affine, (name, lanes, form, "affine"))
        es.close()


# ---- 4: two rollouts back to back ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [ACROBOT, PENDULUM, DOUBLE, REACHER])
def test_second_rollout_reads_the_first_merge(name):
    """two rollouts enqueued with no synchronisation between them: the second runs on the affine the first's merge wrote"""
    S = on.SHAPES[name][0]
    theta, init = case(name)
    theta2, init2 = case(name, seed=4)
    stats0, affine0 = on.fresh(S)
    _, _, _, p1 = reference(name, affine0)
    stats1, affine1 = on.merge(stats0, affine0, p1)
    w_fit, w_ret, w_steps, p2 = on.rollout(name, theta2, init2, E, T, affine1)
    stats2, affine2 = on.merge(stats1, affine1, p2)
    assert not np.array_equal(bits(affine1), bits(affine0)) and not np.array_equal(bits(affine2), bits(affine1))
    for lanes in LANES[name][::2]:
        es = handle(name, lanes)
        stats, affine = es.obs_norm_new()
        es.obs_norm_bind(stats, affine, update=True)
        th1, in1, th2, in2 = dev(theta), dev(init), dev(theta2), dev(init2)
        es.rollout(th1, in1)
        fit, ret, steps = es.rollout(th2, in2, want_episodes=True)
        same(host(steps), w_steps, (name, lanes, "ep_steps"))
        same(host(ret), w_ret, (name, lanes, "ep_return"))
        same(host(fit), w_fit, (name, lanes, "fitness"))
        same(host(stats), stats2, (name, lanes, "stats"))
        same(host(affine), affine2, (name, lanes, "affine"))
        es.close()


# ---- 5: the merge alone ----------------------------------------------------------------------------------------------------------
def crafted_merge_inputs():
    """(stats0 float64[3, 3], partials float64[7, n_env]) for a Pendulum handle (S = 3): component 0 mean 0 / std 1, component 1
    mean 100 / std 0.01, component 2 a constant -- the data of tests/test_obs_norm_host.py -- 10007 envs of one step each"""
    rng = np.random.default_rng(5)
    n = 10007
    x = np.stack([rng.standard_normal(n).astype(np.float32), (100.0 + 0.01 * rng.standard_normal(n)).astype(np.float32),
                  np.full(n, 0.3, np.float32)]).astype(np.float64)
    return np.concatenate([np.ones((1, n)), x, x * x])


def test_merge_on_crafted_partials():
    es = handle(PENDULUM)
    partials = crafted_merge_inputs()
    cut = 6000
    stats, affine = es.obs_norm_new()
    w_stats, w_affine = on.fresh(3)
    for part in (partials[:, :cut], partials[:, cut:]):                    # two batches: from the fresh state, then onto it
        es.obs_norm_merge(dev(part), stats, affine)
        w_stats, w_affine = on.merge(w_stats, w_affine, np.ascontiguousarray(part))
        same(host(stats), w_stats, "stats")
        same(host(affine), w_affine, "affine")
    assert w_affine[1, 2] == 0.0 and w_affine[1, 0] > 0.0 and w_stats[0, 0] == 10007.0
    # a zero step count: nothing is written, whatever the sums say
    before = host(stats).copy(), host(affine).copy()
    empty = np.ascontiguousarray(partials[:, :300]).copy()
    empty[0] = 0.0
    es.obs_norm_merge(dev(empty), stats, affine)
    same(host(stats), before[0], "stats after an empty batch")
    same(host(affine), before[1], "affine after an empty batch")
    # std just below and just above 1e-7: N = 10, mean 0, the batch two observations of 0 -> M2 unchanged, std = sqrt(M2 / 9)
    for k, std in enumerate((0.99e-7, 1.01e-7, 1e-7)):
        s0 = np.zeros((3, 3), np.float64)
        s0[:, 0] = 8.0
        s0[:, 2] = np.float64(std) ** 2 * 9.0
        a0 = on.fresh(3)[1]
        p = np.zeros((7, 2), np.float64)
        p[0] = 1.0
        st, af = dev(s0), dev(a0)
        es.obs_norm_merge(dev(p), st, af)
        w_s, w_a = on.merge(s0, a0, p)
        same(host(st), w_s, ("floor", std, "stats"))
        same(host(af), w_a, ("floor", std, "affine"))
        if k < 2:
            assert (w_a[1] == 0.0).all() == (k == 0)
    # n_env of 1 and of exactly 256 / 257 (the lanes' second terms begin)
    rng = np.random.default_rng(9)
    for n_env in (1, 255, 256, 257):
        x = (rng.standard_normal((3, n_env)) * 10.0 ** rng.integers(-3, 4, (3, n_env))).astype(np.float32).astype(np.float64)
        p = np.concatenate([rng.integers(1, 40, (1, n_env)).astype(np.float64), x * 7.0, x * x * 7.0])
        st, af = dev(used_stats(3)), dev(crafted_affine(3))
        es.obs_norm_merge(dev(p), st, af)
        w_s, w_a = on.merge(used_stats(3), crafted_affine(3), p)
        same(host(st), w_s, (n_env, "stats"))
        same(host(af), w_a, (n_env, "affine"))
    es.close()


# ---- 6: ses_run_generations ------------------------------------------------------------------------------------------------------
def generations_cfg(strategy, name):
    S, A, discrete = on.SHAPES[name]
    s = {"name": strategy, "init_sigma": 0.3, "sigma_decay": 0.98, "learning_rate": 0.1, "offspring_num": 16, "seed": 2}
    if strategy == "ars":
        s["elite_num"] = 4
    return {"env": {"name": name, "max_step": T, "pomdp": False, "seed": 4},
            "network": {"name": "gym_model", "num_state": S, "num_action": A, "discrete_action": discrete, "gru": False, "obs_normalizer": True},
            "strategy": s}


@pytest.mark.parametrize("name", [PENDULUM, DOUBLE])
@pytest.mark.parametrize("strategy", ["ars", "openai_es"])
def test_run_generations_equals_per_generation_calls(strategy, name, tmp_path, monkeypatch):
    """k = 3 in one call against three per-generation calls: theta, mu, stats, affine and best[0 .. 2]"""
    import builder
    from learning_strategies.evolution.loop import _GenerationBatch
    monkeypatch.chdir(tmp_path)
    with contextlib.redirect_stdout(io.StringIO()):
        a = builder.build_loop(generations_cfg(strategy, name), 3, 1, 2, False, 10 ** 9)
        b = builder.build_loop(generations_cfg(strategy, name), 3, 1, 2, False, 10 ** 9)
    assert a.obs_norm is not None and b.obs_norm is not None
    pop = a.offspring_strategy.init_offspring(a.network, a.env.get_agent_ids())
    want_best = []
    for _ in range(3):
        pop, best, _sigma, _stamp = a.generation(pop)
        want_best.append(best.result())
    torch.cuda.synchronize()
    pop_b = b.offspring_strategy.init_offspring(b.network, b.env.get_agent_ids())
    assert _GenerationBatch.eligible(b, b.offspring_strategy, pop_b)
    batch = _GenerationBatch(b, b.offspring_strategy, pop_b)
    best, _stamps, _sigmas = batch.run(3)
    torch.cuda.synchronize()
    pop_b = batch.sync_back()
    assert [float(x) for x in best[:3]] == want_best, (best[:3], want_best)
    same(host(pop_b.theta), host(pop.theta), "theta")
    same(host(b.offspring_strategy.mu_model), host(a.offspring_strategy.mu_model), "mu")
    same(host(b.obs_norm[0]), host(a.obs_norm[0]), "stats")
    same(host(b.obs_norm[1]), host(a.obs_norm[1]), "affine")
    stats, affine = host(a.obs_norm[0]), host(a.obs_norm[1])
    assert np.abs(host(a.offspring_strategy.mu_model)).max() > 0
    assert (stats[:, 0] > 0).all() and (stats[:, 0] == stats[0, 0]).all()
    if name == PENDULUM:
        assert stats[0, 0] == 3 * 16 * 2 * T                               # it never terminates
    assert not np.array_equal(affine, on.fresh(affine.shape[1])[1])


# ---- 7: the loop, its checkpoints, playback ------------------------------------------------------------------------------------------
def test_loop_checkpoints_and_playback(tmp_path, monkeypatch):
    """conf/pendulum_swingup_ars_v2.yaml cut to 16 offspring and 50 steps, 3 generations, a checkpoint each: every checkpoint
    carries the normaliser as of its generation; playing ep_3.pt step by step over the wrapper and the module's forward walks
    the trajectory of the fused rollout of the same parameters, reset row and affine (update off).
    What is compared: the step-wise ABI carries (float)reward, so playback's return is the sum of float32-rounded rewards and
    cannot equal the fused float64 return bit for bit (tests/test_gpu_pendula.py bounds that difference by 2^-23 sum |r_t|).
    Both are therefore held, each bit for bit, to ONE restated trajectory -- the host loop below, normalising as the module
    does: its float64 reward sum is the fused rollout's return, its sum of float32-rounded rewards is playback's."""
    import builder
    from test_gpu_envs import playback
    monkeypatch.chdir(tmp_path)
    cfg = yaml.load(open(os.path.join(SRC, "conf", "pendulum_swingup_ars_v2.yaml")), Loader=yaml.FullLoader)
    cfg["strategy"].update(offspring_num=16, elite_num=4)
    cfg["env"]["max_step"] = 50
    n_ep = 2
    loop = builder.build_loop(cfg, 3, 1, n_ep, False, 1)
    with contextlib.redirect_stdout(io.StringIO()):
        loop.run()
    assert loop.batched_generations == 3                                    # the device-side loop, checkpoints by snapshot
    lines = [json.loads(l) for l in open(os.path.join(loop.save_dir, "metrics.jsonl"))]
    assert {"obs_normalizer": True} in lines[:2]
    sd = {g: torch.load(os.path.join(loop.save_dir, "saved_models", f"ep_{g}.pt")) for g in (1, 2, 3)}
    for g in (1, 2, 3):
        assert {"obs_norm_shift", "obs_norm_scale", "obs_norm_stats"} <= set(sd[g])
        assert sd[g]["obs_norm_stats"].dtype == torch.float64 and sd[g]["obs_norm_shift"].dtype == torch.float32
        assert float(sd[g]["obs_norm_stats"][0, 0]) == g * 16 * n_ep * 50, (g, sd[g]["obs_norm_stats"][:, 0])
    # the last checkpoint is the state the loop ends with
    same(sd[3]["obs_norm_stats"].numpy(), host(loop.obs_norm[0]), "ep_3 stats")
    same(np.stack([sd[3]["obs_norm_shift"].numpy(), sd[3]["obs_norm_scale"].numpy()]), host(loop.obs_norm[1]), "ep_3 affine")
    # and a checkpoint's affine is the merge of its own stats (same point of the stream)
    for g in (1, 2, 3):
        st = sd[g]["obs_norm_stats"].numpy()
        std = np.sqrt(st[:, 2] / (st[:, 0] - 1.0))
        want_scale = np.where(std < 1e-7, 0.0, 1.0 / std).astype(np.float32)
        same(sd[g]["obs_norm_scale"].numpy(), want_scale, (g, "scale of its own stats"))
        same(sd[g]["obs_norm_shift"].numpy(), st[:, 1].astype(np.float32), (g, "shift of its own stats"))

    env = builder.build_env(cfg["env"])
    net = builder.build_network(cfg["network"], cfg["env"]["name"])
    net.load_state_dict(sd[3])
    assert np.abs(net.flat()).max() > 0 and not np.array_equal(net.obs_norm_affine(), on.fresh(5)[1])
    affine = net.obs_norm_affine()
    (ret, steps), = playback(env, net, 1)
    env.close()
    # the fused rollout: same parameters, the reset row playback drew (env seed 0, episode 0, row 0), the same affine, frozen
    es = handle(SWINGUP, n_ep=1, max_step=50)
    init = es.init_states_uniform(0, 0, 0, 1)
    es.obs_norm_bind(dev(net.obs_norm_stats.numpy()), dev(affine), update=False)
    _, ep_ret, ep_steps = es.rollout(dev(net.flat()[None, :]), init, want_episodes=True)
    fused = host(ep_ret)[0, 0]
    assert steps == 50 and int(ep_steps[0, 0]) == 50
    # the restated trajectory
    s = pn.swingup_reset(host(init)[0])
    theta = net.flat()[None, :]
    sum64, sum32, sum_abs = np.float64(0.0), 0.0, 0.0
    for _ in range(50):
        _, _, act, _ = co.policy_forward(5, 1, False, False, theta, on.normalise(pn.pole_obs(s), affine), None)
        s, _, r, _ = pn.swingup_step(s, act)
        sum64 = sum64 + np.float64(r[0])
        sum32 += float(np.float32(r[0]))
        sum_abs += abs(float(r[0]))
    print("playback", ret, "fused", fused, "restated", sum32, float(sum64), "bound", 2.0 ** -23 * sum_abs)
    same(np.float64(fused), np.float64(sum64), "fused rollout against the restated trajectory")
    same(np.float64(ret), np.float64(sum32), "playback against the restated trajectory")
    assert abs(float(ret) - float(fused)) <= 2.0 ** -23 * sum_abs
    # RolloutWorker binds the model's affine too: its fitness is the fused return
    from learning_strategies.evolution.loop import RolloutWorker
    env2 = builder.build_env(cfg["env"])
    got = RolloutWorker((env2, {"0": net}, 1))
    assert got == float(np.float32(fused)), (got, fused)
    es.close()


# ---- 8: refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    from ses import HipES, SesError, _lib
    UNSUPPORTED = -2
    cart = HipES("CartPole-v1", 4, 2, True, False, max_step=50, eval_ep_num=1)
    stats, affine = cart.obs_norm_new()
    rc = cart._lib.ses_obs_norm_bind(cart._h, stats.data_ptr(), affine.data_ptr(), 1)
    assert rc == UNSUPPORTED and b"float64 envs" in cart._lib.ses_last_error()
    with pytest.raises(SesError):
        cart.obs_norm_bind(stats, affine)
    partials = cart.zeros(9, 4, dtype=torch.float64)
    assert cart._lib.ses_obs_norm_merge(cart._h, partials.data_ptr(), 4, stats.data_ptr(), affine.data_ptr()) == UNSUPPORTED
    cart.close()
    gru = handle(PENDULUM, gru=True)
    stats, affine = gru.obs_norm_new()
    rc = gru._lib.ses_obs_norm_bind(gru._h, stats.data_ptr(), affine.data_ptr(), 1)
    assert rc == UNSUPPORTED and b"GRU" in gru._lib.ses_last_error()
    assert gru._lib.ses_obs_norm_bind(gru._h, None, None, 0) == 0              # unbinding nothing is fine
    gru.close()
    es = handle(PENDULUM)
    stats, affine = es.obs_norm_new()
    for bad_stats, bad_affine in ((es.zeros(3, 3), affine), (es.zeros(3, 2, dtype=torch.float64), affine), (stats, es.zeros(3, 2)),
                                  (stats, es.zeros(2, 3, dtype=torch.float64)), (stats.cpu(), affine), (stats, None)):
        with pytest.raises(SesError):
            es.obs_norm_bind(bad_stats, bad_affine)
    with pytest.raises(SesError):
        es.obs_norm_merge(es.zeros(6, 10, dtype=torch.float64), stats, affine)    # 2 S + 1 = 7 rows
    with pytest.raises(SesError):
        es.obs_norm_merge(es.zeros(7, 10), stats, affine)
    # nothing of the above bound anything: a rollout is the unbound one
    theta, init = case(PENDULUM)
    plain = run(es, theta, init)
    w = reference(PENDULUM, on.fresh(3)[1])
    same(plain[1], w[1], "ep_return")
    es.close()
    # the builder refuses where the env name is known, before a handle exists
    import builder
    cfg = generations_cfg("openai_es", PENDULUM)
    cfg["env"]["name"] = "CartPole-v1"
    with pytest.raises(ValueError, match="CartPole-v1"):
        builder.build_loop(cfg, 1, 1, 1, False, 1)
