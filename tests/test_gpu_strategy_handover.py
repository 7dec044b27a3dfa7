"""The hand-over between ses_run_generations (_GenerationBatch) and the per-generation path (ESLoop.generation) for the three
reference strategies, on one GPU:

  * both directions: batch -> sync_back -> generation() -> a new batch -> sync_back equals six generation() calls bit for bit
    (best rewards, theta, the strategy's state, sigma and the generation counters);
  * snapshot / restore on a strategy whose state came back from a batch replays the next generations bit for bit;
  * which strategies _GenerationBatch.eligible takes: the six classes, not a bare subclass, not fused=False, not with
    SES_BATCH_GENERATIONS=0.
Shape: CartPole MLP, 24 offspring (simple_genetic: 5 x 4 rows, simple_evolution: 25 rows), per-offspring resets.
"""
import contextlib
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REFERENCE = ["openai_es", "simple_evolution", "simple_genetic"]
EXTRA = {"pgpe": {"learning_rate": 0.05}, "sep_cma_es": {}, "lm_ma_es": {}}


def cfg(name):
    strat = {"name": name, "init_sigma": 0.6, "sigma_decay": 0.98, "learning_rate": 0.05, "elite_num": 5, "offspring_num": 24, "seed": 2}
    return {"env": {"name": "CartPole-v1", "max_step": 120, "pomdp": False, "seed": 4},
            "network": {"name": "gym_model", "num_state": 4, "num_action": 2, "discrete_action": True, "gru": False},
            "strategy": strat}


def build(name):
    import builder
    with contextlib.redirect_stdout(io.StringIO()):
        loop = builder.build_loop(cfg(name), 6, 1, 2, False, 10 ** 9)
    return loop, loop.offspring_strategy.init_offspring(loop.network, loop.env.get_agent_ids())


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def state(s):
    """the strategy's state as {name: uint32 bits or host scalar}"""
    if hasattr(s, "optimizer"):
        return {"mu": bits(s.mu_model), "m": bits(s.optimizer.m), "v": bits(s.optimizer.v), "t": s.optimizer.t}
    if hasattr(s, "elite_models"):
        return {"elite_models": bits(s.elite_models)}
    return {"mu": bits(s.mu_model), "elite0": bits(s.elite0), "alias": s._alias_state.cpu().numpy()}


def assert_same_state(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k)


def parent(s):
    return s.elite_models[0] if hasattr(s, "elite_models") else s.mu_model


def per_generation(loop, pop, k):
    bests = []
    for _ in range(k):
        pop, best, _sigma, _stamp = loop.generation(pop)
        bests.append(best.result())
    return pop, bests


def batched(loop, pop, k):
    from learning_strategies.evolution.loop import _GenerationBatch
    s = loop.offspring_strategy
    assert _GenerationBatch.eligible(loop, s, pop)
    batch = _GenerationBatch(loop, s, pop)
    best, _stamps, sigmas = batch.run(k)
    torch.cuda.synchronize()
    pop = batch.sync_back()
    assert s.curr_sigma == sigmas[-1]
    return pop, [float(x) for x in best[:k]]


def handed_over(name):
    """run B: three generations in a batch, one per-generation call, two in a new batch on the population that call returned"""
    loop, pop = build(name)
    pop, bests = batched(loop, pop, 3)
    pop, one = per_generation(loop, pop, 1)
    pop, two = batched(loop, pop, 2)
    return loop, pop, bests + one + two


@pytest.mark.parametrize("name", REFERENCE)
def test_hand_over_in_both_directions(tmp_path, monkeypatch, name):
    monkeypatch.chdir(tmp_path)
    a, pop_a = build(name)
    pop_a, bests_a = per_generation(a, pop_a, 6)
    torch.cuda.synchronize()
    b, pop_b, bests_b = handed_over(name)
    sa, sb = a.offspring_strategy, b.offspring_strategy
    print(name, "bests:", bests_a, bests_b)
    assert bests_a == bests_b and len(set(bests_a)) >= 2, (bests_a, bests_b)
    assert np.array_equal(bits(pop_b.theta), bits(pop_a.theta))
    assert_same_state(state(sb), state(sa), "hand-over")
    assert sb.curr_sigma == sa.curr_sigma and sb.gen == sa.gen == 7 and pop_b.gen == pop_a.gen == 6
    assert parent(sa).abs().max().item() > 0                                # the parent vector moved


@pytest.mark.parametrize("name", REFERENCE)
def test_snapshot_and_restore_after_a_hand_back(tmp_path, monkeypatch, name):
    monkeypatch.chdir(tmp_path)
    loop, pop, _ = handed_over(name)
    s = loop.offspring_strategy
    snap = s.snapshot(pop)
    runs = []
    for _ in range(2):
        p, got = pop, []
        for _ in range(2):
            p, b, sigma, _ = loop.generation(p)
            got.append((b.result(), sigma, bits(p.theta), state(s)))
        runs.append(got)
        pop = s.restore(snap)
    for (b0, g0, th0, st0), (b1, g1, th1, st1) in zip(*runs):
        assert b0 == b1 and g0 == g1
        assert np.array_equal(th1, th0)
        assert_same_state(st1, st0, "after restore")
    assert not np.array_equal(runs[0][0][2], runs[0][1][2])                 # the two generations differ


def test_eligibility(tmp_path, monkeypatch):
    from learning_strategies.evolution.loop import ESLoop, _GenerationBatch
    from learning_strategies.evolution.offspring_strategies import openai_es
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("SES_BATCH_GENERATIONS", raising=False)
    for name in REFERENCE + list(EXTRA):
        loop, pop = build(name)
        assert _GenerationBatch.eligible(loop, loop.offspring_strategy, pop), name
    loop, pop = build("openai_es")
    monkeypatch.setenv("SES_BATCH_GENERATIONS", "0")
    assert not _GenerationBatch.eligible(loop, loop.offspring_strategy, pop)
    monkeypatch.delenv("SES_BATCH_GENERATIONS")
    assert _GenerationBatch.eligible(loop, loop.offspring_strategy, pop)

    class my_es(openai_es):            # a user subclass may override evaluate: it stays on the per-generation path
        pass

    for strategy in (my_es(0.6, 0.98, 0.05, 24, seed=2), openai_es(0.6, 0.98, 0.05, 24, seed=2, fused=False)):
        with contextlib.redirect_stdout(io.StringIO()):
            other = ESLoop(cfg("openai_es"), strategy, loop.env, loop.network, 6, 1, 2, False, 10 ** 9)
        pop = strategy.init_offspring(other.network, other.env.get_agent_ids())
        assert not _GenerationBatch.eligible(other, strategy, pop), type(strategy).__name__
