"""A handle that ran ses_run_generations behaves like a fresh one in the per-generation entry points.

Inside one call the loop fuses across entry points: the rollout leaves the episode mean to the rank count of the tail, the tail
leaves its last launch (k_es_apply_perturb) to the next rollout's prologue, the call's last generation launches it.  None of
that may outlive the call -- neither a call that ran to its end nor one whose tail refused its arguments after the rollout of
that generation was enqueued.  Both cases run CartPole MLP, eval_ep_num = 8, n = 2049 (16 392 envs: the smallest population of
the pair kernel's range, so the deferred launch, the fused mean and the fused apply all act), 500 steps, fixed length, shared
init, openai_es; then one generation through the public wrappers (rollout, openai_generation) on the used handle A and on a
fresh handle B, from the same state and population, compared as bit patterns, with A's launch counters read around it.
"""
import numpy as np
import pytest

from test_gpu_fused_perturb_rollout import FIXED, LR, Run, assert_bit_equal, dev, host

pytestmark = pytest.mark.gpu

N, E = 2049, 8


def one_generation(es, start, init, gen, adam_t, sigma):
    """rollout + openai_generation through the public wrappers on handle `es`, from host copies of (theta, mu, m, v)"""
    theta, mu, m, v = (dev(start[name]) for name in ("theta", "mu", "m", "v"))
    out = [es.empty(es.P) for _ in range(3)]
    best = es.zeros(1)
    fitness = es.rollout(theta, dev(init), mode=FIXED)
    t = adam_t + 1
    adam_a = LR * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.99 ** t)
    theta_next = es.openai_generation(fitness, 11, gen, LR, sigma, adam_a, (mu.reshape(-1), m, v), out, sigma * 0.99, gen + 1, 0, N,
                                      best=best)
    es.sync()
    return {"fitness": host(fitness), "best": host(best), "mu": host(out[0]), "m": host(out[1]), "v": host(out[2]),
            "theta": host(theta_next)}


def assert_same_generation(a, b, what):
    for name in ("fitness", "best", "mu", "m", "v", "theta"):
        assert_bit_equal(a[name], b[name], f"{what}: {name}")
    assert len(np.unique(a["fitness"])) > 1, "the returns should not all tie"


def shared_init(es):
    lo, hi = es.init_range
    return np.random.RandomState(5).uniform(lo, hi, (E, es.init_dim)).astype(np.float32)


def test_reuse_after_a_call_that_fused():
    a, b = Run(N, E, 1), Run(N, E, 1)
    try:
        a.run(3)
        # two rollouts took the prologue form, the call's last generation launched k_es_apply_perturb: nothing ran unfused
        assert a.counts() == (3, 2, 1), a.counts()
        start, init = a.state(), shared_init(a.es)
        gen, adam_t, sigma = int(a.st.pop_gen), int(a.st.adam_t), float(a.st.sigma)
        got = one_generation(a.es, start, init, gen, adam_t, sigma)
        want = one_generation(b.es, start, init, gen, adam_t, sigma)
        assert_same_generation(got, want, "after run_generations(k = 3)")
        # one plain pair rollout, no prologue rollout, one k_es_apply_perturb -- on the used handle as on the fresh one
        assert a.counts() == (4, 2, 2), a.counts()
        assert b.counts() == (1, 0, 1), b.counts()
    finally:
        a.close()
        b.close()


def test_reuse_after_a_refused_call():
    from ses import SesError
    a, b = Run(N, E, 1), Run(N, E, 1)
    try:
        start, init = a.state(), shared_init(a.es)
        gen, adam_t = int(a.st.pop_gen), int(a.st.adam_t)
        a.st.sigma = 0.0                                   # the tail of generation 0 refuses it, behind that generation's rollout
        with pytest.raises(SesError, match="bad n / sigma"):
            a.run(2)
        a.es.sync()
        assert a.counts() == (1, 0, 0), a.counts()         # the rollout was enqueued (plain form), no update was launched
        got = one_generation(a.es, start, init, gen, adam_t, 0.05)
        want = one_generation(b.es, start, init, gen, adam_t, 0.05)
        assert_same_generation(got, want, "after a refused run_generations(k = 2)")
        assert a.counts() == (2, 0, 1), a.counts()
        assert b.counts() == (1, 0, 1), b.counts()
    finally:
        a.close()
        b.close()
