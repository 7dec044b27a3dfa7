"""The rows that the prologue form of the pair rollout kernel forms from registers (csrc/ses_perturb_prologue.h: one 16-byte
LDS read of the mean per quad, the four fmas back to back, 8-byte stores to LDS and to theta, no array indexed at run time).

Every case runs one ses_run_generations call of k generations with "fused_perturb_rollout" at 1 and compares it, on bit
patterns, with
  * the same call at knob 0 (k_es_apply_perturb between the generations, rows read from theta), and
  * the per-generation entry points on a third handle: ses_init_states_uniform, ses_rollout, ses_openai_generation, with the
    host scalars advanced as the C loop advances them,
on fitness, best, mu, m, v and theta[cur] after the call.  ses_launch_counts asserts that k - 1 rollouts of the call really ran
the prologue form.  theta[cur] after the call is the whole population of the new mean, at k = 1 (no prologue form runs at all)
and from k = 2 (the call's last generation writes it).

Shapes (fixed-length CartPole MLP, P = 226, 57 quads; the pair kernel runs 16 384 < n x E <= 20 480 envs; a workgroup owns 16
light envs and 64 heavy ones):
  * E = 2: 8 + 32 rows per workgroup = 2280 items, more than 3 x 512: the second batch loop of the prologue runs.
    n = 9001: 18 002 envs, 13 906 heavy = 217 workgroups + 18 envs: a ragged last heavy span, 38 workgroups with none.
  * E = 5: the 16 light envs of a workgroup start at env 16 b, so rows straddle two workgroups (row 3 = envs 15 .. 19) and both
    form them.  n = 3700: a ragged last heavy span; n = 4096: every workgroup full.
  * E = 8: 2 + 8 rows = 570 items, one item for most threads.  n = 2300: 18 400 envs, 14 304 heavy = 223 workgroups + 32 envs.
  * row 0 (the mean itself) is in the light span of workgroup 0 in every case.
Each shape also runs with "rollout_heavy_packed" = 0, the <true, false> instance of the kernel.
"""
import math

import numpy as np
import pytest

import test_gpu_fused_perturb_rollout as fpr

pytestmark = pytest.mark.gpu

dev, host = fpr.dev, fpr.host
SHAPES = [(9001, 2), (3700, 5), (4096, 5), (2300, 8)]
KS = (1, 2, 3, 5)


def stepwise(n, E, k, tuning):
    """k generations through the per-generation entry points, from the state fpr.Run starts in; the state in fpr.Run.state()'s form"""
    from ses import HipES
    es = HipES("CartPole-v1", 4, 2, True, False, max_step=fpr.T, eval_ep_num=E)
    try:
        for name, value in tuning:
            es.set_tuning(name, value)
        sigma = 0.05
        mu, theta, m, v, adam_t, gen = fpr.start_state("trained", n, es.P, sigma, np.random.RandomState(n + E))
        cur, theta = (dev(mu), dev(m), dev(v)), dev(theta)
        best, fit = [], None
        for _ in range(k):
            init = es.init_states_uniform(3, gen, 0, 1, shared=True)[0].contiguous()
            fit = es.rollout(theta, init, mode=fpr.FIXED)
            adam_t += 1
            a = fpr.LR * math.sqrt(1.0 - 0.999 ** adam_t) / (1.0 - 0.99 ** adam_t)      # optimizers.py:43-47, as the C loop forms it
            nxt_sigma = sigma * 0.99
            out = tuple(es.empty(es.P) for _ in range(3))
            b = es.zeros(1)
            theta = es.openai_generation(fit, 11, gen, fpr.LR, sigma, a, cur, out, np.float32(nxt_sigma), gen + 1, 0, n, best=b)
            es.sync()
            best.append(host(b)[0])
            cur, sigma, gen = out, nxt_sigma, gen + 1
        return {"theta": host(theta), "mu": host(cur[0])[None], "m": host(cur[1]), "v": host(cur[2]), "fitness": host(fit),
                "best": np.array(best, np.float32), "scalars": (sigma, sigma, gen, adam_t)}
    finally:
        es.close()


@pytest.mark.parametrize("heavy_packed", [-1, 0], ids=["heavy-packed", "heavy-scalar"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n,E", SHAPES, ids=[f"n{n}-E{E}" for n, E in SHAPES])
def test_rows_from_registers_equal_the_update_launch_and_the_stepwise_path(n, E, k, heavy_packed):
    tuning = (("rollout_heavy_packed", heavy_packed),)
    out = fpr.both_knobs(n, E, [k], tuning=tuning)                  # (asserts knob 1 == knob 0 on all six and the scalars)
    assert out[1][1] == (k, k - 1, 1), out[1][1]                    # the prologue form ran k - 1 times, one update launch per call
    assert out[0][1] == (k, 0, k), out[0][1]
    want = stepwise(n, E, k, tuning)
    got = out[1][0]
    for name in ("fitness", "best", "m", "v", "theta"):
        fpr.assert_bit_equal(got[name], want[name], f"n={n} E={E} k={k}: {name} vs the per-generation entry points")
    fpr.assert_bit_equal(got["mu"].reshape(-1), want["mu"].reshape(-1), f"n={n} E={E} k={k}: mu vs the per-generation entry points")
    assert got["scalars"] == want["scalars"], (got["scalars"], want["scalars"])
    assert len(np.unique(got["fitness"])) > 1, "the returns should not all tie"


@pytest.mark.parametrize("k", [1, 2])
def test_the_current_population_is_whole_after_a_call(k):
    """theta[cur] after k = 1 (no prologue form) and after k = 2 (one rollout in the prologue form) is the population of the new mean:
    row 0 the mean itself, every row what a second call then runs -- a call of one more generation on it equals k + 1 in one call"""
    a = fpr.Run(3700, 5, 1)
    b = fpr.Run(3700, 5, 1)
    try:
        a.run(k)
        s = a.state()
        fpr.assert_bit_equal(s["theta"][0], s["mu"].reshape(-1), f"k={k}: row 0 of theta[cur] vs the mean")
        a.run(1)
        b.run(k + 1)
        fpr.same(a.state(), b.state(), f"{k} + 1 vs {k + 1}")
        assert a.counts() == (k + 1, k - 1, 2) and b.counts() == (k + 1, k, 1), (a.counts(), b.counts())
    finally:
        a.close()
        b.close()
