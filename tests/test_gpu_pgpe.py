"""The pgpe strategy on the device against its numpy restatement (tests/pgpe_np.py) and float64.

  * ses_perturb_mirrored: bit-equal to the restatement, any row range the matching slice of the whole population;
  * ses_pgpe_generation: Gmu / Gs within pgpe_tolerance of float64 parameter by parameter (tests/test_pgpe_host.py shows the
    bound catches one wrong pair), (mu, m, v) bit-equal to AdamNP fed the device Gmu, scale bit-equal to the restatement fed the
    device Gs -- with the +-20 % clip and both limits binding --, best = max(fitness), theta_next bit-equal to the restatement's
    population of the new state, a shard call the same state and the matching slice;
  * the update folded into the perturbation launch (P <= 1024) and as a launch of its own: bit-equal;
  * one handle over changing n, openai_es generations in between: the scratch it assumes cleared is cleared;
  * ses_run_generations with SES_STRATEGY_PGPE bit-equal to per-generation ESLoop.generation calls;
  * conf/cartpole_pgpe.yaml end to end: learns, adapts its scales, restores from a snapshot bit for bit.
Shapes: the smallest population; under one thread round with a ragged tail and P no multiple of 4; exactly one chunk of pairs; a
second chunk of one pair with P > 1024; past the 8192-row switch of the rank path.
"""
import contextlib
import io
import os

import numpy as np
import pytest
import torch
import yaml

import pgpe_np as pg
from oracle import strategies_np as snp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
LR, SIGMA, SEED, DECAY = 0.05, 0.1, 20240611, 0.999
SHAPES = {226: (4, 2, True, False), 6562: (4, 2, True, True), 581: (12, 5, True, False)}
CASES = [(4, 226), (260, 226), (2048, 581), (2050, 6562), (8196, 226)]
IDS = [f"n{n}-P{P}" for n, P in CASES]
WORST = {}


@pytest.fixture(scope="module")
def handles():
    from ses import HipES
    made = {}

    def get(P, key=None):
        if (P, key) not in made:
            S, A, disc, gru = SHAPES[P]
            made[(P, key)] = HipES(None, S, A, disc, gru)
            assert made[(P, key)].P == P
        return made[(P, key)]

    yield get
    for h in made.values():
        h.close()
    if WORST:
        print("\nworst |G - G64| / tol per (n, P): Gmu, Gs")
        for (n, P), (a, b) in sorted(WORST.items()):
            print(f"  n={n:>5} P={P:>4}: {a:.4f} {b:.4f}")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_bit_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = bits(got) != bits(want)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} differ, first at {np.argwhere(bad)[0]}: " \
                          f"{got[tuple(np.argwhere(bad)[0])]!r} vs {want[tuple(np.argwhere(bad)[0])]!r}"


def fitness(kind, n, rng):
    """the generators of tests/test_gpu_es_tail_f64.py: tie-free, and CartPole-like (small integers and saturated returns)"""
    if kind == "perm":
        return rng.permutation(n).astype(np.float32) * 0.25 - 7.0
    fit = rng.randint(0, 60, n).astype(np.float32)
    sat = rng.rand(n) < 0.5
    fit[sat] = rng.choice(np.array([500.0, 137.2, 10.0, 9.8], np.float32), int(sat.sum()))
    return fit


def random_state(P, rng):
    """(mu, m, v, scale), the Adam step t >= 2 they are the state after, and adam_a of step t + 1.  scale: random in [0.01, 100]
    (log-uniform), every tenth parameter just inside the lower / the upper limit so that the limits can bind."""
    mu = (rng.randn(P) * 0.3).astype(np.float32)
    m = (rng.randn(P) * 1e-3).astype(np.float32)
    v = (rng.rand(P) * 1e-5).astype(np.float32)
    scale = np.exp(rng.uniform(np.log(0.01), np.log(100.0), P)).astype(np.float32)
    scale[3::10] = np.float32(0.0101)
    scale[7::10] = np.float32(99.5)
    t = int(rng.randint(2, 40))
    adam = snp.AdamNP(mu.copy(), LR)
    adam.t = t + 1
    return (mu, m, v, scale), t, adam.step_scale()


def generation(es, fit, gen, state, a, first_row, n_rows, slr=0.2, smc=0.2, limits=(0.01, 100.0), fold=1):
    """ses_pgpe_generation from copies of `state`.  fold: the knob "pgpe_fused_apply_perturb" -- 1 (the default): policies up to
    1024 parameters apply the update inside the launch that draws the next population; 0: always a launch of its own."""
    out = tuple(es.zeros(es.P) for _ in range(4))
    best = es.zeros(1)
    es.set_tuning("pgpe_fused_apply_perturb", fold)
    try:
        theta, gmu, gs = es.pgpe_generation(dev(fit), SEED, gen, SIGMA, a, slr, smc, limits, tuple(dev(x) for x in state), out,
                                            np.float32(SIGMA * DECAY), gen + 1, first_row, n_rows, best=best, want_sums=True)
        es.sync()
    finally:
        es.set_tuning("pgpe_fused_apply_perturb", 1)
    return tuple(host(x) for x in out), host(theta), host(best)[0], host(gmu), host(gs)


def check_sums(gmu, gs, ref, n, P, what):
    g64mu, g64s, tol_mu, tol_s = ref
    worst = []
    for name, got, want, tol in (("Gmu", gmu, g64mu, tol_mu), ("Gs", gs, g64s, tol_s)):
        ratio = np.abs(got.astype(np.float64) - want) / tol
        worst.append(float(ratio.max()))
        print(f"{what}: n={n} P={P} {name} worst |err|/tol = {ratio.max():.4f} (median {np.median(ratio):.4f})")
        bad = ~(ratio <= 1.0)
        assert not bad.any(), f"{what}: {name}: {bad.sum()} of {P} parameters outside the float64 bound, worst p={int(ratio.argmax())} " \
                              f"ratio {ratio.max():.3f}: {got[ratio.argmax()]!r} vs {want[ratio.argmax()]!r} +- {tol[ratio.argmax()]!r}"
    old = WORST.get((n, P), (0.0, 0.0))
    WORST[(n, P)] = (max(old[0], worst[0]), max(old[1], worst[1]))


def check_state(out, state, t, gmu, gs, n, what, **kw):
    want = pg.update(*state[:3], t, state[3], gmu, gs, SIGMA, LR, n, **kw)
    for name, got, wnt in zip(("mu", "m", "v", "scale"), out, want):
        assert_bit_equal(got, wnt, f"{what}: {name}")
    return want


@pytest.mark.parametrize("n,P", CASES, ids=IDS)
def test_perturb_mirrored_equals_restatement(handles, n, P):
    es = handles(P)
    rng = np.random.RandomState(n + P)
    (mu, _, _, scale), _, _ = random_state(P, rng)
    gen = 2 ** 32 + 5 if n == 260 else 9
    whole = pg.population(mu, scale, SIGMA, SEED, gen, 0, n)
    got = host(es.perturb_mirrored(dev(mu), dev(scale), SIGMA, SEED, gen, 0, n))
    assert_bit_equal(got, whole, "whole population")
    assert not np.array_equal(whole[0], whole[1])
    for first in (0, 1, n - 3):
        for rows in (1, 2, 3):
            got = host(es.perturb_mirrored(dev(mu), dev(scale), SIGMA, SEED, gen, first, rows))
            assert_bit_equal(got, whole[first:first + rows], f"rows [{first}, +{rows})")


@pytest.mark.parametrize("kind", ["perm", "cartpole"])
@pytest.mark.parametrize("n,P", CASES, ids=IDS)
def test_pgpe_generation_against_float64_and_restatement(handles, n, P, kind):
    es = handles(P)
    rng = np.random.RandomState((n * 31 + P + len(kind)) % (2 ** 31))
    fit = fitness(kind, n, rng)
    state, t, a = random_state(P, rng)
    gen = 11 + len(kind)
    ref = pg.pgpe_sums_f64(fit, SEED, gen, P)
    # the whole population, default constants
    out, theta, best, gmu, gs = generation(es, fit, gen, state, a, 0, n)
    check_sums(gmu, gs, ref, n, P, f"{kind}")
    new = check_state(out, state, t, gmu, gs, n, "whole")
    assert best == fit.max(), (best, fit.max())
    assert_bit_equal(theta, pg.population(new[0], new[3], np.float32(SIGMA * DECAY), SEED, gen + 1, 0, n), "theta_next")
    # the update as a launch of its own: bit-equal to the folded form
    out_u, theta_u, best_u, gmu_u, gs_u = generation(es, fit, gen, state, a, 0, n, fold=0)
    for name, x, y in zip(("mu", "m", "v", "scale", "Gmu", "Gs", "theta_next"), out_u + (gmu_u, gs_u, theta_u), out + (gmu, gs, theta)):
        assert_bit_equal(x, y, f"unfolded update: {name}")
    assert best_u == fit.max()
    # a shard that splits a pair at both ends: the same state, the matching slice; and no rows at all
    first = ((n // 2) | 1) if n > 4 else 1                                        # odd: the shard begins with the second row of a pair
    rows = min(n - first - 1, 301) & ~1 if n > 4 else 2              # even: ... and ends with the first row of one
    out2, theta2, best2, gmu2, gs2 = generation(es, fit, gen, state, a, first, rows)
    for name, x, y in zip(("mu", "m", "v", "scale", "Gmu", "Gs"), out2 + (gmu2, gs2), out + (gmu, gs)):
        assert_bit_equal(x, y, f"shard call: {name}")
    assert best2 == fit.max()
    assert_bit_equal(theta2, theta[first:first + rows], "shard call: theta_next")
    out3, theta3, best3, _, _ = generation(es, fit, gen, state, a, 0, 0)
    assert theta3.shape == (0, P) and best3 == fit.max()
    for name, x, y in zip(("mu", "m", "v", "scale"), out3, out):
        assert_bit_equal(x, y, f"no rows: {name}")
    # a large sigma_learning_rate: the +-20 % clip and each limit bind
    kw = dict(sigma_learning_rate=20.0, sigma_max_change=0.2, scale_limits=(0.01, 100.0))
    out4, _, _, gmu4, gs4 = generation(es, fit, gen, state, a, 0, 0, slr=20.0)
    assert_bit_equal(gs4, gs, "Gs does not depend on the step constants")
    new4 = check_state(out4, state, t, gmu4, gs4, n, "large step", **kw)
    sc, s4 = state[3], new4[3]
    if P * n >= 226 * 260:                                            # (with two pairs Gs can come out with one sign only)
        assert (s4 == sc * np.float32(1.2)).any() and (s4 == sc * np.float32(0.8)).any(), "the +-20 % clip never bound"
        assert (s4[3::10] == np.float32(0.01)).any() and (s4[7::10] == np.float32(100.0)).any(), "a limit never bound"
    free = (new[3] != sc * np.float32(1.2)) & (new[3] != sc * np.float32(0.8)) & (new[3] > 0.01) & (new[3] < 100.0)
    assert free.any(), "the default step was clipped everywhere"
    # other limits and another max change
    kw = dict(sigma_learning_rate=0.2, sigma_max_change=0.05, scale_limits=(0.5, 2.0))
    out5, _, _, gmu5, gs5 = generation(es, fit, gen, state, a, 0, 0, smc=0.05, limits=(0.5, 2.0))
    new5 = check_state(out5, state, t, gmu5, gs5, n, "narrow limits", **kw)
    assert new5[3].min() >= 0.5 and new5[3].max() <= 2.0


@pytest.mark.parametrize("P", [226, 6562])
def test_generation_sequence_on_one_handle(handles, P):
    """Generations of changing size on ONE handle, with openai_es generations in between that lay the handle's scratch out
    differently: every result against float64 and the restatement (a rank vector left uncleared would be counted twice)."""
    es = handles(P, "sequence")
    rng = np.random.RandomState(P)
    state, t, _ = random_state(P, rng)
    seq = [(4096, None), (4096, None), (260, None), (9000, None), (4096, 3000), (4096, 4096), (4, None), (8196, 9000), (8196, None)]
    if P > 1024:
        seq = [(2050, None), (2050, 2050), (260, None), (2050, 3000)]
    for k, (n, between) in enumerate(seq):
        gen = 100 + k
        fit = fitness(("perm", "cartpole")[k % 2], n, rng)
        adam = snp.AdamNP(state[0].copy(), LR)
        adam.t = t + 1
        a = adam.step_scale()
        if between is not None:
            junk = fitness("perm", between, rng)
            es.openai_generation(dev(junk), SEED, 1, LR, SIGMA, 1e-3, tuple(es.zeros(P) for _ in range(3)),
                                 tuple(es.zeros(P) for _ in range(3)), SIGMA, 2, 0, 1)
        first = (k * 997) % (n - 1) if k % 2 else 0
        rows = min(n - first, 64)
        out, theta, best, gmu, gs = generation(es, fit, gen, state, a, first, rows, fold=(k // 2) % 2)
        check_sums(gmu, gs, pg.pgpe_sums_f64(fit, SEED, gen, P), n, P, f"sequence step {k}")
        new = check_state(out, state, t, gmu, gs, n, f"sequence step {k} (n={n})")
        assert best == fit.max()
        assert_bit_equal(theta, pg.population(new[0], new[3], np.float32(SIGMA * DECAY), SEED, gen + 1, first, rows),
                         f"sequence step {k}: theta_next")
        state, t = out, t + 1


def test_front_end_rejects_bad_shapes(handles):
    from ses import SesError
    es = handles(226)
    ok = tuple(es.zeros(226) for _ in range(4))
    out = tuple(es.zeros(226) for _ in range(4))
    for n in (3, 2, 7):
        with pytest.raises(SesError):
            es.pgpe_generation(es.zeros(n), 0, 0, 0.1, 1e-3, 0.2, 0.2, (0.01, 100.0), ok, out, 0.1, 1, 0, 0)
    with pytest.raises(SesError):
        es.pgpe_generation(es.zeros(8), 0, 0, 0.1, 1e-3, 0.2, 0.2, (0.01, 100.0), ok, ok, 0.1, 1, 0, 0)
    with pytest.raises(SesError):
        es.pgpe_generation(es.zeros(8), 0, 0, 0.1, 1e-3, 0.2, 0.2, (0.01, 100.0), ok, out, 0.1, 1, 6, 3)
    with pytest.raises(SesError):
        es.perturb_mirrored(es.zeros(225), es.zeros(226), 0.1, 0, 0, 0, 4)


def small_cfg():
    return {"env": {"name": "CartPole-v1", "max_step": 50, "pomdp": False, "seed": 4},
            "network": {"name": "gym_model", "num_state": 4, "num_action": 2, "discrete_action": True, "gru": False},
            "strategy": {"name": "pgpe", "init_sigma": 0.3, "sigma_decay": 0.98, "learning_rate": 0.05, "offspring_num": 64, "seed": 2}}


def strategy_state(s):
    return {"mu": host(s.mu_model), "m": host(s.optimizer.m), "v": host(s.optimizer.v), "scale": host(s.scale)}


def test_run_generations_equals_per_generation_calls(tmp_path, monkeypatch):
    """ses_run_generations with SES_STRATEGY_PGPE, k = 3, against three ESLoop.generation calls: mu, m, v, scale, theta, best[k]."""
    import builder
    from learning_strategies.evolution.loop import _GenerationBatch
    monkeypatch.chdir(tmp_path)
    with contextlib.redirect_stdout(io.StringIO()):
        a = builder.build_loop(small_cfg(), 3, 1, 2, False, 10 ** 9)
        b = builder.build_loop(small_cfg(), 3, 1, 2, False, 10 ** 9)
    pop = a.offspring_strategy.init_offspring(a.network, a.env.get_agent_ids())
    want_best = []
    for _ in range(3):
        pop, best, _sigma, _stamp = a.generation(pop)
        want_best.append(best.result())
    torch.cuda.synchronize()
    pop_b = b.offspring_strategy.init_offspring(b.network, b.env.get_agent_ids())
    assert _GenerationBatch.eligible(b, b.offspring_strategy, pop_b)
    batch = _GenerationBatch(b, b.offspring_strategy, pop_b)
    best, _stamps, sigmas = batch.run(3)
    torch.cuda.synchronize()
    pop_b = batch.sync_back()
    assert [float(x) for x in best[:3]] == want_best and len(set(want_best)) > 1, (best[:3], want_best)
    sa, sb = a.offspring_strategy, b.offspring_strategy
    for k, v in strategy_state(sa).items():
        assert_bit_equal(strategy_state(sb)[k], v, f"run_generations: {k}")
    assert_bit_equal(host(pop_b.theta), host(pop.theta), "run_generations: theta")
    assert sb.curr_sigma == sa.curr_sigma == sigmas[-1] and sb.optimizer.t == sa.optimizer.t == 3 and pop_b.gen == pop.gen == 3
    assert np.abs(strategy_state(sb)["mu"]).max() > 0 and not np.all(strategy_state(sb)["scale"] == 1.0)
    # and the two forms continue from each other: one more per-generation call on the batched run's state
    pop, best_a, _, _ = a.generation(pop)
    pop_b, best_b, _, _ = b.generation(pop_b)
    assert best_a.result() == best_b.result()
    assert_bit_equal(host(pop_b.theta), host(pop.theta), "generation after run_generations: theta")


def test_cartpole_pgpe_config_end_to_end(tmp_path, monkeypatch):
    import builder
    monkeypatch.chdir(tmp_path)
    cfg = yaml.load(open(os.path.join(SRC, "conf", "cartpole_pgpe.yaml")), Loader=yaml.FullLoader)
    loop = builder.build_loop(cfg, 40, 1, 5, False, 10 ** 9)
    with contextlib.redirect_stdout(io.StringIO()):
        pop = loop.run()
    best = [b for b, _ in loop.history]
    print("best per generation:", best)
    assert len(best) == 40 and max(best[-10:]) == 500 and min(best[-10:]) >= 400, best
    assert loop.batched_generations == 40                             # the run went through ses_run_generations
    s = loop.offspring_strategy
    scale = host(s.scale)
    print("scale range:", float(scale.min()), float(scale.max()))
    assert not np.all(scale == 1.0) and scale.min() >= 0.01 and scale.max() <= 100.0
    assert s.curr_sigma == 0.1 and all(sig == 0.1 for _, sig in loop.history)
    assert_bit_equal(s.get_elite_model().flat().astype(np.float32), host(s.mu_model), "get_elite_model")
    # snapshot -> two generations -> restore -> the same two generations
    snap = s.snapshot(pop)
    runs = []
    for _ in range(2):
        p, got = pop, []
        for _ in range(2):
            p, b, sigma, _ = loop.generation(p)
            got.append((b.result(), sigma, host(p.theta), strategy_state(s)))
        runs.append(got)
        pop = s.restore(snap)
    for (b0, g0, th0, st0), (b1, g1, th1, st1) in zip(*runs):
        assert b0 == b1 and g0 == g1
        assert_bit_equal(th1, th0, "after restore: theta")
        for k in st0:
            assert_bit_equal(st1[k], st0[k], f"after restore: {k}")
    assert not np.array_equal(runs[0][0][2], runs[0][1][2])
