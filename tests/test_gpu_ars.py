"""The ars strategy on the device against its numpy restatement (tests/ars_np.py) and float64.

  * the population from mu: bit-equal to the restatement and to ses_perturb_mirrored with a scale of ones;
  * ses_ars_generation: sigma_R bit-equal to the restatement (double), G within ars_tolerance of float64 parameter by parameter
    (tests/test_ars_host.py shows the bound catches one wrong pair), mu_out bit-equal to the restatement fed the device's G,
    best = max(fitness), theta_next bit-equal to the restatement's population of the new state, a shard call the same state and
    the matching slice, two shards the whole; equal returns leave mu alone;
  * the update folded into the perturbation launch (P <= 1024) and as a launch of its own: bit-equal;
  * one handle over changing (n, b), openai_es and pgpe generations in between: every step bit-equal to a fresh handle;
  * ses_run_generations with SES_STRATEGY_ARS bit-equal to per-generation ESLoop.generation calls;
  * conf/cartpole_ars.yaml end to end: learns, restores from a snapshot bit for bit.
Shapes (n, P, b): the smallest; under one thread round, ragged, P no multiple of 4; b = m; exactly one chunk of selected pairs; a
second chunk of one pair with P > 1024 (the unfused apply); 8194 pair scores, past the 8192 switch of the rank path.
"""
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest
import torch
import yaml

import ars_np as an

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
LR, SIGMA, SEED, DECAY = 0.2, 0.1, 20240611, 0.999
SHAPES = {226: (4, 2, True, False), 6562: (4, 2, True, True), 581: (12, 5, True, False)}
CASES = [(4, 226, 1), (260, 226, 37), (260, 226, 130), (2048, 581, 1024), (2050, 6562, 1025), (16388, 226, 100)]
IDS = [f"n{n}-P{P}-b{b}" for n, P, b in CASES]
INVALID_ARG = -1                                                      # SES_ERR_INVALID_ARG of include/ses.h
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
        print("\nworst |G - G64| / tol per (n, P, b)")
        for key, a in sorted(WORST.items()):
            print(f"  n={key[0]:>5} P={key[1]:>4} b={key[2]:>4}: {a:.4f}")


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
    """the generators of tests/test_gpu_pgpe.py -- tie-free, and CartPole-like (small integers and saturated returns: ties across
    the selection boundary) -- and a population in which every return is the same"""
    if kind == "flat":
        return np.full(n, 500.0, np.float32)
    if kind == "perm":
        return rng.permutation(n).astype(np.float32) * 0.25 - 7.0
    fit = rng.randint(0, 60, n).astype(np.float32)
    sat = rng.rand(n) < 0.5
    fit[sat] = rng.choice(np.array([500.0, 137.2, 10.0, 9.8], np.float32), int(sat.sum()))
    return fit


def random_mu(P, rng):
    return (rng.randn(P) * 0.3).astype(np.float32)


def generation(es, fit, b, gen, mu, first_row, n_rows, fold=1, lr=LR):
    """ses_ars_generation from a copy of `mu`.  fold: the knob "ars_fused_apply_perturb" -- 1 (the default): policies up to 1024
    parameters apply the update inside the launch that draws the next population; 0: always a launch of its own.
    Returns (mu_out, theta_next, best, G, sigma_R)."""
    out = (es.zeros(es.P),)
    best = es.zeros(1)
    es.set_tuning("ars_fused_apply_perturb", fold)
    try:
        theta, g, sr = es.ars_generation(dev(fit), b, SEED, gen, SIGMA, lr, (dev(mu),), out, np.float32(SIGMA * DECAY), gen + 1,
                                         first_row, n_rows, best=best, want_sums=True)
        es.sync()
    finally:
        es.set_tuning("ars_fused_apply_perturb", 1)
    return host(out[0]), host(theta), host(best)[0], host(g), float(host(sr)[0])


def check_sum(g, g64, tol, key, what):
    err = np.abs(g.astype(np.float64) - g64)
    ratio = np.divide(err, tol, out=np.zeros_like(err), where=tol > 0)
    print(f"{what}: n={key[0]} P={key[1]} b={key[2]} G worst |err|/tol = {ratio.max():.4f} (median {np.median(ratio):.4f})")
    bad = ~(err <= tol)
    assert not bad.any(), f"{what}: G: {bad.sum()} of {len(g)} parameters outside the float64 bound, worst p={int(ratio.argmax())} " \
                          f"ratio {ratio.max():.3f}: {g[ratio.argmax()]!r} vs {g64[ratio.argmax()]!r} +- {tol[ratio.argmax()]!r}"
    WORST[key] = max(WORST.get(key, 0.0), float(ratio.max()))


@pytest.mark.parametrize("n,P,b", CASES, ids=IDS)
def test_population_equals_restatement_and_mirrored_with_ones(handles, n, P, b):
    es = handles(P)
    rng = np.random.RandomState(n + P)
    mu = random_mu(P, rng)
    gen = 2 ** 32 + 5 if n == 260 else 9
    whole = an.population(mu, SIGMA, SEED, gen, 0, n)
    ones = dev(np.ones(P, np.float32))
    got = host(es.perturb_mirrored(dev(mu), ones, SIGMA, SEED, gen, 0, n))
    assert_bit_equal(got, whole, "ses_perturb_mirrored with ones: whole population")
    # the generation's own perturbation kernel, from a flat fitness (mu_out = mu): the population of (mu, gen)
    mu_out, theta, _, _, _ = generation(es, fitness("flat", n, rng), b, gen - 1, mu, 0, n)
    assert_bit_equal(mu_out, mu, "flat: mu_out")
    assert_bit_equal(theta, an.population(mu, np.float32(SIGMA * DECAY), SEED, gen, 0, n), "the tail's population of (mu, gen)")
    assert_bit_equal(theta, host(es.perturb_mirrored(dev(mu), ones, np.float32(SIGMA * DECAY), SEED, gen, 0, n)),
                     "the tail's population against ses_perturb_mirrored with ones")
    assert not np.array_equal(whole[0], whole[1])


@pytest.mark.parametrize("kind", ["perm", "cartpole", "flat"])
@pytest.mark.parametrize("n,P,b", CASES, ids=IDS)
def test_ars_generation_against_float64_and_restatement(handles, n, P, b, kind):
    es = handles(P)
    rng = np.random.RandomState((n * 31 + P + b + len(kind)) % (2 ** 31))
    fit = fitness(kind, n, rng)
    mu = random_mu(P, rng)
    gen = 11 + len(kind)
    sel, sr_want, g64, tol = an.ars_reference(fit, b, SEED, gen, P)
    if kind == "cartpole" and 1 < b < n // 2:
        scores = an.pair_scores(fit)
        assert scores[sel[-1]] == np.sort(scores)[::-1][b], "no tie across the selection boundary"
    # the whole population
    mu_out, theta, best, g, sr = generation(es, fit, b, gen, mu, 0, n)
    assert sr == sr_want, (sr, sr_want)
    check_sum(g, g64, tol, (n, P, b), kind)
    want = an.update(mu, g, sr, LR, b)
    assert_bit_equal(mu_out, want, "mu_out")
    assert best == fit.max(), (best, fit.max())
    assert_bit_equal(theta, an.population(want, np.float32(SIGMA * DECAY), SEED, gen + 1, 0, n), "theta_next")
    assert np.all(np.isfinite(mu_out)) and np.all(np.isfinite(theta)) and np.all(np.isfinite(g)) and np.isfinite(sr)
    if kind == "flat":
        assert sr == 0.0 and np.all(g == 0.0)
        assert_bit_equal(mu_out, mu, "flat: mu_out against mu_in")
    else:
        assert sr > 0.0 and not np.array_equal(mu_out, mu)
    # the update as a launch of its own: bit-equal to the folded form
    if P <= 1024:
        mu_u, theta_u, best_u, g_u, sr_u = generation(es, fit, b, gen, mu, 0, n, fold=0)
        for name, x, y in zip(("mu", "G", "theta_next"), (mu_u, g_u, theta_u), (mu_out, g, theta)):
            assert_bit_equal(x, y, f"unfolded update: {name}")
        assert best_u == fit.max() and sr_u == sr
    # a shard that splits a pair at both ends: the same state, the matching slice; the two shards around it; no rows at all
    first = ((n // 2) | 1) if n > 4 else 1                            # odd: the shard begins with the second row of a pair
    rows = min(n - first - 1, 301) & ~1 if n > 4 else 2              # even: ... and ends with the first row of one
    mu2, theta2, best2, g2, sr2 = generation(es, fit, b, gen, mu, first, rows)
    assert_bit_equal(mu2, mu_out, "shard call: mu")
    assert_bit_equal(g2, g, "shard call: G")
    assert best2 == fit.max() and sr2 == sr
    assert_bit_equal(theta2, theta[first:first + rows], "shard call: theta_next")
    _, theta_a, _, _, _ = generation(es, fit, b, gen, mu, 0, first)
    _, theta_b, _, _, _ = generation(es, fit, b, gen, mu, first, n - first)
    assert_bit_equal(np.concatenate([theta_a, theta_b]), theta, "two shards concatenated")
    mu3, theta3, best3, _, sr3 = generation(es, fit, b, gen, mu, 0, 0)
    assert theta3.shape == (0, P) and best3 == fit.max() and sr3 == sr
    assert_bit_equal(mu3, mu_out, "no rows: mu")


def other_tail(es, kind, n, rng):
    """an openai_es or a pgpe generation of n rows on the handle: it lays the scratch out its own way"""
    P = es.P
    junk = dev(fitness("perm", n, rng))
    if kind == "openai_es":
        es.openai_generation(junk, SEED, 1, 0.05, SIGMA, 1e-3, tuple(es.zeros(P) for _ in range(3)),
                             tuple(es.zeros(P) for _ in range(3)), SIGMA, 2, 0, 1)
    else:
        ones = tuple(dev(np.ones(P, np.float32)) if i == 3 else es.zeros(P) for i in range(4))
        es.pgpe_generation(junk, SEED, 1, SIGMA, 1e-3, 0.2, 0.2, (0.01, 100.0), ones, tuple(es.zeros(P) for _ in range(4)),
                           SIGMA, 2, 0, 2)


@pytest.mark.parametrize("P", [226, 6562])
def test_generation_sequence_on_one_handle(handles, P):
    """Generations of changing (n, b) on ONE handle, with openai_es and pgpe generations in between that lay the handle's scratch
    out differently (among them pgpe populations of exactly m rows, whose rank vector lies where this tail's does): every step
    bit-equal to the same step on a handle that runs this tail alone, and to the restatement."""
    shared, fresh = handles(P, "sequence"), handles(P, "fresh")
    rng = np.random.RandomState(P)
    mu = random_mu(P, rng)
    seq = [(4096, 1024, None), (4096, 300, ("pgpe", 2048)), (260, 37, None), (18000, 100, ("openai_es", 9000)),
           (4096, 2048, ("openai_es", 3000)), (4096, 5, ("pgpe", 4096)), (4, 1, None), (16388, 8194, ("pgpe", 8194)), (16388, 100, None)]
    if P > 1024:
        seq = [(2050, 1025, None), (2050, 7, ("pgpe", 1026)), (260, 130, None), (2050, 1024, ("openai_es", 3000))]
    for k, (n, b, between) in enumerate(seq):
        gen = 100 + k
        fit = fitness(("perm", "cartpole")[k % 2], n, rng)
        if between is not None:
            other_tail(shared, between[0], between[1], rng)
        first = (k * 997) % (n - 1) if k % 2 else 0
        rows = min(n - first, 64)
        got = generation(shared, fit, b, gen, mu, first, rows, fold=(k // 2) % 2)
        want = generation(fresh, fit, b, gen, mu, first, rows, fold=(k // 2) % 2)
        for name, x, y in zip(("mu", "theta_next"), got[:2], want[:2]):
            assert_bit_equal(x, y, f"sequence step {k} (n={n}, b={b}): {name}")
        assert_bit_equal(got[3], want[3], f"sequence step {k}: G")
        assert got[2] == want[2] == fit.max() and got[4] == want[4]
        sel, sr_want, g64, tol = an.ars_reference(fit, b, SEED, gen, P)
        assert got[4] == sr_want
        check_sum(got[3], g64, tol, (n, P, b), f"sequence step {k}")
        new = an.update(mu, got[3], got[4], LR, b)
        assert_bit_equal(got[0], new, f"sequence step {k}: mu against the restatement")
        assert_bit_equal(got[1], an.population(new, np.float32(SIGMA * DECAY), SEED, gen + 1, first, rows), f"sequence step {k}: theta_next")
        mu = got[0]


def test_front_end_rejects_bad_shapes(handles):
    from ses import SesError
    es = handles(226)
    mu, out = (es.zeros(226),), (es.zeros(226),)
    for n in (3, 2, 7):                                               # odd, too small
        with pytest.raises(SesError):
            es.ars_generation(es.zeros(n), 1, 0, 0, 0.1, 0.2, mu, out, 0.1, 1, 0, 0)
    for b in (0, 5, -1):                                              # b = 0, b > m
        with pytest.raises(SesError):
            es.ars_generation(es.zeros(8), b, 0, 0, 0.1, 0.2, mu, out, 0.1, 1, 0, 0)
    with pytest.raises(SesError):
        es.ars_generation(es.zeros(8), 2, 0, 0, 0.1, 0.2, mu, mu, 0.1, 1, 0, 0)         # in and out the same buffer
    with pytest.raises(SesError):
        es.ars_generation(es.zeros(8), 2, 0, 0, 0.1, 0.2, mu, out, 0.1, 1, 6, 3)        # rows past the population
    # the C entry point itself, past the wrapper's checks: an error code each, nothing launched
    lib, h = es._lib, es._h
    fit, theta = es.zeros(8), es.empty(8, 226)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                      # noqa: E731

    def call(fitness_p, n, b, mu_in, mu_out, first_row, n_rows, theta_p):
        return lib.ses_ars_generation(h, fitness_p, n, b, 0, 0, 0.1, 0.2, mu_in, mu_out, 0.1, 1, first_row, n_rows, theta_p, None, None,
                                      None)

    assert call(p(fit), 8, 2, p(mu[0]), p(out[0]), 0, 8, p(theta)) == 0
    es.sync()
    bad = [(p(fit), 7, 2, p(mu[0]), p(out[0]), 0, 0, None), (p(fit), 8, 0, p(mu[0]), p(out[0]), 0, 0, None),
           (p(fit), 8, 5, p(mu[0]), p(out[0]), 0, 0, None), (None, 8, 2, p(mu[0]), p(out[0]), 0, 0, None),
           (p(fit), 8, 2, None, p(out[0]), 0, 0, None), (p(fit), 8, 2, p(mu[0]), None, 0, 0, None),
           (p(fit), 8, 2, p(mu[0]), p(out[0]), 0, 8, None), (p(fit), 8, 2, p(mu[0]), p(out[0]), 6, 3, p(theta)),
           (p(fit), 8, 2, p(mu[0]), p(mu[0]), 0, 0, None), (p(fit), 2, 1, p(mu[0]), p(out[0]), 0, 0, None)]
    for k, args in enumerate(bad):
        assert call(*args) == INVALID_ARG, (k, args[1], args[2], args[5], args[6])
    es.sync()


def small_cfg():
    return {"env": {"name": "CartPole-v1", "max_step": 50, "pomdp": False, "seed": 4},
            "network": {"name": "gym_model", "num_state": 4, "num_action": 2, "discrete_action": True, "gru": False},
            "strategy": {"name": "ars", "init_sigma": 0.3, "sigma_decay": 0.98, "learning_rate": 0.2, "offspring_num": 64,
                         "elite_num": 12, "seed": 2}}


def test_run_generations_equals_per_generation_calls(tmp_path, monkeypatch):
    """ses_run_generations with SES_STRATEGY_ARS, k = 3, against three ESLoop.generation calls: mu, theta, best[k]."""
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
    assert batch.st.ars_b == 12 and batch.st.elite_num == 0
    best, _stamps, sigmas = batch.run(3)
    torch.cuda.synchronize()
    pop_b = batch.sync_back()
    assert [float(x) for x in best[:3]] == want_best, (best[:3], want_best)
    sa, sb = a.offspring_strategy, b.offspring_strategy
    assert_bit_equal(host(sb.mu_model), host(sa.mu_model), "run_generations: mu")
    assert_bit_equal(host(pop_b.theta), host(pop.theta), "run_generations: theta")
    assert sb.curr_sigma == sa.curr_sigma == sigmas[-1] and pop_b.gen == pop.gen == 3
    assert np.abs(host(sb.mu_model)).max() > 0
    # and the two forms continue from each other: one more per-generation call on the batched run's state
    pop, best_a, _, _ = a.generation(pop)
    pop_b, best_b, _, _ = b.generation(pop_b)
    assert best_a.result() == best_b.result()
    assert_bit_equal(host(pop_b.theta), host(pop.theta), "generation after run_generations: theta")
    assert_bit_equal(host(sb.mu_model), host(sa.mu_model), "generation after run_generations: mu")


def test_cartpole_ars_config_end_to_end(tmp_path, monkeypatch):
    import builder
    from learning_strategies.evolution.offspring_strategies import ars
    from oracle import c_oracle as co
    monkeypatch.chdir(tmp_path)
    cfg = yaml.load(open(os.path.join(SRC, "conf", "cartpole_ars.yaml")), Loader=yaml.FullLoader)
    loop = builder.build_loop(cfg, 40, 1, 5, False, 10 ** 9)
    assert type(loop.offspring_strategy) is ars
    with contextlib.redirect_stdout(io.StringIO()):
        pop = loop.run()
    best = [b for b, _ in loop.history]
    print("best per generation:", best)
    assert len(best) == 40 and max(best[-10:]) == 500 and min(best[-10:]) >= 400, best
    assert loop.batched_generations == 40                             # the run went through ses_run_generations
    s = loop.offspring_strategy
    assert s.curr_sigma == 0.1 and all(sig == 0.1 for _, sig in loop.history)
    assert_bit_equal(s.get_elite_model().flat().astype(np.float32), host(s.mu_model), "get_elite_model")
    # the restatement on the C oracle's CartPole, same seeds: printed next to the run's (tests/test_gpu_pgpe.py asserts no such
    # equality for pgpe either: the device's float32 sum and its host emulation need not round alike; reported, not asserted)
    sc = cfg["strategy"]
    r = an.ArsNP(226, sc["init_sigma"], sc["sigma_decay"], sc["learning_rate"], 256, sc["elite_num"], seed=s.seed)
    rbest = []
    for gen in range(40):
        init = co.init_states_uniform(loop.seed_env, gen, 0, 256, 5, 4, False)
        fit, _, _ = co.rollout_cartpole(r.theta(), init, 5, 500)
        rbest.append(r.evaluate(fit))
    print("restatement, best per generation:", rbest, "equal:", rbest == best)
    # snapshot -> two generations -> restore -> the same two generations
    snap = s.snapshot(pop)
    runs = []
    for _ in range(2):
        p, got = pop, []
        for _ in range(2):
            p, b, sigma, _ = loop.generation(p)
            got.append((b.result(), sigma, host(p.theta), host(s.mu_model)))
        runs.append(got)
        pop = s.restore(snap)
    for (b0, g0, th0, mu0), (b1, g1, th1, mu1) in zip(*runs):
        assert b0 == b1 and g0 == g1
        assert_bit_equal(th1, th0, "after restore: theta")
        assert_bit_equal(mu1, mu0, "after restore: mu")
    assert not np.array_equal(runs[0][0][2], runs[0][1][2])
