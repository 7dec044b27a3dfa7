"""ars without a GPU: the bound the device's sum is held to (tests/ars_np.py ars_tolerance) is worth holding it to, the numpy
restatement of the strategy selects, normalises and learns as include/ses.h says, and the builder knows the strategy.

  * a float32 emulation of the device's summation order (4-fma chain per thread, 8-level LDS tree, ordered chunk sum over the
    SELECTED pairs) stays inside the bound;
  * each mistake a kernel could make -- a selected pair replaced by an unselected one, an unselected pair added, the divisor
    2 b - 1 in sigma_R, a difference with the wrong sign -- moves the result past the bound on at least half of the parameters;
  * the population is pgpe's with scale = 1, bit for bit; the selection is a strict order under ties; equal returns leave mu alone.
"""
import functools
import os

import numpy as np
import pytest
import yaml

import ars_np as an
import pgpe_np as pg
from oracle import c_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
SEED, GEN = 1234, 17
SIZES = [(4100, 226, 2050), (260, 226, 37), (2048, 581, 1024), (2050, 226, 1025)]


@functools.lru_cache(maxsize=None)
def base(n, P, b):
    rng = np.random.RandomState(n + P + b)
    fit = rng.permutation(n).astype(np.float32) * 0.25 - 7.0
    sel_all = an.select(fit, n // 2)                                # every pair in rank order: sel_all[:b] is the selection
    sel = sel_all[:b]
    d64, d32 = an.differences(fit, sel)
    z = an.selected_noise(sel, SEED, GEN, P)
    g64, tol = an.ars_sum_f64(d64, z)
    return fit, sel_all, sel, d64, d32, z, g64, tol


def test_rounding_count():
    assert [an.ars_rounding_count(b) for b in (1, 37, 130, 1024, 1025, 2048, 2049, 100)] == [14, 14, 14, 14, 15, 15, 16, 14]


def test_reference_matches_its_parts():
    n, P, b = 260, 226, 37
    fit, sel_all, sel, d64, d32, z, g64, tol = base(n, P, b)
    sel_r, sr, g_r, tol_r = an.ars_reference(fit, b, SEED, GEN, P)
    assert np.array_equal(sel_r, sel) and np.array_equal(g_r, g64) and np.array_equal(tol_r, tol)
    zall = co.noise(SEED, GEN, 0, n // 2, P).astype(np.float64)
    np.testing.assert_allclose(g64, (fit[2 * sel].astype(np.float64) - fit[2 * sel + 1]) @ zall[sel], rtol=1e-12, atol=1e-13)
    kept = np.concatenate([fit[2 * sel], fit[2 * sel + 1]]).astype(np.float64)
    np.testing.assert_allclose(sr, kept.std(), rtol=1e-13)          # the population standard deviation, divisor 2 b
    K = an.ars_rounding_count(b)
    t_abs = np.abs(d64) @ np.abs(zall[sel])
    assert np.all(tol > K * 2.0 ** -24 * t_abs) and np.all(tol < 1.001 * K * 2.0 ** -24 * t_abs)


@pytest.mark.parametrize("n,P,b", SIZES)
def test_device_order_emulation_stays_inside_the_bound(n, P, b):
    fit, sel_all, sel, d64, d32, z, g64, tol = base(n, P, b)
    g = an.emulate_device_sum(d32, z)
    assert g.dtype == np.float32
    r = np.abs(g.astype(np.float64) - g64) / tol
    print(f"n={n} P={P} b={b}: emulated float32 device order, worst |err|/tol: {r.max():.4f}")
    assert r.max() <= 1.0
    assert r.max() > 1e-4                                            # the bound is not vacuous: the error it covers is real


MUTATIONS = ["wrong_selected_pair", "unselected_pair_added", "divisor_2b_minus_1", "flipped_sign"]


def mutated(kind, n, P, b):
    """the wrong float64 result next to the right one"""
    fit, sel_all, sel, d64, d32, z, g64, tol = base(n, P, b)
    k = int(np.argsort(np.abs(d64))[b // 2])                        # the selected pair with the median |difference|
    if kind == "flipped_sign":
        return g64 - 2.0 * d64[k] * z[k].astype(np.float64)
    if kind == "divisor_2b_minus_1":
        # the step is learning_rate / (b sigma_R): a wrong sigma_R scales the whole move, i.e. the sum the update is fed
        right, wrong = an.sigma_r(fit, sel), an.sigma_r(fit, sel, divisor=2 * b - 1)
        assert wrong != right and abs(wrong / right - np.sqrt(2.0 * b / (2.0 * b - 1.0))) < 1e-3
        return g64 * (right / wrong)
    # the best pair that was not selected (the worst selected one where every pair is: its noise row in place of another's)
    other = int(sel_all[b]) if b < n // 2 else int(sel_all[b - 1])
    d_other = float(fit[2 * other]) - float(fit[2 * other + 1])
    z_other = co.noise(SEED, GEN, other, 1, P)[0].astype(np.float64)
    if kind == "wrong_selected_pair":
        return g64 - d64[k] * z[k].astype(np.float64) + d_other * z_other
    if kind == "unselected_pair_added":
        return g64 + d_other * z_other
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", MUTATIONS)
@pytest.mark.parametrize("n,P,b", SIZES)
def test_bound_detects_mutation(n, P, b, kind):
    fit, sel_all, sel, d64, d32, z, g64, tol = base(n, P, b)
    wrong = mutated(kind, n, P, b)
    frac = float(np.mean(np.abs(wrong - g64) > tol))
    print(f"n={n} P={P} b={b} {kind}: |G_wrong - G64| > tol on {frac:.4f} of {P} parameters")
    assert frac >= 0.5


def test_population_slices_symmetry_and_pgpe_with_ones():
    rng = np.random.RandomState(3)
    P, n = 226, 10
    mu = rng.randn(P).astype(np.float32)
    whole = an.population(mu, 0.1, SEED, GEN, 0, n)
    assert whole.shape == (n, P) and whole.dtype == np.float32
    z = co.noise(SEED, GEN, 0, n // 2, P)
    assert np.array_equal(whole[4], mu + np.float32(0.1) * z[2]) and np.array_equal(whole[5], mu - np.float32(0.1) * z[2])
    assert not np.array_equal(whole[4], whole[5])
    ones = np.ones(P, np.float32)
    assert np.array_equal(whole.view(np.uint32), pg.population(mu, ones, 0.1, SEED, GEN, 0, n).view(np.uint32))
    for first in (0, 1, n - 3):
        for rows in (1, 2, 3):
            got = an.population(mu, 0.1, SEED, GEN, first, rows)
            assert np.array_equal(got, whole[first:first + rows])
            assert np.array_equal(got.view(np.uint32), pg.population(mu, ones, 0.1, SEED, GEN, first, rows).view(np.uint32))


def brute_rank(s):
    return np.array([sum(1 for i in range(len(s)) if s[i] > s[j] or (s[i] == s[j] and i > j)) for j in range(len(s))])


def test_selection_is_a_strict_order_under_ties():
    """half the scores equal, straddling rank b: the tied pairs enter the selection from the highest index down"""
    m, b = 40, 20
    rng = np.random.RandomState(5)
    scores = np.empty(m, np.float32)
    tied = rng.permutation(m)[: m // 2]
    rest = np.setdiff1d(np.arange(m), tied)
    scores[tied] = 100.0
    scores[rest[:10]] = 200.0 + np.arange(10)                       # 10 above the plateau: ranks 10 .. 29 are the tied pairs
    scores[rest[10:]] = np.arange(10)
    fit = np.empty(2 * m, np.float32)
    fit[0::2], fit[1::2] = scores, scores - rng.randint(0, 3, m)     # the other row of a pair is no better (and sometimes equal)
    assert np.array_equal(an.pair_scores(fit), scores)
    rank = an.rank_pairs(scores)
    assert np.array_equal(rank, brute_rank(scores)) and sorted(rank) == list(range(m))
    sel = an.select(fit, b)
    assert np.array_equal(rank[sel], np.arange(b))
    assert set(sel[:10]) == set(rest[:10])
    assert list(sel[10:]) == sorted(tied, reverse=True)[:10]        # ten of the twenty tied pairs: the highest indices, descending
    # all returns equal: rank = m - 1 - index
    assert np.array_equal(an.rank_pairs(np.full(7, 500.0, np.float32)), np.arange(7)[::-1])


def test_flat_returns_leave_mu_unchanged():
    """every kept return equal (CartPole at the 500 cap): sigma_R = 0, step = 0, mu' = mu bit for bit, nothing non-finite"""
    rng = np.random.RandomState(9)
    P, n, b = 226, 64, 16
    mu = rng.randn(P).astype(np.float32)
    fit = rng.randint(0, 400, n).astype(np.float32)
    fit[: 2 * 20] = 500.0                                            # 20 pairs at the cap: the 16 kept are all among them
    sel = an.select(fit, b)
    assert np.all(fit[2 * sel] == 500.0) and np.all(fit[2 * sel + 1] == 500.0)
    sr = an.sigma_r(fit, sel)
    assert sr == 0.0 and an.step_size(0.2, b, sr) == 0.0
    _, d32 = an.differences(fit, sel)
    G = an.emulate_device_sum(d32, an.selected_noise(sel, SEED, GEN, P))
    new = an.update(mu, G, sr, 0.2, b)
    assert np.all(G == 0.0) and np.all(np.isfinite(new)) and np.array_equal(new.view(np.uint32), mu.view(np.uint32))
    s = an.ArsNP(P, 0.1, 1.0, 0.2, n, b)
    s.mu = mu.copy()
    assert s.evaluate(np.full(n, 500.0, np.float32)) == 500.0 and s.last_sigma_r == 0.0
    assert np.array_equal(s.mu.view(np.uint32), mu.view(np.uint32))


def test_constructor_refusals_and_defaults():
    from learning_strategies.evolution.offspring_strategies import ars
    s = ars(0.1, 1.0, 0.2, 256)
    assert s.elite_num == 64 and s.offspring_num == 256 and s._gen_state_constants() == {"ars_b": 64}
    assert ars(0.1, 1.0, 0.2, 4).elite_num == 1 and ars(0.1, 1.0, 0.2, 6).elite_num == 1 and ars(0.1, 1.0, 0.2, 256, 128).elite_num == 128
    assert s.get_wandb_cfg() == dict(init_sigma=0.1, sigma_decay=1.0, learning_rate=0.2, offspring_num=256, elite_num=64)
    for bad_n in (255, 2, 3, 0):
        with pytest.raises(ValueError):
            ars(0.1, 1.0, 0.2, bad_n)
    for bad_b in (0, 129, -1, 1.5):
        with pytest.raises(ValueError):
            ars(0.1, 1.0, 0.2, 256, bad_b)
    with pytest.raises(ValueError):
        ars(0.1, 1.0, 0.2, 256, noise="numpy")
    assert [field for _, _, field in ars._STATE] == ["parents"] and ars._STRATEGY == "STRATEGY_ARS"


def test_builder_builds_ars_from_its_config():
    import builder
    from learning_strategies.evolution.offspring_strategies import ars
    cfg = yaml.load(open(os.path.join(SRC, "conf", "cartpole_ars.yaml")), Loader=yaml.FullLoader)
    s = builder.build_strategy(cfg["strategy"])
    assert type(s) is ars and s.offspring_num == 256 and s.curr_sigma == 0.1 and s.sigma_decay == 1.0
    assert s.learning_rate == 0.2 and s.elite_num == 64
    assert cfg["env"]["name"] == "CartPole-v1" and cfg["network"]["gru"] is False
    s2 = builder.build_strategy({**cfg["strategy"], "elite_num": 16, "seed": 7})
    assert s2.elite_num == 16 and s2.seed == 7
    for key, bad in (("offspring_num", 255), ("offspring_num", 2), ("elite_num", 0), ("elite_num", 129), ("noise", "numpy")):
        with pytest.raises(ValueError):
            builder.build_strategy({**cfg["strategy"], key: bad})
    # (builder.build_loop opens the device: tests/test_gpu_ars.py builds the loop from this file)
    for conf in ("pendulum_swingup_ars", "reacher_ars"):
        other = yaml.load(open(os.path.join(SRC, "conf", conf + ".yaml")), Loader=yaml.FullLoader)
        assert type(builder.build_strategy(other["strategy"])) is ars


def test_restatement_learns_cartpole_on_the_c_oracle():
    """256 offspring, 5 episodes, 40 generations, the config's constants: the best return of the last ten generations (the bar
    and the length of tests/test_pgpe_host.py's run)."""
    cfg = yaml.load(open(os.path.join(SRC, "conf", "cartpole_ars.yaml")), Loader=yaml.FullLoader)["strategy"]
    n, E, P = 256, 5, 226
    assert cfg["offspring_num"] == n
    s = an.ArsNP(P, cfg["init_sigma"], cfg["sigma_decay"], cfg["learning_rate"], n, cfg["elite_num"], seed=0)
    best = []
    for gen in range(40):
        init = co.init_states_uniform(0, gen, 0, n, E, 4, False)
        fit, _, _ = co.rollout_cartpole(s.theta(), init, E, 500)
        best.append(s.evaluate(fit))
    print("best per generation:", best)
    assert max(best[-10:]) == 500 and min(best[-10:]) >= 400, best
    assert np.all(np.isfinite(s.mu)) and np.abs(s.mu).max() > 0
