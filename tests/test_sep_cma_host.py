"""sep_cma_es without a GPU: the constants, the bound the device's two sums are held to (tests/sep_cma_np.py sepcma_tolerance),
the numpy restatement of the strategy learning CartPole on the C oracle, and the builder.

  * the constants of (n, P) = (256, 226) against values computed by hand (pure-Python sums, no numpy);
  * a float32 emulation of the device's summation order (4-fma chain per thread with skipped rows, 8-level LDS tree, ordered
    chunk sum) stays inside the bound, and the error the bound covers is real;
  * one row given the wrong weight -- a selected row dropped or counted twice, an unselected row drawn, the two best rows swapped
    -- moves the float64 sum past the bound on at least half of the parameters.
"""
import functools
import math
import os

import numpy as np
import pytest
import yaml

import sep_cma_np as sc
from oracle import c_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
SEED, GEN = 1234, 17
SIZES = [(4100, 226), (260, 226), (1024, 581)]


def test_constants_against_hand_computed_values():
    """(n, P) = (256, 226), mu = 128.  The expected numbers: w_k from math.log in a Python loop, sums by math.fsum, then the
    formulas of the issue typed out once more with the numbers in."""
    c, w = sc.constants(256, 226)
    raw = [math.log(128.5) - math.log(k + 1) for k in range(128)]
    tot = math.fsum(raw)
    mueff = 1.0 / math.fsum((x / tot) ** 2 for x in raw)
    assert c["mu"] == 128 and w.shape == (128,) and w.dtype == np.float32
    assert c["mueff"] == pytest.approx(mueff, rel=1e-13) and c["mueff"] == pytest.approx(66.857796, rel=1e-6)
    assert c["c_sigma"] == pytest.approx((mueff + 2.0) / (226 + mueff + 5.0), rel=1e-13) and c["c_sigma"] == pytest.approx(0.23117674, rel=1e-6)
    assert c["d_sigma"] == pytest.approx(1.0 + c["c_sigma"], rel=1e-13)        # sqrt((mueff - 1) / 227) = 0.539 < 1: the max is 0
    assert math.sqrt((mueff - 1.0) / 227.0) < 1.0
    assert c["c_c"] == pytest.approx((4.0 + mueff / 226) / (230.0 + 2.0 * mueff / 226), rel=1e-13) and c["c_c"] == pytest.approx(0.018629602, rel=1e-6)
    assert c["c_1"] == pytest.approx(228.0 / 3.0 * 2.0 / (227.3 ** 2 + mueff), rel=1e-13) and c["c_1"] == pytest.approx(0.0029382117, rel=1e-6)
    cmu = 228.0 / 3.0 * 2.0 * (mueff - 2.0 + 1.0 / mueff) / (228.0 ** 2 + mueff)
    assert cmu < 1.0 - c["c_1"]
    assert c["c_mu"] == pytest.approx(cmu, rel=1e-13) and c["c_mu"] == pytest.approx(0.18944276, rel=1e-6)
    assert c["chi"] == pytest.approx(math.sqrt(226.0) * (1.0 - 1.0 / 904.0 + 1.0 / (21.0 * 226.0 ** 2)), rel=1e-14)
    assert c["chi"] == pytest.approx(15.016681, rel=1e-6)
    assert sc.hsig_scale(c, 1) == pytest.approx(1.0 / math.sqrt(1.0 - (1.0 - c["c_sigma"]) ** 2), rel=1e-15)
    assert sc.hsig_threshold(c, 226) == pytest.approx((1.4 + 2.0 / 227.0) * c["chi"], rel=1e-15)


def test_constants_where_the_min_and_the_max_bind():
    """(n, P, mu) = (512, 10, 256): few parameters, many selected rows -- the branches (256, 226) does not reach.  By hand:
    mueff = 131.6645; sqrt((mueff - 1) / 11) = 3.4465 > 1, so d_sigma = 1 + 2 * 2.4465 + c_sigma; c_mu's formula gives
    8 * 129.672 / 275.66 = 3.763 > 1 - c_1, so c_mu = 1 - c_1."""
    c, w = sc.constants(512, 10, 256)
    raw = [math.log(256.5) - math.log(k + 1) for k in range(256)]
    tot = math.fsum(raw)
    mueff = 1.0 / math.fsum((x / tot) ** 2 for x in raw)
    assert c["mueff"] == pytest.approx(mueff, rel=1e-13) and c["mueff"] == pytest.approx(131.66450, rel=1e-6)
    assert c["c_sigma"] == pytest.approx(133.66450 / 146.66450, rel=1e-6) and c["c_sigma"] == pytest.approx(0.91136233, rel=1e-6)
    root = math.sqrt((mueff - 1.0) / 11.0)
    assert root == pytest.approx(3.4465332, rel=1e-6)
    assert c["d_sigma"] == pytest.approx(1.0 + 2.0 * (root - 1.0) + c["c_sigma"], rel=1e-13) and c["d_sigma"] == pytest.approx(6.8044288, rel=1e-6)
    assert c["c_1"] == pytest.approx(4.0 * 2.0 / (11.3 ** 2 + mueff), rel=1e-13) and c["c_1"] == pytest.approx(0.030845811, rel=1e-6)
    assert 4.0 * 2.0 * (mueff - 2.0 + 1.0 / mueff) / (144.0 + mueff) == pytest.approx(3.7631860, rel=1e-6)
    assert c["c_mu"] == 1.0 - c["c_1"] and c["c_mu"] == pytest.approx(0.96915419, rel=1e-6)
    assert c["c_c"] == pytest.approx((4.0 + mueff / 10) / (14.0 + 2.0 * mueff / 10), rel=1e-13) and c["c_c"] == pytest.approx(0.42561904, rel=1e-6)
    assert c["chi"] == pytest.approx(math.sqrt(10.0) * (1.0 - 1.0 / 40.0 + 1.0 / 2100.0), rel=1e-14) and c["chi"] == pytest.approx(3.0847266, rel=1e-6)


@pytest.mark.parametrize("n,mu", [(256, None), (64, None), (4, None), (9, 1), (8, 8), (1025, 700)])
def test_weights_sum_to_one_and_decrease(n, mu):
    c, w = sc.constants(n, 226, mu)
    assert len(w) == (n // 2 if mu is None else mu) == c["mu"]
    assert abs(float(w.astype(np.float64).sum()) - 1.0) <= len(w) * 2.0 ** -25          # each entry rounded to float32 once
    assert np.all(w > 0) and np.all(np.diff(w) < 0)
    assert 1.0 <= c["mueff"] <= len(w) and 0 < c["c_sigma"] < 1 and 0 < c["c_c"] <= 1 and c["c_1"] + c["c_mu"] <= 1


@functools.lru_cache(maxsize=None)
def base(n, P):
    rng = np.random.RandomState(n + P)
    fit = rng.permutation(n).astype(np.float32)
    c, weights = sc.constants(n, P)
    w = sc.row_weights(fit, weights)
    cs = sc.chunk_sums_f64(w, SEED, GEN, P)
    tol_z = sc.sepcma_tolerance(n, "z", cs["Az"].sum(0))
    tol_zz = sc.sepcma_tolerance(n, "zz", cs["Szz"].sum(0))
    return fit, weights, w, cs, tol_z, tol_zz


def test_rounding_count():
    assert [sc.rounding_count(n, "z") for n in (4, 260, 1024, 1025, 4100, 8196)] == [13, 13, 13, 14, 17, 21]
    assert sc.rounding_count(4100, "zz") == 18 and sc.rounding_count(260, "zz") == 14


def test_row_weights_follow_the_tie_rule():
    weights = sc.constants(8, 226)[1]                                   # mu = 4
    fit = np.array([1, 5, 5, 0, 5, 2, 2, 9], np.float32)
    w = sc.row_weights(fit, weights)                                    # order: 7, then the 5s by index descending 4, 2, 1
    assert np.array_equal(w, np.array([0, weights[3], weights[2], 0, weights[1], 0, 0, weights[0]], np.float64))


def test_sums_f64_match_their_parts():
    n, P = 260, 226
    fit, weights, w, cs, tol_z, tol_zz = base(n, P)
    z = co.noise(SEED, GEN, 0, n, P).astype(np.float64)
    sz, szz, t_z, t_zz = sc.sums_f64(fit, weights, SEED, GEN, P)
    np.testing.assert_allclose(sz, w @ z, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(szz, w @ (z * z), rtol=1e-12, atol=1e-14)
    assert np.array_equal(t_z, tol_z) and np.array_equal(t_zz, tol_zz)
    assert (w > 0).sum() == n // 2 and w.sum() == pytest.approx(1.0, abs=1e-6)


@pytest.mark.parametrize("n,P", SIZES)
def test_device_order_emulation_stays_inside_the_bound(n, P):
    fit, weights, w, cs, tol_z, tol_zz = base(n, P)
    sz, szz = sc.emulate_device_sums(w, SEED, GEN, P)
    r_z = np.abs(sz.astype(np.float64) - cs["Sz"].sum(0)) / tol_z
    r_zz = np.abs(szz.astype(np.float64) - cs["Szz"].sum(0)) / tol_zz
    print(f"n={n} P={P}: emulated float32 device order, worst |err|/tol: Sz {r_z.max():.4f}, Szz {r_zz.max():.4f}")
    assert r_z.max() <= 1.0 and r_zz.max() <= 1.0
    assert r_z.max() > 1e-4 and r_zz.max() > 1e-4                    # the bound is not vacuous: the error it covers is real


# (The last selected rows are left alone: w_k falls to ln(1 + 1 / (2 mu)) / sum at k = mu - 1, 1.2e-7 at mu = 2050 against a
#  rounding bound of 8e-7 there -- a term smaller than the rounding of the others cannot be told from it, by any bound.)
MUTATIONS = ["best_row_dropped", "median_selected_dropped", "unselected_drawn_as_median", "top_two_swapped", "median_selected_twice"]


def mutated_weights(kind, fit, weights, w):
    rank = sc.snp.stable_rank(fit)
    mu = len(weights)
    row = {r: int(np.argmax(rank == r)) for r in (0, 1, mu // 2, mu - 1, mu)}
    v = w.copy()
    if kind == "best_row_dropped":
        v[row[0]] = 0.0
    elif kind == "median_selected_dropped":
        v[row[mu // 2]] = 0.0
    elif kind == "unselected_drawn_as_median":                      # the first row past the selection, with the median weight
        v[row[mu]] = float(weights[mu // 2])
    elif kind == "top_two_swapped":
        v[row[0]], v[row[1]] = w[row[1]], w[row[0]]
    elif kind == "median_selected_twice":
        v[row[mu // 2]] *= 2.0
    else:
        raise AssertionError(kind)
    assert (v != w).sum() in (1, 2)
    return v


@pytest.mark.parametrize("kind", MUTATIONS)
@pytest.mark.parametrize("n,P", SIZES)
def test_bound_detects_one_wrong_weight(n, P, kind):
    fit, weights, w, cs, tol_z, tol_zz = base(n, P)
    wrong = sc.chunk_sums_f64(mutated_weights(kind, fit, weights, w), SEED, GEN, P)
    for name, key, tol in (("Sz", "Sz", tol_z), ("Szz", "Szz", tol_zz)):
        frac = float(np.mean(np.abs(wrong[key].sum(0) - cs[key].sum(0)) > tol))
        print(f"n={n} P={P} {kind}: |{name}_wrong - {name}64| > tol on {frac:.4f} of {P} parameters")
        assert frac >= 0.5


def test_population_is_the_stated_arithmetic_and_slices():
    rng = np.random.RandomState(3)
    P, n = 226, 9
    mu = rng.randn(P).astype(np.float32)
    C = np.exp(rng.uniform(np.log(1e-4), np.log(1e4), P)).astype(np.float32)
    step = np.float32(1.7)
    whole = sc.population(mu, C, step, 0.5, SEED, GEN, 0, n)
    assert whole.shape == (n, P) and whole.dtype == np.float32
    z = co.noise(SEED, GEN, 0, n, P)
    want4 = mu + ((np.float32(0.5) * step) * np.sqrt(C)) * z[4]
    assert want4.dtype == np.float32 and np.array_equal(whole[4], want4)
    for first in (0, 1, n - 3):
        for rows in (1, 2, 3):
            assert np.array_equal(sc.population(mu, C, step, 0.5, SEED, GEN, first, rows), whole[first:first + rows])


def test_norm2_order_and_scalar_path():
    rng = np.random.RandomState(5)
    for P in (226, 1024, 2049):
        ps = rng.randn(P).astype(np.float32)
        got = sc.norm2_device_order(ps)
        assert got == pytest.approx(float((ps.astype(np.float64) ** 2).sum()), rel=1e-14)
    c, _ = sc.constants(256, 226)
    # a path of the expected length leaves the step where it is (to a rounding); a long one raises it, capped at e
    h, s1, info = sc.scalar_path(c["chi"] ** 2, 1.0, c, 226, sc.hsig_scale(c, 50))
    assert h and abs(float(s1) - 1.0) < 1e-6 and not info["capped"]
    h, s2, info = sc.scalar_path((100.0 * c["chi"]) ** 2, 2.0, c, 226, sc.hsig_scale(c, 50))
    assert not h and info["capped"] and s2 == np.float32(2.0 * math.e)
    h, s3, info = sc.scalar_path(0.0, 1.0, c, 226, sc.hsig_scale(c, 1))
    assert h and s3 == np.float32(math.exp(-c["c_sigma"] / c["d_sigma"]))
    _, s4, _ = sc.scalar_path((100.0 * c["chi"]) ** 2, 2.0, c, 226, 1.0, step_limits=(0.5, 3.0))
    _, s5, _ = sc.scalar_path(0.0, 1.0, c, 226, 1.0, step_limits=(0.9, 3.0))
    assert s4 == np.float32(3.0) and s5 == np.float32(0.9)


def test_update_clamps_the_variance_and_switches_on_h():
    P = 226
    c, _ = sc.constants(256, P)
    one, zero = np.ones(P, np.float32), np.zeros(P, np.float32)
    Sz = np.full(P, 0.05, np.float32)
    Szz = one.copy()
    Szz[0], Szz[1] = 1e6, 0.0
    C = one.copy()
    C[1] = np.float32(1.0001e-4)
    for norm2, want_h in ((c["chi"] ** 2, True), ((10 * c["chi"]) ** 2, False)):
        new, h, info = sc.update(zero, C, zero, zero, 1.0, Sz, Szz, norm2, 0.5, sc.hsig_scale(c, 50), c)
        assert h is want_h
        assert new[1][0] == np.float32(100.0) * np.float32(100.0) and new[1][1] == np.float32(0.01) * np.float32(0.01)
        assert np.all(new[1][2:] == new[1][2]) and 0.99 < new[1][2] < 1.01
        assert np.all(new[3] == 0) != want_h                          # h = 0 stalls p_c (here from zero: it stays zero)
        assert np.array_equal(new[0], (np.float32(0.5) * np.float32(1.0)) * np.sqrt(C) * Sz)


def test_restatement_learns_cartpole_on_the_c_oracle():
    """conf/cartpole_sep_cma.yaml at 64 offspring (to keep it short), 5 episodes, 40 generations: the best return holds 500 over
    the last ten generations."""
    n, E, P = 64, 5, 226
    s = sc.SepCmaNP(P, 0.5, 1.0, n, seed=0)
    best, steps = [], []
    for gen in range(40):
        init = co.init_states_uniform(0, gen, 0, n, E, 4, False)
        fit, _, _ = co.rollout_cartpole(s.theta(), init, E, 500)
        best.append(s.evaluate(fit))
        steps.append(float(s.step))
    first = next(g for g in range(40) if min(best[g:]) == 500)
    print("best per generation:", best, "\nholds 500 from generation", first, "step:", steps[-1],
          "sqrt(C) range:", float(np.sqrt(s.C.min())), float(np.sqrt(s.C.max())))
    assert min(best[-10:]) == 500, best
    assert s.step != 1.0 and not np.all(s.C == 1.0) and s.C.min() >= 1e-4 and s.C.max() <= 1e4
    assert s.curr_sigma == 0.5 and s.t == 40


def test_builder_builds_sep_cma_es_from_its_config():
    import builder
    from learning_strategies.evolution.offspring_strategies import sep_cma_constants, sep_cma_es
    cfg = yaml.load(open(os.path.join(SRC, "conf", "cartpole_sep_cma.yaml")), Loader=yaml.FullLoader)
    s = builder.build_strategy(cfg["strategy"])
    assert type(s) is sep_cma_es and s.offspring_num == 256 and s.elite_num == 128 and s.curr_sigma == 0.5 and s.sigma_decay == 1.0
    assert s.scale_limits == (0.01, 100.0) and s.step_limits == (1e-6, 1e6) and s.noise == "philox"
    assert cfg["env"]["name"] == "CartPole-v1" and cfg["network"]["gru"] is False
    s2 = builder.build_strategy({**cfg["strategy"], "elite_num": 32, "scale_limits": [0.5, 2.0], "step_limits": [0.1, 10.0], "seed": 7})
    assert s2.elite_num == 32 and s2.scale_limits == (0.5, 2.0) and s2.step_limits == (0.1, 10.0) and s2.seed == 7
    assert s2.get_wandb_cfg()["elite_num"] == 32
    for key, bad in (("offspring_num", 3), ("offspring_num", 0), ("offspring_num", 4.5), ("elite_num", 0), ("elite_num", 257),
                     ("elite_num", -1), ("scale_limits", [1.5, 2.0]), ("scale_limits", [0.0, 2.0]), ("scale_limits", [0.5, 0.9]),
                     ("step_limits", [2.0, 3.0]), ("step_limits", [0.1, 0.5]), ("step_limits", [-1.0, 2.0]), ("noise", "numpy")):
        with pytest.raises(ValueError):
            builder.build_strategy({**cfg["strategy"], key: bad})
    with pytest.raises(KeyError):
        builder.build_strategy({k: v for k, v in cfg["strategy"].items() if k != "sigma_decay"})
    # the product's constants are the restatement's, bit for bit (they are formed once on the host and handed to the kernels)
    for n, P, mu in ((256, 226, 128), (64, 6562, 5), (4, 581, 4)):
        got, w = sep_cma_constants(n, P, mu)
        want, ww = sc.constants(n, P, mu)
        assert got == want and np.array_equal(w, ww) and w.dtype == np.float32
