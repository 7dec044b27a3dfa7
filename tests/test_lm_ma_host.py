"""lm_ma_es without a GPU: the constants, the linearity that pins the mean update to the paper's, the bound the device's dots are
held to (tests/lm_ma_np.py dot_tolerance), the numpy restatement learning CartPole on the C oracle and aligning a direction vector
with the long axis of a rotated cigar, and the builder.
"""
import math
import os

import numpy as np
import pytest
import yaml

import lm_ma_np as lm
import sep_cma_np as sc
from oracle import c_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
SEED, GEN = 4321, 19


def random_vectors(m, P, rng):
    """direction vectors of the length the fast ones reach, |M_j| ~ sqrt(P)"""
    return rng.randn(m, P).astype(np.float32)


def test_constants_against_hand_computed_values():
    """(n, P) = (256, 226) and (4096, 6756), the formulas of the issue typed out once more with the numbers in.  c_c[0] is capped
    at 1 where n >= P ((256, 226): 256 / 226 = 1.13); at (4096, 6756) the quotient 4096 / 6756 = 0.606 stays."""
    c, w = lm.constants(256, 226)
    cs, ws = sc.constants(256, 226)
    assert c["m"] == 20 == 4 + math.floor(3 * math.log(226)) and c["mu"] == 128 and np.array_equal(w, ws)
    assert all(c[k] == cs[k] for k in ("mueff", "c_sigma", "d_sigma", "chi"))
    assert c["mueff"] == pytest.approx(66.857796, rel=1e-6) and c["chi"] == pytest.approx(15.016681, rel=1e-6)
    assert len(c["c_d"]) == len(c["c_c"]) == 20
    assert c["c_d"][0] == 1.0 / 226.0 and c["c_d"][1] == pytest.approx(1.0 / 339.0, rel=1e-15)
    assert c["c_d"][19] == pytest.approx(1.0 / (1.5 ** 19 * 226.0), rel=1e-15) and 1.5 ** 19 == pytest.approx(2216.84, rel=1e-5)
    assert c["c_c"][0] == 1.0 and 256.0 / 226.0 > 1.0                                               # the cap binds
    assert c["c_c"][1] == pytest.approx(256.0 / 904.0, rel=1e-15) and c["c_c"][2] == pytest.approx(256.0 / 3616.0, rel=1e-15)
    assert c["c_c"][19] == pytest.approx(256.0 / (4.0 ** 19 * 226.0), rel=1e-15)
    t = lm.tables(c)
    assert all(t[k].dtype == np.float32 and t[k].shape == (20,) for k in ("cd", "ad", "ac", "bc"))
    assert t["cd"][0] == np.float32(1.0 / 226.0) and t["ad"][0] == np.float32(225.0 / 226.0)
    assert t["ac"][0] == 0.0 and t["bc"][0] == np.float32(math.sqrt(c["mueff"]))                   # c_c = 1: sqrt(mueff * 1 * 1)
    assert t["ac"][1] == np.float32(1.0 - 256.0 / 904.0)
    assert t["bc"][1] == np.float32(math.sqrt(c["mueff"] * (256.0 / 904.0) * (2.0 - 256.0 / 904.0)))
    assert t["bc"][1] == pytest.approx(5.7013, rel=1e-4)                                            # sqrt(66.8578 * 0.283186 * 1.716814) = sqrt(32.505)

    c, w = lm.constants(4096, 6756)
    assert c["m"] == 30 == 4 + math.floor(3 * math.log(6756)) and c["mu"] == 2048 and w.shape == (2048,)
    raw = [math.log(2048.5) - math.log(k + 1) for k in range(2048)]
    tot = math.fsum(raw)
    mueff = 1.0 / math.fsum((x / tot) ** 2 for x in raw)
    assert c["mueff"] == pytest.approx(mueff, rel=1e-12)
    assert c["c_sigma"] == pytest.approx((mueff + 2.0) / (6756.0 + mueff + 5.0), rel=1e-12)
    assert c["chi"] == pytest.approx(math.sqrt(6756.0) * (1.0 - 1.0 / 27024.0 + 1.0 / (21.0 * 6756.0 ** 2)), rel=1e-14)
    assert c["c_d"][0] == 1.0 / 6756.0 and c["c_d"][29] == pytest.approx(1.0 / (1.5 ** 29 * 6756.0), rel=1e-15)
    assert c["c_c"][0] == 4096.0 / 6756.0 < 1.0                                                     # no cap here
    assert c["c_c"][1] == pytest.approx(1024.0 / 6756.0, rel=1e-15) and c["c_c"][29] == pytest.approx(4096.0 / (4.0 ** 29 * 6756.0), rel=1e-15)
    t = lm.tables(c)
    assert t["bc"][0] == np.float32(math.sqrt(mueff * (4096.0 / 6756.0) * (2.0 - 4096.0 / 6756.0)))
    # a population of at least P rows caps the first rate, whatever P
    assert lm.constants(8196, 226)[0]["c_c"][0] == 1.0 and lm.constants(1024, 581)[0]["c_c"][0] == 1.0
    assert lm.constants(1025, 6562)[0]["c_c"][0] == 1025.0 / 6562.0


def test_default_memory_and_its_range():
    assert [lm.default_memory(P) for P in (226, 581, 6562, 6756)] == [20, 23, 30, 30]
    assert lm.default_memory(16384) == 32 and lm.default_memory(10 ** 6) == 32                     # 4 + floor(29.1) = 33: capped
    for m in (0, 1, 32):
        c, _ = lm.constants(64, 226, m=m)
        assert c["m"] == m == len(c["c_d"]) == len(c["c_c"]) and lm.tables(c)["cd"].shape == (m,)


def test_rounding_counts():
    assert [lm.dot_rounding_count(P) for P in (64, 226, 256, 257, 581, 6562, 6756, 16384)] == [9, 9, 9, 11, 11, 17, 17, 26]
    assert [lm.sdot_rounding_count(P) for P in (226, 1024, 1025, 6562, 16384)] == [11, 11, 12, 17, 26]


@pytest.mark.parametrize("n,P", [(64, 226), (300, 581)])
def test_transform_of_the_weighted_sum_is_the_weighted_sum_of_the_transforms(n, P):
    """In float64 the transform applied to sum w_i z_i equals sum w_i v_i to 1e-12 relative: the transform is linear, so the mean
    update mu' = mu + sigma step T(Sz) is the paper's mu + sigma step sum w_i d_i."""
    rng = np.random.RandomState(n + P)
    c, weights = lm.constants(n, P)
    M = random_vectors(c["m"], P, rng)
    w = sc.row_weights(rng.permutation(n).astype(np.float32), weights)
    z = co.noise(SEED, GEN, 0, n, P).astype(np.float64)
    of_sum = lm.transform_f64(w @ z, M, c, c["m"])
    sum_of = w @ lm.transform_f64(z, M, c, c["m"])
    rel = np.linalg.norm(of_sum - sum_of) / np.linalg.norm(sum_of)
    print(f"n={n} P={P} m={c['m']}: |T(sum w z) - sum w T(z)| / |sum w T(z)| = {rel:.3e}")
    assert rel <= 1e-12
    assert np.linalg.norm(of_sum - w @ z) / np.linalg.norm(w @ z) > 1e-3       # (the transform is not the identity here)


@pytest.mark.parametrize("P", [226, 581, 6562])
def test_dot_bound_holds_the_device_order_and_catches_one_wrong_element(P):
    """The float32 dots in the device's order stay inside dot_tolerance of the float64 dot, the error the bound covers is real, and
    ONE entry of M_j off by 1e-3 relative (the entry that carries the row's largest term) moves the float64 dot past the bound."""
    rng = np.random.RandomState(P)
    rows = 16
    Mj = random_vectors(1, P, rng)[0]
    v = co.noise(SEED, GEN, 0, rows, P)
    d32, d64, tol = lm.dot_device_order(Mj, v), lm.dot_f64(Mj, v), lm.dot_tolerance(Mj, v)
    ratio = np.abs(d32.astype(np.float64) - d64) / tol
    print(f"P={P}: K={lm.dot_rounding_count(P)}, emulated device order, worst |err|/tol = {ratio.max():.4f}")
    assert d32.dtype == np.float32 and ratio.max() <= 1.0 and ratio.max() > 1e-3
    assert lm.dot_device_order(Mj, v[3]) == d32[3]
    for i in range(rows):
        p = int(np.argmax(np.abs(Mj * v[i])))
        wrong = Mj.astype(np.float64)
        wrong[p] *= 1.0 + 1e-3
        assert abs(float(v[i].astype(np.float64) @ wrong) - d64[i]) > tol[i], (i, p)
    # the update's dot, one vector
    s32, s64 = lm.sdot_device_order(Mj, v[0]), float(lm.dot_f64(Mj, v[0]))
    assert abs(float(s32) - s64) <= lm.sdot_tolerance(Mj, v[0])


def test_sz_device_order_is_the_sep_cma_restatements():
    for n, P in ((1300, 226), (32, 64), (260, 581)):
        rng = np.random.RandomState(n)
        w = sc.row_weights(rng.permutation(n).astype(np.float32), lm.constants(n, P)[1])
        a, b = lm.sz_device_order(w, SEED, GEN, P), sc.emulate_device_sums(w, SEED, GEN, P)[0]
        assert a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_no_vectors_is_isotropic_sampling():
    rng = np.random.RandomState(2)
    P, n = 226, 7
    mu = rng.randn(P).astype(np.float32)
    step, sigma = np.float32(1.7), 0.3
    z = co.noise(SEED, GEN, 0, n, P)
    want = mu + (np.float32(sigma) * step) * z
    for m in (0, 5):                                                     # no vectors at all, and vectors none of which is active yet
        c, _ = lm.constants(n, P, m=m)
        theta, dots = lm.population(mu, random_vectors(m, P, rng), step, sigma, SEED, GEN, lm.tables(c), 0, 0, n)
        assert theta.dtype == np.float32 and np.array_equal(theta, want) and dots.shape == (n, 0)


def test_population_is_the_stated_arithmetic_and_slices():
    rng = np.random.RandomState(3)
    P, n = 581, 9
    c, _ = lm.constants(n, P, m=3)
    tab = lm.tables(c)
    mu, M = rng.randn(P).astype(np.float32), random_vectors(3, P, rng)
    step = np.float32(0.8)
    whole, dots, vs = lm.population(mu, M, step, 0.5, SEED, GEN, tab, 3, 0, n, chain=True)
    assert whole.shape == (n, P) and dots.shape == (n, 3) and len(vs) == 3
    v = co.noise(SEED, GEN, 4, 1, P)[0]
    for j in range(3):
        assert np.array_equal(vs[j][4], v) and dots[4, j] == lm.dot_device_order(M[j], v)
        v = tab["ad"][j] * v + (tab["cd"][j] * dots[4, j]) * M[j]
    assert np.array_equal(whole[4], mu + (np.float32(0.5) * step) * v)
    assert not np.array_equal(whole, lm.population(mu, M, step, 0.5, SEED, GEN, tab, 0, 0, n)[0])
    for first in (0, 1, n - 3):
        for rows in (1, 2, 3):
            part, d = lm.population(mu, M, step, 0.5, SEED, GEN, tab, 3, first, rows)
            assert np.array_equal(part, whole[first:first + rows]) and np.array_equal(d, dots[first:first + rows])
    # given dots are used as they are
    other, used = lm.population(mu, M, step, 0.5, SEED, GEN, tab, 3, 0, n, dots=dots * np.float32(1.5))
    assert np.array_equal(used, dots * np.float32(1.5)) and not np.array_equal(other, whole)


def test_update_is_the_stated_arithmetic():
    rng = np.random.RandomState(4)
    n, P = 256, 226
    c, _ = lm.constants(n, P, m=4)
    tab = lm.tables(c)
    mu, ps, M = rng.randn(P).astype(np.float32), rng.randn(P).astype(np.float32), random_vectors(4, P, rng)
    Sz = (rng.randn(P) * 0.1).astype(np.float32)
    norm2 = sc.norm2_device_order(sc.path_sigma(ps, Sz, c))
    (mu2, ps2, M2, step2), info = lm.update(mu, ps, M, 1.3, Sz, None, norm2, 0.5, c, tab, 2)
    assert np.array_equal(ps2, sc.path_sigma(ps, Sz, c))
    u = Sz
    for j in range(2):
        assert info["sdots"][j] == lm.sdot_device_order(M[j], u)
        u = tab["ad"][j] * u + (tab["cd"][j] * info["sdots"][j]) * M[j]
    assert np.array_equal(info["u_last"], u) and np.array_equal(mu2, mu + (np.float32(0.5) * np.float32(1.3)) * u)
    assert np.array_equal(M2[0], tab["bc"][0] * Sz)                      # c_c[0] = 1 at n >= P: the first vector is replaced
    for j in range(1, 4):                                                # every vector moves, the inactive ones too
        assert np.array_equal(M2[j], tab["ac"][j] * M[j] + tab["bc"][j] * Sz)
    # the step: a path of the expected length leaves it (to a rounding), a long one is capped at e, the limits bind
    s1, i1 = lm.step_update(c["chi"] ** 2, 1.0, c)
    s2, i2 = lm.step_update((100.0 * c["chi"]) ** 2, 2.0, c)
    s3, _ = lm.step_update(0.0, 1.0, c)
    assert abs(float(s1) - 1.0) < 1e-6 and not i1["capped"] and i2["capped"] and s2 == np.float32(2.0 * math.e)
    assert s3 == np.float32(math.exp(-c["c_sigma"] / c["d_sigma"]))
    assert lm.step_update((100.0 * c["chi"]) ** 2, 2.0, c, (0.5, 3.0))[0] == np.float32(3.0)
    assert lm.step_update(0.0, 1.0, c, (0.9, 3.0))[0] == np.float32(0.9)
    # given dots are used as they are, and m = 0 moves the mean along Sz itself
    assert np.array_equal(lm.update(mu, ps, M, 1.3, Sz, info["sdots"], norm2, 0.5, c, tab, 2)[0][0], mu2)
    c0, _ = lm.constants(n, P, m=0)
    (mu0, _, M0, _), _ = lm.update(mu, ps, np.zeros((0, P), np.float32), 1.3, Sz, None, norm2, 0.5, c0, lm.tables(c0), 0)
    assert np.array_equal(mu0, mu + (np.float32(0.5) * np.float32(1.3)) * Sz) and M0.shape == (0, P)


def test_restatement_learns_cartpole_on_the_c_oracle():
    """conf/cartpole_lm_ma.yaml's settings (256 offspring, init_sigma 0.5, sigma_decay 1, the default 128 selected rows and 20
    vectors), 5 episodes, 40 generations: the criterion of the device's end-to-end test."""
    cfg = yaml.load(open(os.path.join(SRC, "conf", "cartpole_lm_ma.yaml")), Loader=yaml.FullLoader)["strategy"]
    n, E, P = cfg["offspring_num"], 5, 226
    s = lm.LmMaNP(P, cfg["init_sigma"], cfg["sigma_decay"], n, seed=0)
    assert (n, cfg["init_sigma"], cfg["sigma_decay"], s.c["m"], s.c["mu"]) == (256, 0.5, 1.0, 20, 128)
    best = []
    for gen in range(40):
        assert s.m_active == min(gen, 20)
        init = co.init_states_uniform(0, gen, 0, n, E, 4, False)
        fit, _, _ = co.rollout_cartpole(s.theta(), init, E, 500)
        best.append(s.evaluate(fit))
    norms = np.linalg.norm(s.M.astype(np.float64), axis=1)
    print("best per generation:", best, "\nstep:", float(s.step), "|M_j|:", np.round(norms, 2))
    assert max(best[-10:]) == 500 and min(best[-10:]) >= 400, best
    assert s.step != 1.0 and 1e-6 <= s.step <= 1e6 and norms.max() > 0 and s.curr_sigma == 0.5 and s.t == 40


def cigar_alignment(seed, generations=1200):
    """max_j |cos(M_j, long axis)| after `generations` of LmMaNP on f(x) = (v.x)^2 + 1e6 (|x|^2 - (v.x)^2), P = 64, n = 32, start
    3 * 1, init_sigma 1; v = a unit vector drawn from RandomState(seed), the strategy's noise seed = seed.  The step floor is lowered
    to 1e-20: with curvature 1e6 across the axis the step this problem asks for falls below the default floor of 1e-6 (seed 2 gets
    there before generation 1200), and a step held at its floor is no step-size adaptation any more -- the floor guards policy
    search against a collapsed distribution, it is not part of the algorithm this test is about."""
    P, n = 64, 32
    v = np.random.RandomState(seed).randn(P)
    v /= np.linalg.norm(v)
    s = lm.LmMaNP(P, 1.0, 1.0, n, seed=seed, step_limits=(1e-20, 1e6))
    s.mu = np.full(P, 3.0, np.float32)
    for _ in range(generations):
        x = s.theta().astype(np.float64)
        a = x @ v
        s.evaluate((-(a * a + 1e6 * ((x * x).sum(1) - a * a))).astype(np.float32))
    M = s.M.astype(np.float64)
    return float((np.abs(M @ v) / np.linalg.norm(M, axis=1)).max()), float(s.step)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_a_direction_vector_aligns_with_the_long_axis_of_a_rotated_cigar(seed):
    """>= 0.9 (a float64 prototype of the algorithm gave 0.990, 0.991, 0.996, 0.990 with its own normals; the margin is for the
    float32 sums).  This restatement: 0.988, 0.988, 0.951, 0.991 (NOTES.md)."""
    cos, step = cigar_alignment(seed)
    print(f"seed {seed}: max |cos| = {cos:.4f}, step = {step:.3e}")
    assert cos >= 0.9


def test_builder_builds_lm_ma_es_from_its_config():
    import builder
    from learning_strategies.evolution.offspring_strategies import lm_ma_constants, lm_ma_es, lm_ma_params
    cfg = yaml.load(open(os.path.join(SRC, "conf", "cartpole_lm_ma.yaml")), Loader=yaml.FullLoader)
    s = builder.build_strategy(cfg["strategy"])
    assert type(s) is lm_ma_es and s.offspring_num == 256 and s.elite_num == 128 and s.curr_sigma == 0.5 and s.sigma_decay == 1.0
    assert s.memory is None and s.step_limits == (1e-6, 1e6) and s.noise == "philox"         # memory: fixed once P is known
    assert cfg["env"]["name"] == "CartPole-v1" and cfg["network"]["gru"] is False
    s2 = builder.build_strategy({**cfg["strategy"], "elite_num": 32, "memory": 7, "step_limits": [0.1, 10.0], "seed": 7})
    assert s2.elite_num == 32 and s2.memory == 7 and s2.step_limits == (0.1, 10.0) and s2.seed == 7
    assert s2.get_wandb_cfg()["memory"] == 7 and s2.m_active(3) == 3 and s2.m_active(9) == 7
    assert builder.build_strategy({**cfg["strategy"], "memory": 0}).memory == 0
    for key, bad in (("offspring_num", 3), ("offspring_num", 0), ("offspring_num", 4.5), ("elite_num", 0), ("elite_num", 257),
                     ("elite_num", -1), ("memory", 33), ("memory", -1), ("memory", 2.5), ("step_limits", [2.0, 3.0]),
                     ("step_limits", [0.1, 0.5]), ("step_limits", [-1.0, 2.0]), ("noise", "numpy")):
        with pytest.raises(ValueError):
            builder.build_strategy({**cfg["strategy"], key: bad})
    with pytest.raises(KeyError):
        builder.build_strategy({k: v for k, v in cfg["strategy"].items() if k != "sigma_decay"})
    # the product's constants and tables are the restatement's, bit for bit (formed once on the host and handed to the kernels)
    for n, P, mu, m in ((256, 226, 128, None), (64, 6562, 5, 30), (4, 581, 4, 0), (4096, 6756, None, None)):
        got, w = lm_ma_constants(n, P, n // 2 if mu is None else mu, m)
        want, ww = lm.constants(n, P, mu, m)
        assert got == want and np.array_equal(w, ww) and w.dtype == np.float32
        p, tab = lm_ma_params(got, (1e-6, 1e6)), lm.tables(want)
        assert (p.mu, p.m, p.mueff, p.c_sigma, p.d_sigma, p.chi) == tuple(want[k] for k in ("mu", "m", "mueff", "c_sigma", "d_sigma", "chi"))
        assert p.step_lo == np.float32(1e-6) and p.step_hi == np.float32(1e6)
        for k in ("cd", "ad", "ac", "bc"):
            assert np.array_equal(np.array(getattr(p, k)[:want["m"]], np.float32), tab[k]), k
            assert all(x == 0.0 for x in getattr(p, k)[want["m"]:])
