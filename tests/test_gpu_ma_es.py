"""The ma_es strategy on the device against its numpy restatement (tests/ma_es_np.py) and float64.

  * ses_perturb_maes (M = I + 0.3 randn / sqrt(P), step 1.37, a generation key above 2^32 in one case): every element of D within
    product_tolerance of the float64 product (tests/test_ma_es_host.py shows the bound catches one wrong element), theta bit-equal to
    the restatement fed the device's D, any row range the matching slice of the whole population (D included; rows [5, 75) of 260
    start off a tile boundary), M = I gives the normals themselves, and at the three smaller shapes D bit-equal to the k-ascending
    fma chain restated on the host;
  * ses_maes_generation: Sz within sepcma_tolerance of float64; Sd, qv and every element of G within product_tolerance; norm2
    bit-equal to the ordered float64 sum of the device's p_sigma'; (mu, p_sigma, M)' bit-equal to update() fed the device's Sz, Sd,
    qv, G and norm2; step' the restatement's float32 or the adjacent one (two exp implementations within one double ulp each can
    round to neighbouring floats, no further); best = max(fitness); theta_next bit-equal to the restatement's population of the new
    state with the device's step' and D, and that D bit-equal to ses_perturb_maes of the new state (and to the host's chain at the
    smaller shapes); d_in = NULL the same state bit for bit; a shard call and a call without rows the same state; mu = 1, mu = n
    and the default; tie-free and CartPole-like fitness;
  * each step limit binding, and neither;
  * one handle over changing n with openai_es and lm_ma_es generations in between;
  * the front end rejects odd shapes, aliased buffers and a policy of 1028 parameters;
  * ses_run_generations with SES_STRATEGY_MA_ES bit-equal to per-generation ESLoop.generation calls;
  * conf/cartpole_ma_es.yaml end to end: learns, adapts step and matrix, restores from a snapshot bit for bit.
Shapes (n, P): the smallest population and policy (one row tile, a column tile of one element, odd P); ragged in both dimensions;
the config's policy with more than one chunk of tiles; the largest policy (P mod 32 = 4, M in several tiles each way); past the
8192-row switch of the rank path.
"""
import contextlib
import functools
import io
import os

import numpy as np
import pytest
import torch
import yaml

import lm_ma_np as lm
import ma_es_np as ma
import sep_cma_np as sc
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
SIGMA, SEED, DECAY = 0.5, 20241019, 0.999
SES_ERR_UNSUPPORTED = -2                                  # include/ses.h
NEXT_SIGMA = np.float32(SIGMA * DECAY)
SHAPES = {97: (1, 1, False), 161: (3, 1, False), 226: (4, 2, True), 932: (24, 4, False), 1028: (27, 4, False)}
CASES = [(4, 97), (37, 161), (260, 226), (300, 932), (8196, 226)]
IDS = [f"n{n}-P{P}" for n, P in CASES]
CHAIN_ON_HOST = {(4, 97), (37, 161), (260, 226)}          # where the host restates the fma chains themselves, bit for bit
WORST = {}


@pytest.fixture(scope="module")
def handles():
    from ses import HipES
    made = {}

    def get(P, key=None):
        if (P, key) not in made:
            S, A, disc = SHAPES[P]
            made[(P, key)] = HipES(None, S, A, disc, False)
            assert made[(P, key)].P == P
        return made[(P, key)]

    yield get
    for h in made.values():
        h.close()
    if WORST:
        print("\nworst |x - x64| / tol per (what, n, P)")
        for key, r in sorted(WORST.items()):
            print(f"  {key}: {r:.4f}")


@functools.lru_cache(maxsize=12)
def cached_noise(seed, gen, first, rows, P):
    """the oracle's normals of a chunk, drawn once for the cases that share (gen, n, P)"""
    z = co.noise(seed, gen, first, rows, P)
    z.setflags(write=False)
    return z


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


def near(a, b):
    """float32 a and b are equal or adjacent"""
    return abs(int(bits(np.array([a], np.float32))[0]) - int(bits(np.array([b], np.float32))[0])) <= 1


def fitness(kind, n, rng):
    """the generators of tests/test_gpu_es_tail_f64.py: tie-free, and CartPole-like (small integers and saturated returns)"""
    if kind == "perm":
        return rng.permutation(n).astype(np.float32) * 0.25 - 7.0
    fit = rng.randint(0, 60, n).astype(np.float32)
    sat = rng.rand(n) < 0.5
    fit[sat] = rng.choice(np.array([500.0, 137.2, 10.0, 9.8], np.float32), int(sat.sum()))
    return fit


def random_state(P, rng, ps_scale=1.0):
    """(mu, p_sigma, M, step): mu random, p_sigma standard normal times ps_scale, M = I + 0.3 randn / sqrt(P), step 1.37"""
    mu = (rng.randn(P) * 0.3).astype(np.float32)
    ps = (rng.randn(P) * ps_scale).astype(np.float32)
    M = (np.eye(P) + 0.3 * rng.randn(P, P) / np.sqrt(P)).astype(np.float32)
    return mu, ps, M, np.array([1.37], np.float32)


def make_params(c, step_limits=(1e-6, 1e6)):
    """a SesMaesParams from the RESTATEMENT's constants and factors"""
    from ses import _lib
    p = _lib.SesMaesParams()
    p.mu = c["mu"]
    p.mueff, p.c_sigma, p.d_sigma, p.chi, p.c_1, p.c_mu = (c[k] for k in ("mueff", "c_sigma", "d_sigma", "chi", "c_1", "c_mu"))
    p.a_m, p.c1h, p.cmuh = (float(x) for x in ma.factors(c))
    p.step_lo, p.step_hi = step_limits
    return p


def check_product(got, want64, tol, what, key):
    ratio = np.abs(got.astype(np.float64) - want64) / tol
    worst = float(ratio.max())
    WORST[key] = max(WORST.get(key, 0.0), worst)
    print(f"{what}: worst |x - x64| / tol = {worst:.4f}")
    assert worst <= 1.0, f"{what}: element {np.unravel_index(int(ratio.argmax()), ratio.shape)} is {worst:.3f} of the float64 bound away"
    assert worst > 1e-4, f"{what}: suspiciously exact"


def draw(es, state, gen, first, rows):
    """(theta, D) of rows [first, first + rows) on the host"""
    theta, D = es.perturb_maes(dev(state[0]), dev(state[2]), dev(state[3]), SIGMA, SEED, gen, first, rows, want_d=True)
    return host(theta), host(D)


@pytest.mark.parametrize("n,P", CASES, ids=IDS)
def test_perturb_maes_against_float64_and_restatement(handles, n, P):
    es = handles(P)
    rng = np.random.RandomState(n + P)
    state = random_state(P, rng)
    mu, _, M, step = state
    gen = 2 ** 32 + 5 if n == 260 else 9
    z = cached_noise(SEED, gen, 0, n, P)
    theta, D = draw(es, state, gen, 0, n)
    assert theta.shape == D.shape == (n, P)
    check_product(D, ma.d_f64(M, z), ma.d_tolerance(M, z), f"n={n} P={P}: D", ("D", n, P))
    assert_bit_equal(theta, ma.population(mu, step[0], SIGMA, D), "whole population")
    assert not np.array_equal(theta[0], theta[1]) and not np.array_equal(D, z)
    if (n, P) in CHAIN_ON_HOST:
        assert_bit_equal(D, ma.d_device_order(M, z), "D against the fma chain on the host")
    ranges = [(0, 1), (1, 2), (n - 3, 3)] + ([(5, 70), (32, 33)] if n == 260 else [])
    for first, rows in ranges:
        th, d = draw(es, state, gen, first, rows)
        assert_bit_equal(th, theta[first:first + rows], f"rows [{first}, +{rows})")
        assert_bit_equal(d, D[first:first + rows], f"rows [{first}, +{rows}): D")
    # without a D buffer: the same theta
    only = es.perturb_maes(dev(mu), dev(M), dev(step), SIGMA, SEED, gen, 0, n)
    assert_bit_equal(host(only), theta, "theta without d_out")
    # the identity passes the normals through: fma(z, 1, 0) and fma(z', 0, z) are exact
    eye = (mu, None, np.eye(P, dtype=np.float32), step)
    th_i, d_i = draw(es, eye, gen, 0, n)
    assert_bit_equal(d_i, z, "M = I: D is the noise")
    assert_bit_equal(th_i, mu[None, :] + (np.float32(SIGMA) * step[0]) * z, "M = I: isotropic rows")


def generation(es, fit, gen, state, D, c, weights, first_row, n_rows, step_limits=(1e-6, 1e6)):
    """ses_maes_generation from copies of `state` (D: the evaluated population's, or None): dict of host arrays"""
    out = tuple(es.zeros(*x.shape) for x in state)
    best = es.zeros(1)
    d_next = es.zeros(n_rows, es.P)
    theta, sz, sd, qv, g, norm2 = es.maes_generation(dev(fit), SEED, gen, SIGMA, make_params(c, step_limits), dev(weights),
                                                     tuple(dev(x) for x in state), out, None if D is None else dev(D), NEXT_SIGMA,
                                                     gen + 1, first_row, n_rows, d_next_out=d_next, best=best, want_sums=True)
    es.sync()
    return dict(state=tuple(host(x) for x in out), theta=host(theta), d_next=host(d_next), best=host(best)[0], Sz=host(sz), Sd=host(sd),
                qv=host(qv), G=host(g), norm2=float(host(norm2)[0]))


def check_generation(res, state, D, fit, gen, c, weights, what, n, P, step_limits=(1e-6, 1e6), products=True):
    """everything but theta_next: the sums and products against float64, the new state against update() fed the device's numbers.
    Returns (the restatement's state with the DEVICE's step', info)."""
    out = res["state"]
    w = sc.row_weights(fit, weights)
    z = cached_noise(SEED, gen, 0, n, P)
    cs = sc.chunk_sums_f64(w, SEED, gen, P, noise=cached_noise)
    ratio = np.abs(res["Sz"].astype(np.float64) - cs["Sz"].sum(0)) / sc.sepcma_tolerance(n, "z", cs["Az"].sum(0))
    assert ratio.max() <= 1.0, f"{what}: Sz: parameter {int(ratio.argmax())} is {ratio.max():.3f} of the float64 bound away"
    WORST[("Sz", n, P)] = max(WORST.get(("Sz", n, P), 0.0), float(ratio.max()))
    assert res["norm2"] == sc.norm2_device_order(out[1]), f"{what}: norm2 {res['norm2']!r} vs {sc.norm2_device_order(out[1])!r}"
    M = state[2]
    if products:
        check_product(res["Sd"], ma.matvec_f64(M, res["Sz"]), ma.matvec_tolerance(M, res["Sz"]), f"{what}: Sd", ("Sd", n, P))
        check_product(res["qv"], ma.matvec_f64(M, out[1]), ma.matvec_tolerance(M, out[1]), f"{what}: qv", ("qv", n, P))
        check_product(res["G"], ma.g_f64(w, D, z), ma.g_tolerance(w, D, z), f"{what}: G", ("G", n, P))
    want, info = ma.update(state[0], state[1], M, state[3][0], res["Sz"], res["Sd"], res["qv"], res["G"], res["norm2"], SIGMA, c,
                           step_limits)
    for name, got, wnt in zip(("mu", "p_sigma", "M"), out[:3], want[:3]):
        assert_bit_equal(got, wnt, f"{what}: {name}")
    got_step = out[3]
    assert got_step.shape == (1,) and got_step.dtype == np.float32
    d = abs(int(bits(got_step)[0]) - int(bits(np.array([want[3]], np.float32))[0]))
    assert d <= 1, f"{what}: step' {got_step[0]!r} vs {want[3]!r}: {d} float32 steps apart"
    assert res["best"] == fit.max(), (res["best"], fit.max())
    return want[:3] + (got_step,), info


@pytest.mark.parametrize("kind", ["perm", "cartpole"])
@pytest.mark.parametrize("n,P", CASES, ids=IDS)
def test_maes_generation_against_float64_and_restatement(handles, n, P, kind):
    es = handles(P)
    rng = np.random.RandomState((n * 31 + P + len(kind)) % (2 ** 31))
    fit = fitness(kind, n, rng)
    gen = 11                                                            # (shared by the two kinds: one set of normals per shape)
    first = (n // 2) | 1 if n > 4 else 1                                # a shard in the middle of the population
    rows = min(n - first - 1, 301) if n > 4 else 2
    z = cached_noise(SEED, gen, 0, n, P)
    for mu_sel in (None, 1, n):
        c, weights = ma.constants(n, P, mu_sel)
        state = random_state(P, rng)
        _, D = draw(es, state, gen, 0, n)
        what = f"{kind} n={n} P={P} mu={c['mu']}"
        res = generation(es, fit, gen, state, D, c, weights, 0, n)
        new, _ = check_generation(res, state, D, fit, gen, c, weights, what, n, P)
        if (n, P) in CHAIN_ON_HOST and mu_sel is None:
            w = sc.row_weights(fit, weights)
            assert_bit_equal(res["G"], ma.g_device_order(w, D, z), f"{what}: G against the fma chain on the host")
            assert_bit_equal(res["Sd"], ma.matvec_device_order(state[2], res["Sz"]), f"{what}: Sd against its order on the host")
            assert_bit_equal(res["qv"], ma.matvec_device_order(state[2], new[1]), f"{what}: qv against its order on the host")
        assert not np.array_equal(new[2], state[2]) and not np.array_equal(new[0], state[0])
        # the next population: the restatement fed the device's D, and that D the perturbation's of the new state
        assert_bit_equal(res["theta"], ma.population(new[0], new[3][0], NEXT_SIGMA, res["d_next"]), f"{what}: theta_next")
        th2, d2 = es.perturb_maes(dev(new[0]), dev(new[2]), dev(new[3]), NEXT_SIGMA, SEED, gen + 1, 0, n, want_d=True)
        assert_bit_equal(host(d2), res["d_next"], f"{what}: d_next_out against ses_perturb_maes of the new state")
        assert_bit_equal(host(th2), res["theta"], f"{what}: theta_next against ses_perturb_maes of the new state")
        if mu_sel is not None:
            continue
        z1 = cached_noise(SEED, gen + 1, 0, n, P)
        check_product(res["d_next"], ma.d_f64(new[2], z1), ma.d_tolerance(new[2], z1), f"{what}: D of the next population", ("D", n, P))
        # d_in = NULL: the call recomputes D of all n rows; the same state and products bit for bit
        res0 = generation(es, fit, gen, state, None, c, weights, 0, n)
        for name in ("Sz", "Sd", "qv", "G", "theta", "d_next"):
            assert_bit_equal(res0[name], res[name], f"d_in = NULL: {name}")
        for name, x, y in zip(("mu", "p_sigma", "M", "step"), res0["state"], res["state"]):
            assert_bit_equal(x, y, f"d_in = NULL: {name}")
        assert res0["norm2"] == res["norm2"] and res0["best"] == res["best"]
        # a shard call as the replicated tail makes it (d_in = NULL, its own rows): the same state, the matching slice; and no rows
        res2 = generation(es, fit, gen, state, None, c, weights, first, rows)
        for name, x, y in zip(("mu", "p_sigma", "M", "step"), res2["state"], res["state"]):
            assert_bit_equal(x, y, f"shard call: {name}")
        assert_bit_equal(res2["G"], res["G"], "shard call: G")
        assert res2["best"] == fit.max() and res2["norm2"] == res["norm2"]
        assert_bit_equal(res2["theta"], res["theta"][first:first + rows], "shard call: theta_next")
        assert_bit_equal(res2["d_next"], res["d_next"][first:first + rows], "shard call: D of theta_next")
        res3 = generation(es, fit, gen, state, D, c, weights, 0, 0)
        assert res3["theta"].shape == (0, P) and res3["best"] == fit.max() and res3["norm2"] == res["norm2"]
        for name, x, y in zip(("mu", "p_sigma", "M", "step"), res3["state"], res["state"]):
            assert_bit_equal(x, y, f"no rows: {name}")


def test_each_step_limit_binds_and_neither(handles):
    """Each branch of the step by construction of the input state, asserted from the restatement's record of the path it took (info)
    and held bit for bit on the device like every other case."""
    n, P, gen = 37, 161, 21
    es = handles(P)
    rng = np.random.RandomState(78)
    fit = fitness("perm", n, rng)
    c, weights = ma.constants(n, P)
    state = random_state(P, rng)
    _, D = draw(es, state, gen, 0, n)

    def run(st, step_limits=(1e-6, 1e6)):
        res = generation(es, fit, gen, st, D, c, weights, 0, 0, step_limits)
        return check_generation(res, st, D, fit, gen, c, weights, "limits", n, P, step_limits, products=False)

    # a path of the natural length: the exponent uncapped, no limit binds
    new, info = run(state)
    assert not info["capped"] and abs(info["exponent"]) < 0.5
    assert 1e-6 < new[3][0] < 1e6 and near(new[3][0], info["unclamped"]) and new[3][0] != state[3][0]
    # a path thirty times as long ((c_sigma / d_sigma) (30 * 0.93 - 1) = 1.7 at this shape): the exponent is capped at 1
    long_state = state[:1] + (state[1] * np.float32(30.0),) + state[2:]
    new0, info0 = run(long_state)
    assert info0["capped"] and info0["exponent"] == 1.0 and near(new0[3][0], info0["unclamped"]) and 3.7 < new0[3][0] < 3.75   # 1.37 e
    # the same against step limits that bind: the capped rise against the upper, a vanishing path against the lower
    new_hi, info_hi = run(long_state, (0.5, 2.0))
    assert info_hi["unclamped"] > 2.0 and new_hi[3][0] == np.float32(2.0)
    short_state = state[:1] + (np.zeros(P, np.float32),) + state[2:]
    new_lo, info_lo = run(short_state, (1.36, 2.0))
    assert not info_lo["capped"] and info_lo["exponent"] < -0.02 and info_lo["unclamped"] < 1.36 and new_lo[3][0] == np.float32(1.36)
    # the matrix does not depend on the limits, the mean uses the OLD step
    assert_bit_equal(new_hi[2], new0[2], "M' under a binding limit")
    assert_bit_equal(new_hi[0], new0[0], "mu' under a binding limit")


def test_generation_sequence_on_one_handle(handles):
    """Generations of changing size on ONE handle, with openai_es and lm_ma_es generations in between that lay the handle's scratch
    out differently: every result against float64 and the restatement (a rank vector left uncleared would be counted twice).  The
    state carries on from generation to generation, D with it (d_next_out of one call is d_in of the next where n stays)."""
    P = 226
    es = handles(P, "sequence")
    rng = np.random.RandomState(P)
    seq = [(260, None), (260, None), (4096, None), (9000, "openai_es"), (4096, "lm_ma_es"), (4, None), (8196, "lm_ma_es"), (8196, None)]
    state = random_state(P, rng)
    carried = None                                                       # (n, gen, D) of the population the last call drew
    for k, (n, between) in enumerate(seq):
        gen = 100 + k
        fit = fitness(("perm", "cartpole")[k % 2], n, rng)
        if between == "openai_es":
            junk = fitness("perm", (n * 3) // 4, rng)
            es.openai_generation(dev(junk), SEED, 1, 0.05, SIGMA, 1e-3, tuple(es.zeros(P) for _ in range(3)),
                                 tuple(es.zeros(P) for _ in range(3)), SIGMA, 2, 0, 1)
        elif between == "lm_ma_es":
            from ses import _lib
            junk = fitness("perm", n + 7, rng)
            cl, wl = lm.constants(n + 7, P, m=3)
            pl, tab = _lib.SesLmmaParams(), lm.tables(cl)
            pl.mu, pl.m = cl["mu"], cl["m"]
            pl.mueff, pl.c_sigma, pl.d_sigma, pl.chi = cl["mueff"], cl["c_sigma"], cl["d_sigma"], cl["chi"]
            pl.step_lo, pl.step_hi = 1e-6, 1e6
            for name in ("cd", "ad", "ac", "bc"):
                for j in range(3):
                    getattr(pl, name)[j] = float(tab[name][j])
            lst = lambda: (es.zeros(P), es.zeros(P), es.zeros(3, P), es.zeros(1) + 1.0)
            es.lmma_generation(dev(junk), SEED, 1, SIGMA, pl, dev(wl), 2, 3, lst(), lst(), SIGMA, 2, 0, 2)
        c, weights = ma.constants(n, P)
        if carried is not None and carried[:2] == (n, gen):
            D = carried[2]
        else:
            _, D = draw(es, state, gen, 0, n)
        res = generation(es, fit, gen, state, D, c, weights, 0, n)
        new, _ = check_generation(res, state, D, fit, gen, c, weights, f"sequence step {k} (n={n})", n, P, products=k in (0, 5))
        assert_bit_equal(res["theta"], ma.population(new[0], new[3][0], NEXT_SIGMA, res["d_next"]), f"sequence step {k}: theta_next")
        state = res["state"]
        carried = (n, gen + 1, res["d_next"])
    assert carried[0] == 8196


def test_front_end_rejects_bad_shapes(handles):
    from ses import SesError, _lib
    P = 226
    es = handles(P)
    c, w = ma.constants(8, P)
    params, weights = make_params(c), dev(w)

    def st():
        return es.zeros(P), es.zeros(P), es.zeros(P, P), es.zeros(1) + 1.0

    ok, out = st(), st()
    D = es.zeros(8, P)
    args = (0.5, params, weights)
    tail = (0.5, 1, 0, 0)
    es.maes_generation(es.zeros(8), 0, 0, *args, ok, out, D, *tail)                              # the well-formed calls
    es.maes_generation(es.zeros(8), 0, 0, *args, ok, out, None, *tail)
    for n in (3, 2, 0):
        with pytest.raises(SesError):
            es.maes_generation(es.zeros(n), 0, 0, *args, ok, out, None, *tail)
    for mu in (0, 9, -1):
        with pytest.raises(SesError):
            es.maes_generation(es.zeros(8), 0, 0, 0.5, make_params({**c, "mu": mu}), weights, ok, out, D, *tail)
    with pytest.raises(SesError):                                                               # a table shorter than mu
        es.maes_generation(es.zeros(8), 0, 0, 0.5, params, weights[:3].contiguous(), ok, out, D, *tail)
    with pytest.raises(SesError):                                                               # not a SesMaesParams
        es.maes_generation(es.zeros(8), 0, 0, 0.5, _lib.SesLmmaParams(), weights, ok, out, D, *tail)
    with pytest.raises(SesError):                                                               # bad step limits
        es.maes_generation(es.zeros(8), 0, 0, 0.5, make_params(c, (2.0, 1.0)), weights, ok, out, D, *tail)
    with pytest.raises(SesError):                                                               # aliased in and out
        es.maes_generation(es.zeros(8), 0, 0, *args, ok, ok, D, *tail)
    for k in range(4):
        with pytest.raises(SesError):
            es.maes_generation(es.zeros(8), 0, 0, *args, ok, out[:k] + (ok[k],) + out[k + 1:], D, *tail)
    with pytest.raises(SesError):                                                               # D of the next rows over D of these
        es.maes_generation(es.zeros(8), 0, 0, *args, ok, out, D, 0.5, 1, 0, 8, d_next_out=D)
    with pytest.raises(SesError):                                                               # rows outside the population
        es.maes_generation(es.zeros(8), 0, 0, *args, ok, out, D, 0.5, 1, 6, 3)
    for bad_D in (es.zeros(7, P), es.zeros(8, P + 1), es.zeros(8 * P)):
        with pytest.raises(SesError):
            es.maes_generation(es.zeros(8), 0, 0, *args, ok, out, bad_D, *tail)
    with pytest.raises(SesError):
        es.maes_generation(es.zeros(8), 0, 0, *args, ok, out, D, 0.5, 1, 0, 4, d_next_out=es.zeros(5, P))
    for bad_M in (es.zeros(P - 1, P), es.zeros(P, P + 1), es.zeros(P * P), es.zeros(20, P)):    # a wrong M shape
        with pytest.raises(SesError):
            es.maes_generation(es.zeros(8), 0, 0, *args, ok[:2] + (bad_M, ok[3]), out, D, *tail)
        with pytest.raises(SesError):
            es.perturb_maes(es.zeros(P), bad_M, es.zeros(1), 0.5, 0, 0, 0, 4)
    with pytest.raises(SesError):
        es.maes_generation(es.zeros(8), 0, 0, *args, ok[:1] + (es.zeros(P + 1),) + ok[2:], out, D, *tail)
    with pytest.raises(SesError):
        es.maes_generation(es.zeros(8), 0, 0, *args, ok[:3] + (es.zeros(2),), out, D, *tail)
    with pytest.raises(SesError):
        es.perturb_maes(es.zeros(225), es.zeros(P, P), es.zeros(1), 0.5, 0, 0, 0, 4)
    with pytest.raises(SesError):
        es.perturb_maes(es.zeros(P), es.zeros(P, P), es.zeros(P), 0.5, 0, 0, 0, 4)
    with pytest.raises(SesError):
        es.perturb_maes(es.zeros(P), es.zeros(P, P), es.zeros(1), 0.5, 0, 0, 0, 0)
    with pytest.raises(SesError):
        es.perturb_maes(es.zeros(P), es.zeros(P, P), es.zeros(1), 0.5, 0, 0, 0, 4, d_out=es.zeros(5, P))
    # 1028 parameters (S = 27, A = 4: the first MLP shape past the limit): the wrapper refuses, and so does the library itself
    big = handles(1028)
    Pb = 1028
    assert _lib.MAES_MAX_P == 1024
    bst = lambda: (big.zeros(Pb), big.zeros(Pb), big.zeros(Pb, Pb), big.zeros(1) + 1.0)
    with pytest.raises(SesError, match="at most 1024"):
        big.perturb_maes(big.zeros(Pb), big.zeros(Pb, Pb), big.zeros(1), 0.5, 0, 0, 0, 4)
    with pytest.raises(SesError, match="lm_ma_es"):
        big.maes_generation(big.zeros(8), 0, 0, *args, bst(), bst(), None, *tail)
    import ctypes
    mu_b, M_b, step_b, theta_b = big.zeros(Pb), big.zeros(Pb, Pb), big.zeros(1), big.zeros(4, Pb)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = big._lib.ses_perturb_maes(big._h, ptr(mu_b), ptr(M_b), ptr(step_b), 0.5, 0, 0, 0, 4, ptr(theta_b), None)
    assert rc == SES_ERR_UNSUPPORTED
    a, b = bst(), bst()
    rc = big._lib.ses_maes_generation(big._h, ptr(big.zeros(8)), 8, 0, 0, 0.5, ctypes.byref(params), ptr(weights), ptr(a[0]), ptr(a[1]),
                                      ptr(a[2]), ptr(a[3]), None, ptr(b[0]), ptr(b[1]), ptr(b[2]), ptr(b[3]), 0.5, 1, 0, 0, None, None,
                                      None, None, None, None, None, None)
    assert rc == SES_ERR_UNSUPPORTED
    # the strategy class refuses such a network by name
    from learning_strategies.evolution.offspring_strategies import ma_es
    with pytest.raises(ValueError, match="lm_ma_es"):
        ma_es.check_parameters(Pb)


def small_cfg():
    # (200 steps: see tests/test_gpu_sep_cma.py small_cfg -- a best that varies tells the generations apart)
    return {"env": {"name": "CartPole-v1", "max_step": 200, "pomdp": False, "seed": 4},
            "network": {"name": "gym_model", "num_state": 4, "num_action": 2, "discrete_action": True, "gru": False},
            "strategy": {"name": "ma_es", "init_sigma": 0.3, "sigma_decay": 0.98, "offspring_num": 64, "seed": 2}}


def strategy_state(s):
    return {"mu": host(s.mu_model), "p_sigma": host(s._ps), "M": host(s.matrix), "step": host(s.step), "D": host(s._D)}


def test_run_generations_equals_per_generation_calls(tmp_path, monkeypatch):
    """ses_run_generations with SES_STRATEGY_MA_ES, k = 3, against three ESLoop.generation calls: the state (D included), theta,
    best[k]; and the two forms continue from each other."""
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
    assert sb.curr_sigma == sa.curr_sigma == sigmas[-1] and sb.t == sa.t == 3 and pop_b.gen == pop.gen == 3
    state = strategy_state(sb)
    assert state["M"].shape == (226, 226) and state["D"].shape == (64, 226)
    assert np.abs(state["mu"]).max() > 0 and state["step"][0] != 1.0 and not np.array_equal(state["M"], np.eye(226, dtype=np.float32))
    # and the two forms continue from each other: one more per-generation call on the batched run's state
    pop, best_a, _, _ = a.generation(pop)
    pop_b, best_b, _, _ = b.generation(pop_b)
    assert best_a.result() == best_b.result()
    assert_bit_equal(host(pop_b.theta), host(pop.theta), "generation after run_generations: theta")
    for k, v in strategy_state(sa).items():
        assert_bit_equal(strategy_state(sb)[k], v, f"generation after run_generations: {k}")
    # ... and a batched chunk on the per-generation run's state
    batch_a = _GenerationBatch(a, sa, pop)
    best2, _, _ = batch_a.run(2)
    for _ in range(2):
        pop_b, bb, _, _ = b.generation(pop_b)
    torch.cuda.synchronize()
    pop = batch_a.sync_back()
    assert float(best2[1]) == bb.result() and sa.t == sb.t == 6
    assert_bit_equal(host(pop.theta), host(pop_b.theta), "run_generations after generation: theta")
    for k, v in strategy_state(sa).items():
        assert_bit_equal(strategy_state(sb)[k], v, f"run_generations after generation: {k}")


def test_cartpole_ma_es_config_end_to_end(tmp_path, monkeypatch):
    """The bar is the host test's (tests/test_ma_es_host.py: the restatement reaches 500 on the C oracle): max(best) == 500."""
    import builder
    monkeypatch.chdir(tmp_path)
    cfg = yaml.load(open(os.path.join(SRC, "conf", "cartpole_ma_es.yaml")), Loader=yaml.FullLoader)
    loop = builder.build_loop(cfg, 40, 1, 5, False, 10 ** 9)
    with contextlib.redirect_stdout(io.StringIO()):
        pop = loop.run()
    best = [b for b, _ in loop.history]
    print("best per generation:", best)
    assert len(best) == 40 and max(best) == 500, best
    assert loop.batched_generations == 40                             # the run went through ses_run_generations
    s = loop.offspring_strategy
    M, step = host(s.matrix), float(host(s.step)[0])
    moved = float(np.abs(M - np.eye(226, dtype=np.float32)).max())
    print("step:", step, "max |M - I|:", moved)
    assert step != 1.0 and 1e-6 <= step <= 1e6
    assert M.shape == (226, 226) and moved > 1e-3 and np.isfinite(M).all()
    assert s.curr_sigma == 0.5 and all(sig == 0.5 for _, sig in loop.history) and s.t == 40
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
