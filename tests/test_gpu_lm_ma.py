"""The lm_ma_es strategy on the device against its numpy restatement (tests/lm_ma_np.py) and float64.

  * ses_perturb_lmma (random M with |M_j| ~ sqrt(P), step != 1, a generation key above 2^32 in one case; m_active in {0, 1, m}):
    every dot of every row within dot_tolerance of the float64 dot of the restated v_j (tests/test_lm_ma_host.py shows the bound
    catches one wrong element), theta bit-equal to the restatement fed the device's dots, any row range the matching slice of the
    whole population (dots included), theta different from the population without vectors;
  * ses_lmma_generation: Sz within sepcma_tolerance of float64, the mean chain's dots within sdot_tolerance, norm2 bit-equal to the
    ordered float64 sum of the device's p_sigma', (mu, p_sigma, M, u_last) bit-equal to update() fed the device's Sz, dots and
    norm2, step' the restatement's float32 or the adjacent one (two exp implementations within one double ulp each can round to
    neighbouring floats, no further), best = max(fitness), theta_next bit-equal to the restatement's population of the new state
    WITH the device's own step' and dots, a shard call and a call without rows the same state; mu = 1, mu = n and the default;
    tie-free and CartPole-like fitness;
  * every branch taken, by construction: the cap of the exponent, each step limit binding and neither, m_active < m and = m, and
    c_c[0] = 1 (M'[0] = bc[0] Sz exactly);
  * one handle over changing n with openai_es, pgpe and sep_cma_es generations in between;
  * the front end rejects odd shapes;
  * ses_run_generations with SES_STRATEGY_LM_MA_ES bit-equal to per-generation ESLoop.generation calls;
  * conf/cartpole_lm_ma.yaml end to end: learns, adapts step and vectors, restores from a snapshot bit for bit.
Shapes (n, P): the smallest population; a ragged round with P no multiple of 4 (one wave per row); exactly one chunk (four waves
per row, two quads per thread); a second chunk of one row with several rounds of the update loop (P > 1024: eight quads per
thread); past the 8192-row switch of the rank path.
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
import sep_cma_np as sc
from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
SIGMA, SEED, DECAY = 0.5, 20240915, 0.999
NEXT_SIGMA = np.float32(SIGMA * DECAY)
SHAPES = {226: (4, 2, True, False), 6562: (4, 2, True, True), 581: (12, 5, True, False)}
CASES = [(4, 226), (260, 226), (1024, 581), (1025, 6562), (8196, 226)]
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


def random_state(P, m, rng, ps_scale=1.0):
    """(mu, p_sigma, M, step): M standard normal rows (|M_j| ~ sqrt(P), the length the fast vectors reach), p_sigma standard normal
    times ps_scale (its natural length: |N(0, I)| ~ chi), step 1.37"""
    mu = (rng.randn(P) * 0.3).astype(np.float32)
    ps = (rng.randn(P) * ps_scale).astype(np.float32)
    M = rng.randn(m, P).astype(np.float32)
    return mu, ps, M, np.array([1.37], np.float32)


def make_params(c, step_limits=(1e-6, 1e6)):
    """a SesLmmaParams from the RESTATEMENT's constants and tables"""
    from ses import _lib
    p, tab = _lib.SesLmmaParams(), lm.tables(c)
    p.mu, p.m = c["mu"], c["m"]
    p.mueff, p.c_sigma, p.d_sigma, p.chi = c["mueff"], c["c_sigma"], c["d_sigma"], c["chi"]
    p.step_lo, p.step_hi = step_limits
    for k in ("cd", "ad", "ac", "bc"):
        for j in range(c["m"]):
            getattr(p, k)[j] = float(tab[k][j])
    return p


def check_dots(dots, M, vs, what, key):
    """device dots[rows, m_active] against the float64 dots of the restated vectors they were taken of"""
    worst = 0.0
    for j, v in enumerate(vs):
        ratio = np.abs(dots[:, j].astype(np.float64) - lm.dot_f64(M[j], v)) / lm.dot_tolerance(M[j], v)
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, f"{what}: dot {j}: row {int(ratio.argmax())} is {ratio.max():.3f} of the float64 bound away"
    print(f"{what}: worst |dot - dot64| / tol = {worst:.4f} over {len(vs)} vectors")
    WORST[key] = max(WORST.get(key, 0.0), worst)


@pytest.mark.parametrize("n,P", CASES, ids=IDS)
def test_perturb_lmma_against_float64_and_restatement(handles, n, P):
    es = handles(P)
    rng = np.random.RandomState(n + P)
    c, _ = lm.constants(n, P)
    m, tab, params = c["m"], lm.tables(c), make_params(c)
    mu, _, M, step = random_state(P, m, rng)
    gen = 2 ** 32 + 5 if n == 260 else 9
    plain = None
    for m_active in (0, 1, m):
        theta, dots = es.perturb_lmma(dev(mu), dev(M), dev(step), params, m_active, SIGMA, SEED, gen, 0, n, want_dots=True)
        theta, dots = host(theta), host(dots)
        assert dots.shape == (n, m_active)
        want, used, vs = lm.population(mu, M, step[0], SIGMA, SEED, gen, tab, m_active, 0, n, dots=dots, chain=True)
        check_dots(dots, M, vs, f"n={n} P={P} m_active={m_active}", ("dot", n, P))
        assert_bit_equal(theta, want, f"m_active={m_active}: whole population")
        assert not np.array_equal(theta[0], theta[1])
        if m_active == 0:
            plain = theta
            assert_bit_equal(theta, mu[None, :] + (np.float32(SIGMA) * step[0]) * cached_noise(SEED, gen, 0, n, P), "isotropic rows")
            assert not np.array_equal(theta, mu[None, :] + np.float32(SIGMA) * cached_noise(SEED, gen, 0, n, P))      # the step is in it
        else:
            assert not np.array_equal(theta, plain) and np.abs(dots).min() > 0
    for first in (0, 1, n - 3):
        for rows in (1, 2, 3):
            th, d = es.perturb_lmma(dev(mu), dev(M), dev(step), params, m, SIGMA, SEED, gen, first, rows, want_dots=True)
            assert_bit_equal(host(th), theta[first:first + rows], f"rows [{first}, +{rows})")
            assert_bit_equal(host(d), dots[first:first + rows], f"rows [{first}, +{rows}): dots")


def generation(es, fit, gen, state, c, weights, m_active, m_next, first_row, n_rows, step_limits=(1e-6, 1e6)):
    """ses_lmma_generation from copies of `state`: (state', theta_next, best, Sz, u_last, sdots, norm2, dots_next) on the host"""
    out = tuple(es.zeros(*x.shape) for x in state)
    best = es.zeros(1)
    theta, sz, sd, sdots, norm2, dots = es.lmma_generation(dev(fit), SEED, gen, SIGMA, make_params(c, step_limits), dev(weights),
                                                           m_active, m_next, tuple(dev(x) for x in state), out, NEXT_SIGMA, gen + 1,
                                                           first_row, n_rows, best=best, want_sums=True)
    es.sync()
    return (tuple(host(x) for x in out), host(theta), host(best)[0], host(sz), host(sd), host(sdots), float(host(norm2)[0]),
            host(dots))


def check_generation(res, state, fit, gen, c, weights, m_active, what, n, P, step_limits=(1e-6, 1e6)):
    """everything but theta_next: Sz and the chain's dots against float64, the new state against update() fed the device's numbers.
    Returns (the restatement's state with the DEVICE's step', info)."""
    out, _, best, sz, sd, sdots, norm2, _ = res
    tab = lm.tables(c)
    cs = sc.chunk_sums_f64(sc.row_weights(fit, weights), SEED, gen, P, noise=cached_noise)
    ratio = np.abs(sz.astype(np.float64) - cs["Sz"].sum(0)) / sc.sepcma_tolerance(n, "z", cs["Az"].sum(0))
    print(f"{what}: n={n} P={P} Sz worst |err|/tol = {ratio.max():.4f}")
    assert ratio.max() <= 1.0, f"{what}: Sz: parameter {int(ratio.argmax())} is {ratio.max():.3f} of the float64 bound away"
    WORST[("Sz", n, P)] = max(WORST.get(("Sz", n, P), 0.0), float(ratio.max()))
    assert norm2 == sc.norm2_device_order(out[1]), f"{what}: norm2 {norm2!r} vs {sc.norm2_device_order(out[1])!r}"
    want, info = lm.update(state[0], state[1], state[2], state[3][0], sz, sdots, norm2, SIGMA, c, tab, m_active, step_limits)
    assert sdots.shape == (m_active,)
    for j, u in enumerate(info["chain"]):
        err, tol = abs(float(sdots[j]) - float(lm.dot_f64(state[2][j], u))), lm.sdot_tolerance(state[2][j], u)
        assert err <= tol, f"{what}: mean chain dot {j}: {err / tol:.3f} of the float64 bound away"
        WORST[("sdot", n, P)] = max(WORST.get(("sdot", n, P), 0.0), err / tol)
    for name, got, wnt in zip(("mu", "p_sigma", "M"), out[:3], want[:3]):
        assert_bit_equal(got, wnt, f"{what}: {name}")
    assert_bit_equal(sd, info["u_last"], f"{what}: u_last")
    got_step = out[3]
    assert got_step.shape == (1,) and got_step.dtype == np.float32
    d = abs(int(bits(got_step)[0]) - int(bits(np.array([want[3]], np.float32))[0]))
    assert d <= 1, f"{what}: step' {got_step[0]!r} vs {want[3]!r}: {d} float32 steps apart"
    assert best == fit.max(), (best, fit.max())
    return want[:3] + (got_step,), info


@pytest.mark.parametrize("kind", ["perm", "cartpole"])
@pytest.mark.parametrize("n,P", CASES, ids=IDS)
def test_lmma_generation_against_float64_and_restatement(handles, n, P, kind):
    es = handles(P)
    rng = np.random.RandomState((n * 31 + P + len(kind)) % (2 ** 31))
    fit = fitness(kind, n, rng)
    gen = 11                                                            # (shared by the two kinds: one set of normals per shape)
    first = (n // 2) | 1 if n > 4 else 1                                # a shard in the middle of the population
    rows = min(n - first - 1, 301) if n > 4 else 2
    for mu_sel in (None, 1, n):
        c, weights = lm.constants(n, P, mu_sel)
        m, tab = c["m"], lm.tables(c)
        state = random_state(P, m, rng)
        # all vectors in use; a few, one more in the next population; none yet, the first in the next population
        m_active, m_next = {None: (m, m), 1: (3, 4), n: (0, 1)}[mu_sel]
        what = f"{kind} mu={c['mu']} m_active={m_active}"
        res = generation(es, fit, gen, state, c, weights, m_active, m_next, 0, n)
        new, info = check_generation(res, state, fit, gen, c, weights, m_active, what, n, P)
        theta, dots = res[1], res[7]
        assert dots.shape == (n, m_next)
        want, _, vs = lm.population(new[0], new[2], new[3][0], NEXT_SIGMA, SEED, gen + 1, tab, m_next, 0, n, dots=dots, chain=True)
        assert_bit_equal(theta, want, f"{what}: theta_next")
        if mu_sel is not None:
            check_dots(dots, new[2], vs, f"{what}: next population", ("dot", n, P))
            continue
        # a shard call: the same state, the matching slice; and no rows at all
        res2 = generation(es, fit, gen, state, c, weights, m_active, m_next, first, rows)
        for name, x, y in zip(("mu", "p_sigma", "M", "step", "Sz", "u_last", "sdots"), res2[0] + res2[3:6], res[0] + res[3:6]):
            assert_bit_equal(x, y, f"shard call: {name}")
        assert res2[2] == fit.max() and res2[6] == res[6]
        assert_bit_equal(res2[1], theta[first:first + rows], "shard call: theta_next")
        assert_bit_equal(res2[7], dots[first:first + rows], "shard call: dots of theta_next")
        res3 = generation(es, fit, gen, state, c, weights, m_active, m_next, 0, 0)
        assert res3[1].shape == (0, P) and res3[2] == fit.max() and res3[6] == res[6]
        for name, x, y in zip(("mu", "p_sigma", "M", "step"), res3[0], res[0]):
            assert_bit_equal(x, y, f"no rows: {name}")


def test_every_branch_of_the_update_is_taken(handles):
    """Each branch by construction of the input state, asserted from the restatement's record of the path it took (info) and held
    bit for bit on the device like every other case."""
    n, P, gen = 260, 226, 21
    es = handles(P)
    rng = np.random.RandomState(78)
    fit = fitness("perm", n, rng)
    c, weights = lm.constants(n, P)
    m, tab = c["m"], lm.tables(c)
    assert c["c_c"][0] == 1.0 and tab["ac"][0] == 0.0                    # n >= P: the first rate is capped

    def run(state, m_active, step_limits=(1e-6, 1e6)):
        res = generation(es, fit, gen, state, c, weights, m_active, min(m_active + 1, m), 0, 0, step_limits)
        return check_generation(res, state, fit, gen, c, weights, m_active, "branches", n, P, step_limits) + (res,)

    # a path of the natural length: the exponent uncapped, no limit binds; all vectors active
    state = random_state(P, m, rng)
    new, info, res = run(state, m)
    assert not info["capped"] and abs(info["exponent"]) < 0.5
    assert 1e-6 < new[3][0] < 1e6 and near(new[3][0], info["unclamped"]) and new[3][0] != state[3][0]
    assert len(info["chain"]) == m and np.abs(info["sdots"]).min() > 0
    # c_c[0] = 1: M'[0] = fl(bc[0] Sz) exactly, whatever M[0] was; the other vectors keep a share of themselves
    assert_bit_equal(new[2][0], tab["bc"][0] * res[3], "M'[0] = bc[0] Sz")
    assert not np.array_equal(new[2][1], tab["bc"][1] * res[3])
    # fewer vectors active than kept: the chain stops early, the mean moves differently, every vector is still updated
    new_few, info_few, _ = run(state, 2)
    assert len(info_few["chain"]) == 2 and not np.array_equal(new_few[0], new[0])
    assert_bit_equal(new_few[2], new[2], "M' does not depend on m_active")
    # a path ten times as long: the exponent is capped at 1
    long_state = state[:1] + (state[1] * np.float32(10.0),) + state[2:]
    new0, info0, _ = run(long_state, m)
    assert info0["capped"] and info0["exponent"] == 1.0
    assert near(new0[3][0], info0["unclamped"]) and 3.7 < new0[3][0] < 3.75      # 1.37 e
    # the same against step limits that bind: the capped rise against the upper, a vanishing path against the lower
    new_hi, info_hi, _ = run(long_state, m, (0.5, 2.0))
    assert info_hi["unclamped"] > 2.0 and new_hi[3][0] == np.float32(2.0)
    short_state = state[:1] + (np.zeros(P, np.float32),) + state[2:]
    # (p_sigma = 0: |p_sigma'|^2 = b_s^2 |Sz|^2 ~ P c_sigma (2 - c_sigma) = 0.41 P against chi^2 ~ P: the exponent is about -0.07)
    new_lo, info_lo, _ = run(short_state, m, (1.36, 2.0))
    assert not info_lo["capped"] and info_lo["exponent"] < -0.02 and info_lo["unclamped"] < 1.36
    assert new_lo[3][0] == np.float32(1.36)


@pytest.mark.parametrize("P", [226, 6562])
def test_generation_sequence_on_one_handle(handles, P):
    """Generations of changing size on ONE handle, with openai_es, pgpe and sep_cma_es generations in between that lay the handle's
    scratch out differently: every result against float64 and the restatement (a rank vector left uncleared would be counted twice)."""
    es = handles(P, "sequence")
    rng = np.random.RandomState(P)
    seq = [(4096, None), (4096, None), (260, None), (9000, "openai_es"), (4096, "pgpe"), (4096, "sep_cma_es"), (4, None),
           (8196, "pgpe"), (8196, None)]
    if P > 1024:
        seq = [(1025, None), (1025, "pgpe"), (260, "sep_cma_es"), (1025, "openai_es")]
    m = lm.default_memory(P)
    state = random_state(P, m, rng)
    for k, (n, between) in enumerate(seq):
        gen = 100 + k
        fit = fitness(("perm", "cartpole")[k % 2], n, rng)
        if between == "openai_es":
            junk = fitness("perm", (n * 3) // 4, rng)
            es.openai_generation(dev(junk), SEED, 1, 0.05, SIGMA, 1e-3, tuple(es.zeros(P) for _ in range(3)),
                                 tuple(es.zeros(P) for _ in range(3)), SIGMA, 2, 0, 1)
        elif between == "pgpe":
            junk = fitness("perm", n + n % 2, rng)                      # (pgpe wants an even population)
            es.pgpe_generation(dev(junk), SEED, 1, SIGMA, 1e-3, 0.2, 0.2, (0.01, 100.0), tuple(es.zeros(P) for _ in range(3)) +
                               (es.zeros(P) + 1.0,), tuple(es.zeros(P) for _ in range(4)), SIGMA, 2, 0, 2)
        elif between == "sep_cma_es":
            from ses import _lib
            junk = fitness("perm", n + 7, rng)
            cc, ww = sc.constants(n + 7, P)
            pp = _lib.SesSepcmaParams(cc["mu"], 0, cc["mueff"], cc["c_sigma"], cc["d_sigma"], cc["c_c"], cc["c_1"], cc["c_mu"], cc["chi"],
                                      0.01, 100.0, 1e-6, 1e6)
            es.sepcma_generation(dev(junk), SEED, 1, SIGMA, 1.0, pp, dev(ww), tuple(es.zeros(P) + 1.0 for _ in range(4)) + (es.zeros(1) + 1.0,),
                                 tuple(es.zeros(P) for _ in range(4)) + (es.zeros(1),), SIGMA, 2, 0, 2)
        c, weights = lm.constants(n, P)
        m_active, m_next = min(k, m), min(k + 1, m)
        first = (k * 997) % (n - 1) if k % 2 else 0
        rows = min(n - first, 64)
        res = generation(es, fit, gen, state, c, weights, m_active, m_next, first, rows)
        new, _ = check_generation(res, state, fit, gen, c, weights, m_active, f"sequence step {k} (n={n})", n, P)
        want, _ = lm.population(new[0], new[2], new[3][0], NEXT_SIGMA, SEED, gen + 1, lm.tables(c), m_next, first, rows, dots=res[7])
        assert_bit_equal(res[1], want, f"sequence step {k}: theta_next")
        state = res[0]


def test_front_end_rejects_bad_shapes(handles):
    from ses import SesError, _lib
    es = handles(226)
    P = 226
    c, w = lm.constants(8, P, m=5)
    params, weights = make_params(c), dev(w)

    def st(m=5):
        return es.zeros(P), es.zeros(P), es.zeros(m, P), es.zeros(1)

    ok, out = st(), st()
    args = (0.5, params, weights, 2, 3)
    es.lmma_generation(es.zeros(8), 0, 0, *args, ok, out, 0.5, 1, 0, 0)                          # the well-formed call
    for n in (3, 2, 0):
        with pytest.raises(SesError):
            es.lmma_generation(es.zeros(n), 0, 0, *args, ok, out, 0.5, 1, 0, 0)
    for mu in (0, 9, -1):
        with pytest.raises(SesError):
            es.lmma_generation(es.zeros(8), 0, 0, 0.5, make_params({**c, "mu": mu}), weights, 2, 3, ok, out, 0.5, 1, 0, 0)
    with pytest.raises(SesError):                                                               # a table shorter than mu
        es.lmma_generation(es.zeros(8), 0, 0, 0.5, params, weights[:3].contiguous(), 2, 3, ok, out, 0.5, 1, 0, 0)
    big = make_params(c)
    big.m = 33                                                                                  # more vectors than the tables hold
    with pytest.raises(SesError):
        es.lmma_generation(es.zeros(8), 0, 0, 0.5, big, weights, 2, 3, st(33), st(33), 0.5, 1, 0, 0)
    with pytest.raises(SesError):
        es.perturb_lmma(es.zeros(P), es.zeros(33, P), es.zeros(1), big, 2, 0.5, 0, 0, 0, 4)
    for m_active, m_next in ((6, 3), (2, 6), (-1, 0)):                                          # more active vectors than kept
        with pytest.raises(SesError):
            es.lmma_generation(es.zeros(8), 0, 0, 0.5, params, weights, m_active, m_next, ok, out, 0.5, 1, 0, 0)
    with pytest.raises(SesError):
        es.perturb_lmma(es.zeros(P), es.zeros(5, P), es.zeros(1), params, 6, 0.5, 0, 0, 0, 4)
    with pytest.raises(SesError):                                                               # aliased in and out
        es.lmma_generation(es.zeros(8), 0, 0, *args, ok, ok, 0.5, 1, 0, 0)
    with pytest.raises(SesError):
        es.lmma_generation(es.zeros(8), 0, 0, *args, ok, out[:2] + (ok[2], out[3]), 0.5, 1, 0, 0)
    with pytest.raises(SesError):
        es.lmma_generation(es.zeros(8), 0, 0, *args, ok, out[:3] + (ok[3],), 0.5, 1, 0, 0)
    with pytest.raises(SesError):                                                               # rows outside the population
        es.lmma_generation(es.zeros(8), 0, 0, *args, ok, out, 0.5, 1, 6, 3)
    for bad_M in (es.zeros(4, P), es.zeros(5, P + 1), es.zeros(5 * P)):                         # a wrong M shape
        with pytest.raises(SesError):
            es.lmma_generation(es.zeros(8), 0, 0, *args, ok[:2] + (bad_M, ok[3]), out, 0.5, 1, 0, 0)
        with pytest.raises(SesError):
            es.perturb_lmma(es.zeros(P), bad_M, es.zeros(1), params, 2, 0.5, 0, 0, 0, 4)
    with pytest.raises(SesError):
        es.lmma_generation(es.zeros(8), 0, 0, *args, ok[:1] + (es.zeros(P + 1),) + ok[2:], out, 0.5, 1, 0, 0)
    with pytest.raises(SesError):
        es.lmma_generation(es.zeros(8), 0, 0, *args, ok[:3] + (es.zeros(2),), out, 0.5, 1, 0, 0)
    with pytest.raises(SesError):
        es.perturb_lmma(es.zeros(225), es.zeros(5, P), es.zeros(1), params, 2, 0.5, 0, 0, 0, 4)
    with pytest.raises(SesError):
        es.perturb_lmma(es.zeros(P), es.zeros(5, P), es.zeros(P), params, 2, 0.5, 0, 0, 0, 4)
    with pytest.raises(SesError):
        es.perturb_lmma(es.zeros(P), es.zeros(5, P), es.zeros(1), params, 2, 0.5, 0, 0, 0, 0)
    # more parameters than a row's workgroup holds.  No network this library builds is that large (ses_create: at most 7656
    # parameters), so the front end is shown a handle that claims to be: the check answers before anything reaches the library
    assert _lib.LMMA_MAX_P == 16384
    es.P = _lib.LMMA_MAX_P + 4
    try:
        with pytest.raises(SesError, match="at most 16384"):
            es.perturb_lmma(es.zeros(es.P), es.zeros(5, es.P), es.zeros(1), params, 2, 0.5, 0, 0, 0, 4)
        with pytest.raises(SesError, match="at most 16384"):
            es.lmma_generation(es.zeros(8), 0, 0, *args, (es.zeros(es.P), es.zeros(es.P), es.zeros(5, es.P), es.zeros(1)),
                               (es.zeros(es.P), es.zeros(es.P), es.zeros(5, es.P), es.zeros(1)), 0.5, 1, 0, 0)
    finally:
        es.P = P
    # memory = 0 is a legal setting: no vectors at all
    c0, w0 = lm.constants(8, P, m=0)
    theta = es.lmma_generation(es.zeros(8), 0, 0, 0.5, make_params(c0), dev(w0), 0, 0, st(0), st(0), 0.5, 1, 0, 8)
    es.sync()
    assert theta.shape == (8, P) and bool(torch.isfinite(theta).all())


def small_cfg(memory=None):
    # (200 steps: see tests/test_gpu_sep_cma.py small_cfg -- a best that varies tells the generations apart)
    cfg = {"env": {"name": "CartPole-v1", "max_step": 200, "pomdp": False, "seed": 4},
           "network": {"name": "gym_model", "num_state": 4, "num_action": 2, "discrete_action": True, "gru": False},
           "strategy": {"name": "lm_ma_es", "init_sigma": 0.3, "sigma_decay": 0.98, "offspring_num": 64, "seed": 2}}
    if memory is not None:
        cfg["strategy"]["memory"] = memory
    return cfg


def strategy_state(s):
    return {"mu": host(s.mu_model), "p_sigma": host(s._ps), "M": host(s.directions), "step": host(s.step)}


@pytest.mark.parametrize("memory", [None, 2, 0])
def test_run_generations_equals_per_generation_calls(tmp_path, monkeypatch, memory):
    """ses_run_generations with SES_STRATEGY_LM_MA_ES, k = 3, against three ESLoop.generation calls: the state, theta, best[k]; the
    number of active vectors grows with the update counter in both forms (memory = 2: it stops growing inside the three)."""
    import builder
    from learning_strategies.evolution.loop import _GenerationBatch
    monkeypatch.chdir(tmp_path)
    with contextlib.redirect_stdout(io.StringIO()):
        a = builder.build_loop(small_cfg(memory), 3, 1, 2, False, 10 ** 9)
        b = builder.build_loop(small_cfg(memory), 3, 1, 2, False, 10 ** 9)
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
    want_m = 20 if memory is None else memory
    assert sb.memory == want_m and state["M"].shape == (want_m, 226)
    assert np.abs(state["mu"]).max() > 0 and state["step"][0] != 1.0 and (want_m == 0 or np.abs(state["M"]).min(axis=1).max() > 0)
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


def test_cartpole_lm_ma_config_end_to_end(tmp_path, monkeypatch):
    import builder
    monkeypatch.chdir(tmp_path)
    cfg = yaml.load(open(os.path.join(SRC, "conf", "cartpole_lm_ma.yaml")), Loader=yaml.FullLoader)
    loop = builder.build_loop(cfg, 40, 1, 5, False, 10 ** 9)
    with contextlib.redirect_stdout(io.StringIO()):
        pop = loop.run()
    best = [b for b, _ in loop.history]
    print("best per generation:", best)
    assert len(best) == 40 and max(best[-10:]) == 500 and min(best[-10:]) >= 400, best
    assert loop.batched_generations == 40                             # the run went through ses_run_generations
    s = loop.offspring_strategy
    M, step = host(s.directions), float(host(s.step)[0])
    norms = np.linalg.norm(M.astype(np.float64), axis=1)
    print("step:", step, "|M_j|:", np.round(norms, 2))
    assert step != 1.0 and 1e-6 <= step <= 1e6
    assert M.shape == (20, 226) and norms.max() > 0
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
