"""The openai_es tail against float64 at production sizes (oracle/strategies_np.py es_grad_f64).

Every form of the tail -- the stepwise rank_center + es_update_philox, and ses_openai_generation with Adam applied by the
gradient kernel's last workgroup (es_final_max_chunks), inside the perturbation launch (k_es_apply_perturb) or by a separate
k_es_apply launch -- is held to the float64 gradient of the same fitness and noise, parameter by parameter, within the bound
es_grad_f64 derives from the device's summation order (|grad - g64| <= tol; tests/test_es_grad_bound.py shows the bound
catches a single wrong row).  Beyond the gradient:
  * Adam: mu / m / v bit-equal to snp.AdamNP fed the device gradient, from random moments at t >= 2;
  * the fused forms: bit-equal to the stepwise result, theta_next bit-equal to the C oracle's perturbation of the new mu;
  * handle state: one handle runs a sequence of generations of changing size and finishing form with stepwise calls in
    between (rank_zeroed / counter_armed: scratch the previous call is assumed to have left cleared).
Sizes reach past 64 gradient chunks (n > 65 536: the second pass of k_es_apply's readlane loop) and the GRU policies
(P > 1024: no k_es_apply_perturb).
"""
import numpy as np
import pytest
import torch

from oracle import c_oracle as co
from oracle import strategies_np as snp

pytestmark = pytest.mark.gpu

LR, SIGMA, SEED, DECAY = 0.05, 0.1, 20240611, 0.999
SHAPES = {226: (4, 2, True, False), 6562: (4, 2, True, True), 581: (12, 5, True, False), 932: (24, 4, False, False),
          6756: (8, 4, False, True)}
THETA_FLOATS = 1 << 22                     # rows of theta_next compared per call: at most this many floats
OMB1 = np.float32(1.0 - 0.99)
WORST = {}                                 # (n, P) -> worst |err| / tol, printed at the end of the module


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
        print("\nworst |grad - g64| / tol per (n, P):")
        for (n, P), r in sorted(WORST.items()):
            print(f"  n={n:>6} P={P:>4}: {r:.4f}")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def assert_bit_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    assert not bad.any(), f"{what}: {bad.sum()} of {bad.size} differ, first at {np.argwhere(bad)[0]}: " \
                          f"{got[tuple(np.argwhere(bad)[0])]!r} vs {want[tuple(np.argwhere(bad)[0])]!r}"


def fitness(kind, n, rng):
    if kind == "perm":                                              # tie-free
        return rng.permutation(n).astype(np.float32) * 0.25 - 7.0
    if kind == "cartpole":                                          # tie-heavy: small integer returns and saturated ones
        fit = rng.randint(0, 60, n).astype(np.float32)
        sat = rng.rand(n) < 0.5
        fit[sat] = rng.choice(np.array([500.0, 137.2, 10.0, 9.8], np.float32), int(sat.sum()))
        return fit
    if kind == "equal":
        return np.full(n, 3.5, np.float32)
    if kind == "neginf":
        fit = rng.permutation(n).astype(np.float32)
        fit[rng.randint(n)] = -np.inf
        return fit
    raise AssertionError(kind)


def adam_state(P, rng):
    """random (mu, m, v) and the step t >= 2 they are the state after; adam_a of step t + 1"""
    mu = (rng.randn(P) * 0.3).astype(np.float32)
    m = (rng.randn(P) * 1e-3).astype(np.float32)
    v = (rng.rand(P) * 1e-5).astype(np.float32)
    t = int(rng.randint(2, 40))
    adam = snp.AdamNP(mu.copy(), LR)
    adam.t = t + 1
    return mu, m, v, t, adam.step_scale()


def adam_expect(mu, m, v, t, grad):
    adam = snp.AdamNP(mu.copy(), LR)
    adam.m, adam.v, adam.t = m.copy(), v.copy(), t
    adam.update(grad)
    return adam.theta, adam.m, adam.v


def check_grad(grad, g64, tol, n, P, what):
    ratio = np.abs(grad.astype(np.float64) - g64) / tol
    worst = float(ratio.max())
    WORST[(n, P)] = max(WORST.get((n, P), 0.0), worst)
    print(f"{what}: n={n} P={P} worst |err|/tol = {worst:.4f} (median {np.median(ratio):.4f})")
    bad = ~(ratio <= 1.0)
    assert not bad.any(), f"{what}: {bad.sum()} of {P} parameters outside the float64 bound, worst p={int(ratio.argmax())} " \
                          f"ratio {worst:.3f}: grad {grad[ratio.argmax()]!r} vs g64 {g64[ratio.argmax()]!r} +- {tol[ratio.argmax()]!r}"


def stepwise(es, fit, gen, state, g64, tol, what):
    """rank_center + es_update_philox on copies of `state`: gradient within the bound, Adam bit-exact, best = max(fitness).
    Returns (mu, m, v) after the update and the device gradient."""
    n = len(fit)
    mu0, m0, v0, t, a = state
    best = es.zeros(1)
    rank, w = es.rank_center(dev(fit), best=best)
    np.testing.assert_allclose(host(w), snp.centered_ranks(fit, stable=True), rtol=0, atol=snp.WEIGHT_ATOL)
    mu, m, v = dev(mu0), dev(m0), dev(v0)
    grad = host(es.es_update_philox(w, SEED, gen, LR, SIGMA, a, mu, m, v, skip_row0=True, want_grad=True))
    check_grad(grad, g64, tol, n, es.P, what)
    want = adam_expect(mu0, m0, v0, t, grad)
    for name, got, wnt in zip(("mu", "m", "v"), (mu, m, v), want):
        assert_bit_equal(host(got), wnt, f"{what}: {name}")
    assert host(best)[0] == fit.max(), (host(best)[0], fit.max())
    return tuple(host(x) for x in (mu, m, v)), grad


def fused(es, fit, gen, state, first_row, n_rows, final=None, apply_perturb=None):
    """ses_openai_generation from copies of `state`: (mu, m, v)_out, theta_next, best"""
    mu0, m0, v0, t, a = state
    if final is not None:
        es.set_tuning("es_final_max_chunks", final)
    if apply_perturb is not None:
        es.set_tuning("fused_apply_perturb", apply_perturb)
    try:
        out = (es.zeros(es.P), es.zeros(es.P), es.zeros(es.P))
        best = es.zeros(1)
        theta = es.openai_generation(dev(fit), SEED, gen, LR, SIGMA, a, (dev(mu0), dev(m0), dev(v0)), out,
                                     np.float32(SIGMA * DECAY), gen + 1, first_row, n_rows, best=best)
        es.sync()
    finally:                                                        # back to the handle's defaults
        es.set_tuning("es_final_max_chunks", 0)
        es.set_tuning("fused_apply_perturb", 1)
    return tuple(host(x) for x in out), host(theta), host(best)[0]


def check_theta(theta, mu_out, gen, first_row, n_rows, what):
    want = co.perturb(mu_out[None], None, np.float32(SIGMA * DECAY), SEED, gen + 1, first_row, n_rows)
    if first_row == 0 and n_rows > 0:
        want[0] = mu_out                                            # row 0 of an openai_es population is mu itself
    assert_bit_equal(theta, want, what)


# n over the chunk edges (1024), the counting / sort rank switch (8192), the 64-chunk pass of the readlane loop (65 536) and
# past two of them (131 077 = 129 chunks); fitness kinds spread over the cases; one generation beyond 32 bits
CASES = []
for i, n in enumerate([2, 3, 1023, 1024, 1025, 4096, 8192, 8193, 16384, 16385, 65536, 65537, 131077]):
    for j, P in enumerate((226, 6562)):
        kind = ("perm", "cartpole", "equal", "neginf")[(i + j) % 4]
        gen = 2 ** 32 + 3 if (n, P) == (65537, 226) else 5 + i
        CASES.append((n, P, kind, gen))
for P, kinds in ((581, ("perm", "cartpole", "neginf")), (932, ("cartpole", "equal", "perm")), (6756, ("neginf", "perm", "cartpole"))):
    for n, kind in zip((1025, 4096, 8193), kinds):
        CASES.append((n, P, kind, 11))


@pytest.mark.parametrize("n,P,kind,gen", CASES, ids=[f"n{n}-P{P}-{k}" for n, P, k, _ in CASES])
def test_openai_tail_against_float64(handles, n, P, kind, gen):
    es = handles(P)
    rng = np.random.RandomState((n * 31 + P) % (2 ** 31))
    fit = fitness(kind, n, rng)
    state = adam_state(P, rng)
    g64, s_abs, tol = snp.es_grad_f64(fit, SEED, gen, P, LR, SIGMA)
    (mu1, m1, v1), grad = stepwise(es, fit, gen, state, g64, tol, f"stepwise {kind}")
    rows = max(1, THETA_FLOATS // P)
    # default knobs (P <= 1024 and <= 16 chunks: k_es_apply_perturb; otherwise k_es_apply), rows from 0
    n_rows = min(n, rows)
    out, theta, best = fused(es, fit, gen, state, 0, n_rows)
    for name, got, want in zip(("mu", "m", "v"), out, (mu1, m1, v1)):
        assert_bit_equal(got, want, f"fused default: {name}")
    assert best == fit.max()
    check_theta(theta, out[0], gen, 0, n_rows, "fused default: theta_next")
    # Adam by the gradient kernel's last workgroup, a slice of rows that starts past row 0
    first = n // 2 + 1 if n > 2 else 1
    n_rows = min(n - first, rows)
    out, theta, best = fused(es, fit, gen, state, first, n_rows, final=1 << 20)
    for name, got, want in zip(("mu", "m", "v"), out, (mu1, m1, v1)):
        assert_bit_equal(got, want, f"fused final-in-gradient: {name}")
    assert best == fit.max()
    check_theta(theta, out[0], gen, first, n_rows, "fused final-in-gradient: theta_next")
    # separate k_es_apply launch, no rows; from m = 0, so that m_out is omb1 * grad and can be held to g64 directly
    mu0, _, v0, t, a = state
    zero_m = (mu0, np.zeros(P, np.float32), v0, t, a)
    out, theta, best = fused(es, fit, gen, zero_m, 0, 0, apply_perturb=0)
    assert theta.shape == (0, P)
    for name, got, want in zip(("mu", "m", "v"), out, adam_expect(mu0, zero_m[1], v0, t, grad)):
        assert_bit_equal(got, want, f"fused k_es_apply from m = 0: {name}")
    assert best == fit.max()
    m_out = out[1].astype(np.float64)
    err = np.abs(m_out - float(OMB1) * g64)
    allowed = float(OMB1) * tol + np.spacing(np.abs(out[1])).astype(np.float64)
    assert np.all(err <= allowed), f"m_out vs omb1 * g64: worst {np.max(err / allowed):.3f} of the allowance"


def test_noise_rows_and_generations_past_32_bits(handles):
    """es.noise at rows >= 65 536 and a generation >= 2^32 against the C oracle, bit for bit: a truncated row or generation
    counter would give other normals (and a gradient the float64 check above would also reject)."""
    for P in (226, 6562):
        es = handles(P)
        for gen, first in ((2 ** 32 + 3, 65536), (7, 131070), (2 ** 40 + 9, 70001)):
            got = host(es.noise(SEED, gen, first, 9))
            assert_bit_equal(got, co.noise(SEED, gen, first, 9, P), f"noise P={P} gen={gen} first={first}")
        assert not np.array_equal(co.noise(SEED, 2 ** 32 + 3, 65536, 2, P), co.noise(SEED, 3, 65536, 2, P))
        assert not np.array_equal(co.noise(SEED, 7, 65536 + 5, 2, P), co.noise(SEED, 7, 5, 2, P))


# (n, es_final_max_chunks, fused_apply_perturb, stepwise call on the same handle before it: None or its n)
SEQ_226 = [(4096, 0, 1, None), (9000, 0, 1, None), (4096, 1 << 20, 1, None), (4096, 1 << 20, 1, None), (4096, 0, 1, 3000),
           (1025, 0, 0, None), (65537, 0, 1, None), (4096, 1 << 20, 1, None), (4096, 0, 1, 20000), (1025, 1 << 20, 0, None),
           (1025, 0, 1, None)]
SEQ_6562 = [(4096, 0, 1, None), (1025, 1 << 20, 1, None), (4096, 1 << 20, 1, None), (4096, 0, 1, 700), (9000, 1 << 20, 1, None),
            (4096, 0, 1, None)]


@pytest.mark.parametrize("P,seq", [(226, SEQ_226), (6562, SEQ_6562)], ids=["P226", "P6562"])
def test_generation_sequence_on_one_handle(handles, P, seq):
    """Generations of changing size and finishing form on ONE handle, each from the previous one's output, with stepwise calls
    in between that lay the handle's scratch out differently.  Every generation is checked on its own: against the float64
    gradient (through a stepwise update on a second handle, which also gives the bits the fused result must equal) and its
    theta_next against the C oracle."""
    es = handles(P, "sequence")
    ref = handles(P)
    rng = np.random.RandomState(P)
    mu, m, v, t, _ = adam_state(P, rng)
    for k, (n, final, apply_perturb, between) in enumerate(seq):
        gen = 100 + k
        fit = fitness(("perm", "cartpole", "neginf")[k % 3], n, rng)
        adam = snp.AdamNP(mu.copy(), LR)
        adam.t = t + 1
        state = (mu, m, v, t, adam.step_scale())
        g64, _, tol = snp.es_grad_f64(fit, SEED, gen, P, LR, SIGMA)
        want, _ = stepwise(ref, fit, gen, state, g64, tol, f"sequence step {k} (reference handle)")
        if between is not None:                                     # re-lays es's scratch: rank vector and counters move
            junk = fitness("perm", between, rng)
            _, w = es.rank_center(dev(junk))
            es.es_update_philox(w, SEED, 1, LR, SIGMA, 1e-3, es.zeros(P), es.zeros(P), es.zeros(P))
        first = (k * 997) % n if k % 2 else 0
        n_rows = min(n - first, max(1, THETA_FLOATS // P))
        out, theta, best = fused(es, fit, gen, state, first, n_rows, final=final, apply_perturb=apply_perturb)
        for name, got, wnt in zip(("mu", "m", "v"), out, want):
            assert_bit_equal(got, wnt, f"sequence step {k} (n={n}, final={final}, apply_perturb={apply_perturb}): {name}")
        assert best == fit.max()
        check_theta(theta, out[0], gen, first, n_rows, f"sequence step {k}: theta_next")
        mu, m, v = out
        t += 1
