"""The float64 reference of the openai_es gradient and its error bound (oracle/strategies_np.py es_grad_f64), on the CPU.

tests/test_gpu_es_tail_f64.py holds the device's float32 gradient to |grad - g64| <= tol for every parameter.  This file checks,
without a GPU, that the bound is worth holding it to:
  * a float32 emulation of the device's summation order (4 fmas per thread, the 8-level LDS tree, the ordered chunk sum, the
    float32 factor) stays inside tol -- by a wide margin;
  * each of the mistakes a kernel could make below -- a row too few or too many, a chunk lost or counted twice, the noise of the
    wrong generation or quad, the wrong tie rule -- moves the float64 sum by more than tol on at least half of the parameters the
    mistake touches.
"""
import functools

import numpy as np
import pytest

from oracle import c_oracle as co
from oracle import strategies_np as snp

LR, SIGMA, SEED, GEN = 0.05, 0.1, 1234, 17
SIZES = [(4096, 226), (65537, 226), (8193, 6562)]


def tie_heavy(n, rng):
    """CartPole-like returns: most rows a small integer, the rest one of a few saturated values."""
    fit = rng.randint(0, 60, n).astype(np.float32)
    sat = rng.rand(n) < 0.5
    fit[sat] = rng.choice(np.array([500.0, 137.2, 10.0, 9.8], np.float32), int(sat.sum()))
    return fit


def centered_from_order(order):
    """centered_ranks' arithmetic for a given rank order (order[k] = row of rank k)."""
    n = len(order)
    r = np.zeros(n)
    for idx in reversed(range(n)):
        r[order[idx]] = ((n - 1 - idx) / (n - 1)) - 0.5
    return (r - r.mean()) / r.std()


@functools.lru_cache(maxsize=None)
def base(n, P):
    """Tie-free fitness: weights, per-chunk float64 sums, g64 and tol (es_grad_f64's quantities, kept per chunk)."""
    rng = np.random.RandomState(n + P)
    fit = rng.permutation(n).astype(np.float32)
    w = snp.centered_ranks(fit, stable=True)
    S, A, Z = snp.es_chunk_sums_f64(w, SEED, GEN, P)
    uf = -(LR / (n * SIGMA))
    s_abs = abs(uf) * A.sum(0)
    tol = snp.es_grad_tolerance(n, uf, s_abs, Z.sum(0))
    return fit, w, S, uf, uf * S.sum(0), tol


def detected(g_wrong, g64, tol):
    return float(np.mean(np.abs(g_wrong - g64) > tol))


def test_es_grad_f64_matches_its_parts():
    n, P = 3000, 226
    fit, w, S, uf, g64, tol = base(n, P)
    g, s_abs, tol2 = snp.es_grad_f64(fit, SEED, GEN, P, LR, SIGMA)
    z = co.noise(SEED, GEN, 0, n, P).astype(np.float64)
    z[0] = 0.0
    np.testing.assert_allclose(g, uf * (w @ z), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(s_abs, abs(uf) * (np.abs(w) @ np.abs(z)), rtol=1e-12)
    assert np.array_equal(g, g64) and np.array_equal(tol2, tol)
    K = snp.es_grad_rounding_count(n)
    assert K == 4 + 8 + 3 + 3
    assert np.all(tol > K * 2.0 ** -24 * s_abs) and np.all(tol < 1.001 * K * 2.0 ** -24 * s_abs + 1e-9)


def emulate_device(w, seed, gen, P, uf):
    """float32 gradient in the device's order: k_es_grad_partial (fma chains over rows c, c + 256, ..., LDS tree over 256
    threads) then k_es_apply (chunk partials added in ascending order, times float(uf)).  The fma is emulated in float64
    (the product is exact there; the double rounding it may add is far below what is measured here)."""
    n = len(w)
    wf = w.astype(np.float32).astype(np.float64)
    wf[0] = 0.0                                                      # skip_row0: fma(0, z, acc) == acc
    total = None
    for c in range(-(-n // snp.ES_CHUNK)):
        r0, r1 = c * snp.ES_CHUNK, min(n, (c + 1) * snp.ES_CHUNK)
        z = np.zeros((snp.ES_CHUNK, P))
        z[: r1 - r0] = co.noise(seed, gen, r0, r1 - r0, P)
        wc = np.zeros(snp.ES_CHUNK)
        wc[: r1 - r0] = wf[r0:r1]
        z = z.reshape(4, 256, P)
        wc = wc.reshape(4, 256, 1)
        acc = np.zeros((256, P), np.float32)
        for k in range(4):
            acc = (wc[k] * z[k] + acc.astype(np.float64)).astype(np.float32)
        s = 128
        while s:
            acc[:s] = acc[:s] + acc[s:2 * s]
            s >>= 1
        total = acc[0] if total is None else total + acc[0]
    return total * np.float32(uf)


@pytest.mark.parametrize("n,P", SIZES)
def test_device_order_emulation_stays_inside_the_bound(n, P):
    fit, w, S, uf, g64, tol = base(n, P)
    g = emulate_device(w, SEED, GEN, P, uf).astype(np.float64)
    ratio = np.abs(g - g64) / tol
    print(f"n={n} P={P}: emulated float32 device order, worst |err|/tol = {ratio.max():.4f}, median {np.median(ratio):.4f}")
    assert ratio.max() <= 1.0
    # and the bound is not vacuous: the rounding error it covers is real
    assert ratio.max() > 1e-4


def row_term(w, i, P, gen=GEN):
    return w[i] * co.noise(SEED, gen, i, 1, P)[0].astype(np.float64)


MUTATIONS = ["last_row_dropped", "row0_included", "chunk_dropped", "chunk_twice", "gen_minus_1", "last_quad_from_next_quad",
             "ties_index_ascending"]


def mutated(kind, n, P):
    """(float64 gradient a kernel with the mistake would compute, g64, tol, mask of the parameters the mistake touches)"""
    fit, w, S, uf, g64, tol = base(n, P)
    every = np.ones(P, bool)
    chunks = S.shape[0]
    # a single row is seen in proportion to its weight |w_i| (a row ranked near the median weighs ~0 and is invisible to any
    # bound); measured with these fitness vectors: >= 0.99 of the parameters at n = 4096 and 8193, 0.88 at n = 65 537
    if kind == "last_row_dropped":
        return g64 - uf * row_term(w, n - 1, P), g64, tol, every
    if kind == "row0_included":
        return g64 + uf * row_term(w, 0, P), g64, tol, every
    if kind == "chunk_dropped":
        return g64 - uf * S[chunks // 2], g64, tol, every
    if kind == "chunk_twice":
        return g64 + uf * S[chunks // 2], g64, tol, every
    if kind == "gen_minus_1":
        S1, _, _ = snp.es_chunk_sums_f64(w, SEED, GEN - 1, P)
        return uf * S1.sum(0), g64, tol, every
    if kind == "last_quad_from_next_quad":
        # the parameters of the last quad q get the normals of quad q + 1
        q = (P + 3) // 4 - 1
        lim = P - 4 * q
        S2, _, _ = snp.es_chunk_sums_f64(w, SEED, GEN, lim,
                                         noise=lambda s, g, r0, rows, _P: co.noise(s, g, r0, rows, 4 * q + 8)[:, 4 * q + 4: 4 * q + 4 + lim])
        got = g64.copy()
        got[4 * q:] = uf * S2.sum(0)
        mask = np.zeros(P, bool)
        mask[4 * q:] = True
        return got, g64, tol, mask
    if kind == "ties_index_ascending":
        # the tie-heavy fitness: rank by return descending, then index ASCENDING instead of descending
        tfit = tie_heavy(n, np.random.RandomState(n * 7 + P))
        g, s_abs, ttol = snp.es_grad_f64(tfit, SEED, GEN, P, LR, SIGMA)
        w_desc = snp.centered_ranks(tfit, stable=True)
        w_asc = centered_from_order(np.lexsort((np.arange(n), -tfit.astype(np.float64))))
        assert not np.array_equal(w_asc, w_desc)
        D, _, _ = snp.es_chunk_sums_f64(w_asc - w_desc, SEED, GEN, P)
        return g + uf * D.sum(0), g, ttol, every
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", MUTATIONS)
@pytest.mark.parametrize("n,P", SIZES)
def test_bound_detects_mutation(n, P, kind):
    g_wrong, g64, tol, mask = mutated(kind, n, P)
    frac = detected(g_wrong[mask], g64[mask], tol[mask])
    print(f"n={n} P={P} {kind}: |g_wrong - g64| > tol on {frac:.3f} of {int(mask.sum())} parameters")
    assert frac >= 0.5
