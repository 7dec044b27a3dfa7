"""The shared front end of the ranked tails (csrc/ses_tail.h: tail_rank_begin / tail_rank_cleared) and the handle's "this rank vector
is known to be zero" cache, across the four tails that use that cache -- openai_es, pgpe, sep_cma_es, lm_ma_es -- on ONE handle.

Every step of a ring of generations runs twice: on a shared handle that has run all the steps before it (other tails, other
population sizes, both rank paths) and on a fresh handle that has seen nothing else.  The output state vectors, theta_next and best
are compared BIT FOR BIT: both sides are the code under test at different cache states, and the kernels are order-deterministic for
a given n, so no tolerance is involved.  A rank vector counted twice, or left uncleared by the front end, changes the sums.

The population sizes 4, 260, 8192, 8193, 260, 8194, 4 cross the count / sort boundary (8192 rows) in both directions.  At P = 226
all their layouts fit the scratch's first allocation (1 MiB), so the ring ends with a step of 80 000 rows, whose sorted tiles and
ranks need more -- the scratch moves, which must drop the cache -- and one more step of 260 rows behind it.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P, SHAPE = 226, (4, 2, True, False)
SEED, SIGMA, NEXT_SIGMA = 20241018, 0.5, 0.4995
TAILS = ("openai_es", "pgpe", "sep_cma_es", "lm_ma_es")
SIZES = (4, 260, 8192, 8193, 260, 8194, 4)            # (8194: even, it is pgpe's turn)
GROW = (80000, 260)
MEMORY = 2


def fitness(k, n, rng):
    """alternating: a random permutation (tie-free), and heavy ties -- 16 multiples of 0.2, capped at 2.4"""
    if k % 2 == 0:
        return rng.permutation(n).astype(np.float32) * 0.25 - 7.0
    return np.minimum(rng.randint(0, 16, n).astype(np.float32) * np.float32(0.2), np.float32(2.4))


def vectors(tail, rng):
    """the input state of one generation, as host arrays"""
    mu = (rng.randn(P) * 0.3).astype(np.float32)
    pos = lambda: (0.5 + rng.rand(P)).astype(np.float32)              # noqa: E731  (scale, C: positive, near 1)
    step = np.array([1.37], np.float32)
    if tail == "openai_es":
        return mu, (rng.randn(P) * 0.01).astype(np.float32), (rng.rand(P) * 1e-4).astype(np.float32)
    if tail == "pgpe":
        return mu, (rng.randn(P) * 0.01).astype(np.float32), (rng.rand(P) * 1e-4).astype(np.float32), pos()
    if tail == "sep_cma_es":
        return mu, pos(), rng.randn(P).astype(np.float32), rng.randn(P).astype(np.float32), step
    return mu, rng.randn(P).astype(np.float32), rng.randn(MEMORY, P).astype(np.float32), step


def run_tail(es, tail, fit, state_in, gen, k, first_row, n_rows):
    """one generation of `tail` on handle `es`; returns host copies of (every output state vector ..., theta_next, best)"""
    from learning_strategies.evolution.offspring_strategies import lm_ma_constants, lm_ma_params, sep_cma_constants
    from ses import _lib
    n = fit.shape[0]
    out = tuple(torch.empty_like(x) for x in state_in)
    best = es.zeros(1)
    rows = dict(best=best)
    if tail == "openai_es":
        theta = es.openai_generation(fit, SEED, gen, 0.05, SIGMA, 1e-3, state_in, out, NEXT_SIGMA, gen + 1, first_row, n_rows, **rows)
    elif tail == "pgpe":
        theta = es.pgpe_generation(fit, SEED, gen, SIGMA, 1e-3, 0.2, 0.2, (0.01, 100.0), state_in, out, NEXT_SIGMA, gen + 1,
                                   first_row, n_rows, **rows)
    elif tail == "sep_cma_es":
        c, w = sep_cma_constants(n, P, n // 2)
        params = _lib.SesSepcmaParams(c["mu"], 0, c["mueff"], c["c_sigma"], c["d_sigma"], c["c_c"], c["c_1"], c["c_mu"], c["chi"],
                                      0.01, 100.0, 1e-6, 1e6)
        theta = es.sepcma_generation(fit, SEED, gen, SIGMA, 1.25, params, torch.from_numpy(w).cuda(), state_in, out, NEXT_SIGMA,
                                     gen + 1, first_row, n_rows, **rows)
    else:
        c, w = lm_ma_constants(n, P, n // 2, MEMORY)
        theta = es.lmma_generation(fit, SEED, gen, SIGMA, lm_ma_params(c, (1e-6, 1e6)), torch.from_numpy(w).cuda(), min(k, MEMORY),
                                   min(k + 1, MEMORY), state_in, out, NEXT_SIGMA, gen + 1, first_row, n_rows, **rows)
    return [x.cpu().numpy() for x in out] + [theta.cpu().numpy(), best.cpu().numpy()]


def test_shared_handle_equals_fresh_handles():
    from ses import HipES
    rng = np.random.RandomState(226)
    # twice round the sizes, the tails one further on the second lap: both laps give pgpe (steps 1 and 5; 0, 4) even populations
    steps = [(n, TAILS[(k + lap) % 4]) for lap in (0, 1) for k, n in enumerate(SIZES)]
    steps += [(GROW[0], "lm_ma_es"), (GROW[1], "sep_cma_es")]
    shared = HipES(None, *SHAPE)
    assert shared.P == P
    try:
        for k, (n, tail) in enumerate(steps):
            fit = torch.from_numpy(fitness(k, n, rng)).cuda()
            state_in = tuple(torch.from_numpy(x).cuda() for x in vectors(tail, rng))
            n_rows = min(n, 64)
            first_row = ((n - n_rows) // 2) | 1 if n > n_rows else 0        # odd where n allows: a pgpe shard that splits pairs
            got = run_tail(shared, tail, fit, state_in, 100 + k, k, first_row, n_rows)
            fresh = HipES(None, *SHAPE)
            try:
                want = run_tail(fresh, tail, fit, state_in, 100 + k, k, first_row, n_rows)
            finally:
                fresh.close()
            names = [f"state_out[{i}]" for i in range(len(state_in))] + ["theta_next", "best"]
            for name, a, b in zip(names, got, want):
                assert a.shape == b.shape and a.dtype == b.dtype == np.float32, (k, tail, n, name)
                bad = a.view(np.uint32) != b.view(np.uint32)
                assert not bad.any(), (f"step {k} ({tail}, n = {n}, rows [{first_row}, +{n_rows})): {name} of the shared handle differs "
                                       f"from a fresh handle's in {int(bad.sum())} of {bad.size} values")
            assert np.isfinite(got[-2]).all() and got[-1][0] == fit.max().item(), (k, tail, n)
    finally:
        shared.close()
