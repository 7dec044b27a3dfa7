"""The simple_evolution / simple_genetic tail of R ragged trials as one set of launches (ses_elite_generation_batch,
csrc/ses_batch_elite.hip), the host layer that advances such runs in lockstep (learning_strategies/evolution/batch.py) and the
sweep driver's --concurrent for them.

The yardstick throughout is the existing solo path on the same device -- rank_center -> elite_select -> perturb(row_ids, parent_idx)
-> [elite_mean] -> perturb on a trial's slice, builder.build_loop(...).run() for a whole run, sweep_main.py --concurrent 1 for a
sweep -- never the batch code itself, and every comparison is for equal bits: a trial in a batch computes what it computes alone.
"""
import copy
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "simple-es_amd", "conf")

EVOLUTION, GENETIC = 1, 2                      # _lib.STRATEGY_SIMPLE_EVOLUTION, _lib.STRATEGY_SIMPLE_GENETIC

HANDLES = {
    226: lambda HipES: HipES(None, 4, 2, True, False),       # CartPole MLP: a ragged last quad
    6562: lambda HipES: HipES(None, 4, 2, True, True),       # CartPole POMDP GRU
}


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def assert_bit_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}"
    width = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    diff = np.flatnonzero(got.view(width).ravel() != want.view(width).ravel())
    assert diff.size == 0, f"{what}: {diff.size} of {got.size} values differ, first at {diff[0]}"


# ---- a few lines of numpy: the ids, flags and aliasing state the handcrafted fitness vectors lead to -------------------------------

def np_order(fit):
    """rows best first: key = (ordered fitness bits, index), -0 as +0, so a tie goes to the higher index"""
    u = np.ascontiguousarray(fit, np.float32).view(np.uint32).astype(np.uint64)
    u[u == 0x80000000] = 0
    ordered = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return np.argsort((ordered << np.uint64(32)) | np.arange(len(fit), dtype=np.uint64))[::-1]


def np_select(fit, k, state):
    """(ids[k], flags[k], the new aliasing state) of simple_evolution (include/ses.h: ses_elite_select)"""
    ids = np_order(fit)[:k]
    first = int(ids[0])
    flags = [int(j > 0 and state != 0 and first in (0, 1) and int(i) in (0, 1) and int(i) != first) for j, i in enumerate(ids)]
    return ids, flags, int(first == 0 or (first == 1 and state != 0))


def crafted(n, top, shift=0):
    """n distinct low values (-10 - a permutation of 0 .. n-1), then the rows of `top` = {row: value} set by hand"""
    step = 5 if n % 5 else 3
    assert math.gcd(step, n) == 1
    fit = np.array([-10.0 - ((i * step + shift) % n) for i in range(n)], np.float32)
    for row, value in top.items():
        fit[row] = value
    return fit


def tie_straddles(fit, k):
    order = np_order(fit)
    return k < len(fit) and fit[order[k - 1]] == fit[order[k]]           # (-0.0 == 0.0 in numpy too)


def has_signed_zero_pair(fit):
    zeros = fit[fit == 0]
    return bool(np.signbit(zeros).any() and (~np.signbit(zeros)).any())


# trial -> generation -> the rows set by hand; n = 13 (N = 12), elite_num (1, 4, 13)
EVOLUTION_K = (1, 4, 13)
EVOLUTION_TOPS = [
    [{0: 5.0}, {i: 1.25 for i in range(13)}, {3: -0.0, 8: 0.0}, {1: 2.0}],
    [{0: 9.0, 1: 8.0, 5: 7.0, 6: 3.0, 9: 3.0}, {1: 9.0, 3: 8.0, 0: 0.0, 4: -0.0}, {5: 9.0, 0: 8.0, 1: 7.0, 2: 6.0},
     {0: 9.0, 1: 8.0, 2: 7.0, 3: 6.0}],
    [{7: 9.0}, {1: 9.0}, {0: 9.0}, {1: 9.0}],
]
# n = 12, 12, 13, 13 (N = 13), elite_num (2, 3, 13, 1): the third trial is all elites, no children
GENETIC_K = (2, 3, 13, 1)
GENETIC_TOPS = [
    [{4: 3.0, 7: 2.0, 9: 2.0}, {0: 1.0, 6: 1.0, 11: 1.0}, {11: 4.0, 0: 3.5}, {5: 0.0, 2: -0.0, 8: -0.0}],
    [{0: 7.0, 1: 6.0, 2: 5.0}, {3: 0.0, 10: -0.0, 5: 0.0, 7: 1.0}, {6: 2.0, 7: 2.0, 8: 2.0, 9: 2.0}, {1: 1.0, 2: 1.5, 3: 1.25}],
    [{12: 1.0}, {0: -0.0, 12: 0.0}, {i: 0.5 for i in range(13)}, {6: 3.0, 5: 3.0}],
    [{12: 1.0, 0: 1.0}, {0: 4.0}, {3: -0.0, 9: 0.0}, {i: -2.0 for i in range(13)}],
]
GENS = 4


def chain_case(strategy):
    """(layout, fitness[g][r], per trial (seed, first key, sigma per population)); trials 0 and 1 share a seed, trial 0's keys lie
    above 2^32"""
    from ses import BatchEliteLayout
    if strategy == EVOLUTION:
        layout, tops = BatchEliteLayout(EVOLUTION, 12, EVOLUTION_K), EVOLUTION_TOPS
    else:
        layout, tops = BatchEliteLayout(GENETIC, 13, GENETIC_K), GENETIC_TOPS
    fits = [[crafted(int(layout.n[r]), tops[r][g], shift=g + 2 * r) for r in range(layout.R)] for g in range(GENS)]
    params = []
    for r in range(layout.R):
        sigma0 = 0.1 + 0.07 * r
        params.append(dict(seed=7 if r < 2 else 7 + r, gen0=(1 << 32) + 5 if r == 0 else 3 * r,
                           sigma=[float(np.float32(sigma0 * (0.97 - 0.01 * r) ** g)) for g in range(GENS + 1)]))
    return layout, fits, params


def check_evolution_cases(layout, fits):
    """every case the evolution chain is meant to contain really occurs in the handcrafted vectors"""
    seen = set()
    for r in range(layout.R):
        k, state, fell = int(layout.elite_num[r]), 1, False
        for g in range(GENS):
            fit = fits[g][r]
            ids, flags, new = np_select(fit, k, state)
            first, members = int(ids[0]), set(int(i) for i in ids)
            if tie_straddles(fit, k):
                seen.add("tie across the elite boundary")
            if has_signed_zero_pair(fit):
                seen.add("+-0 pair")
            if first == 0 and 1 in members and state == 1 and any(flags):
                seen.add("0 first, 1 among the elites: flag")
            if first == 1 and 0 in members and state == 1 and any(flags):
                seen.add("1 first, 0 among the elites while the state is 1")
            if first not in (0, 1) and state == 1 and new == 0:
                fell = True
            if fell and first == 0 and state == 0 and new == 1:
                seen.add("the state falls to 0, then 0 is first again")
            if state == 0 and first == 1 and not any(flags) and new == 0:
                seen.add("state 0 with 1 first: no flag")
            state = new
    assert seen == {"tie across the elite boundary", "+-0 pair", "0 first, 1 among the elites: flag",
                    "1 first, 0 among the elites while the state is 1", "the state falls to 0, then 0 is first again",
                    "state 0 with 1 first: no flag"}, seen


def check_genetic_cases(layout, fits):
    seen = set()
    for r in range(layout.R):
        for g in range(GENS):
            if tie_straddles(fits[g][r], int(layout.elite_num[r])):
                seen.add("tie")
            if has_signed_zero_pair(fits[g][r]):
                seen.add("zero")
                order = np_order(fits[g][r])
                assert list(fits[g][r][order]) == sorted(fits[g][r], reverse=True)
    assert seen == {"tie", "zero"}
    assert tuple(layout.n) == (12, 12, 13, 13) and layout.n[2] == layout.elite_num[2], "ragged, and one trial is all elites"


def elite_table(layout, params, g):
    from learning_strategies.evolution.batch import ELITE_TRIAL_DTYPE
    table = np.zeros(layout.R, dtype=ELITE_TRIAL_DTYPE)
    for r, p in enumerate(params):
        table[r] = (p["seed"], p["gen0"] + g, p["gen0"] + g + 1, np.float32(p["sigma"][g]), np.float32(p["sigma"][g + 1]),
                    layout.row0[r], layout.n[r], layout.elite_num[r], layout.parent0[r])
    return dev(table.view(np.uint8).reshape(layout.R, ELITE_TRIAL_DTYPE.itemsize))


def solo_generation(es, layout, r, fit, p, g, parents_in, alias_state):
    """The solo sequence on trial r's slice: (theta_next[n, P], parents_out, best[1], elite ids[k]); alias_state int32[1] is updated
    in place (simple_evolution) or None"""
    n, k = int(layout.n[r]), int(layout.elite_num[r])
    pmap = dev(layout.parent_map(r))
    best = es.zeros(1)
    rank, _ = es.rank_center(dev(fit), want_weights=False, best=best)
    ids, sel, alias = es.elite_select(rank, k, pmap, alias_state)
    rows = es.perturb(parents_in, p["sigma"][g], p["seed"], p["gen0"] + g, 0, k, parent_idx=sel, row_ids=ids, idx_in_range=True)
    parents_out = es.elite_mean(rows, alias).view(1, -1) if layout.evolution else rows
    theta = es.perturb(parents_out, p["sigma"][g + 1], p["seed"], p["gen0"] + g + 1, 0, n, parent_idx=pmap, idx_in_range=True)
    return theta, parents_out, best, ids


def parent_rows(layout, r):
    p0 = int(layout.parent0[r])
    return slice(p0, p0 + (1 if layout.evolution else int(layout.elite_num[r])))


def run_solo_chain(es, layout, fits, params):
    """per generation and trial: dict of host arrays"""
    out = []
    parents = [es.zeros(parent_rows(layout, r).stop - parent_rows(layout, r).start, es.P) for r in range(layout.R)]
    alias = [torch.ones(1, dtype=torch.int32, device=es.device) if layout.evolution else None for _ in range(layout.R)]
    for g in range(GENS):
        row = []
        for r, p in enumerate(params):
            theta, parents[r], best, ids = solo_generation(es, layout, r, fits[g][r], p, g, parents[r], alias[r])
            es.sync()
            row.append(dict(theta=host(theta).copy(), parents=host(parents[r]).copy(), best=host(best).copy(), ids=host(ids).copy(),
                            alias=host(alias[r]).copy() if layout.evolution else None))
        out.append(row)
    return out


def run_batch_chain(es, layout, fits, params):
    out = []
    parents = [es.zeros(layout.parents_total, es.P), es.empty(layout.parents_total, es.P)]
    alias = torch.ones(layout.R, dtype=torch.int32, device=es.device) if layout.evolution else None
    theta = es.zeros(layout.rows_total, es.P)                         # theta_next is the buffer of the evaluated population
    cur = 0
    for g in range(GENS):
        best = es.zeros(layout.R)
        fit = dev(np.concatenate(fits[g]))
        got, ids = es.elite_generation_batch(fit, layout, elite_table(layout, params, g), parents[cur], parents[cur ^ 1],
                                             alias_state=alias, theta_next=theta, best=best, want_ids=True)
        assert got is theta
        cur ^= 1
        es.sync()
        row = []
        for r in range(layout.R):
            row0, n, k = int(layout.row0[r]), int(layout.n[r]), int(layout.elite_num[r])
            row.append(dict(theta=host(theta[row0:row0 + n]).copy(), parents=host(parents[cur][parent_rows(layout, r)]).copy(),
                            best=host(best[r:r + 1]).copy(),
                            ids=host(ids[r, :k] if layout.evolution else ids[parent_rows(layout, r)]).copy(),
                            alias=host(alias[r:r + 1]).copy() if layout.evolution else None))
        out.append(row)
    return out


def assert_chains_equal(got, want, layout, fits, what):
    for g in range(len(want)):
        for r in range(layout.R):
            for key in ("ids", "best", "parents", "theta") + (("alias",) if layout.evolution else ()):
                assert_bit_equal(got[g][r][key], want[g][r][key], f"{what}: generation {g}, trial {r}: {key}")
            assert got[g][r]["best"][0] == fits[g][r].max()


@pytest.mark.parametrize("P", [226, 6562])
@pytest.mark.parametrize("strategy", [GENETIC, EVOLUTION], ids=["genetic", "evolution"])
def test_batch_tail_equals_solo_calls_on_the_slices(strategy, P):
    from ses import HipES
    layout, fits, params = chain_case(strategy)
    (check_evolution_cases if strategy == EVOLUTION else check_genetic_cases)(layout, fits)      # on the CPU, before any launch
    ref, es = HANDLES[P](HipES), HANDLES[P](HipES)
    try:
        assert es.P == P
        want = run_solo_chain(ref, layout, fits, params)
        got = run_batch_chain(es, layout, fits, params)
        assert_chains_equal(got, want, layout, fits, f"strategy {strategy}, P = {P}")
        if strategy == EVOLUTION:                                       # the device agrees with the few lines of numpy as well
            for r in range(layout.R):
                state = 1
                for g in range(GENS):
                    ids, _, state = np_select(fits[g][r], int(layout.elite_num[r]), state)
                    assert list(got[g][r]["ids"]) == list(ids) and int(got[g][r]["alias"][0]) == state
    finally:
        ref.close()
        es.close()


# ---- one handle, every kind of call ---------------------------------------------------------------------------------------------------

def adam_a(lr, t):
    return lr * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.99 ** t)             # optimizers.py:43-47


def openai_case(R, n, P, salt):
    rng = np.random.RandomState(100 * R + n + salt)
    fit = rng.choice(np.array([-1.5, 0.25, 0.5, 2.0, 3.0], np.float32), size=(R, n))
    state = ((rng.randn(R, P) * 0.3).astype(np.float32), (rng.randn(R, P) * 1e-3).astype(np.float32),
             (rng.rand(R, P) * 1e-5).astype(np.float32))
    trials = [dict(seed=11 + r, gen=4 + r, lr=0.05 / (r + 1), sigma=0.1 + 0.05 * r, next_sigma=float(np.float32(0.09 + 0.05 * r)),
                   adam_t=2 + r) for r in range(R)]
    return fit, state, trials


def openai_solo(es, fit, state, trials):
    """R ses_openai_generation calls on the slices: host (mu, m, v, theta, best) per trial"""
    out = []
    for r, t in enumerate(trials):
        outs = tuple(es.empty(es.P) for _ in range(3))
        best = es.zeros(1)
        theta = es.openai_generation(dev(fit[r]), t["seed"], t["gen"], t["lr"], t["sigma"], adam_a(t["lr"], t["adam_t"]),
                                     tuple(dev(x[r]) for x in state), outs, t["next_sigma"], t["gen"] + 1, 0, fit.shape[1], best=best)
        es.sync()
        out.append(tuple(host(x).copy() for x in outs) + (host(theta).copy(), host(best).copy()))
    return out


def openai_batch(es, fit, state, trials):
    from learning_strategies.evolution.batch import TRIAL_DTYPE
    R, n = fit.shape
    table = np.zeros(R, dtype=TRIAL_DTYPE)
    for r, t in enumerate(trials):
        table[r] = (t["seed"], t["gen"], t["gen"] + 1, adam_a(t["lr"], t["adam_t"]), np.float32(-(t["lr"] / (float(n) * t["sigma"]))),
                    np.float32(t["next_sigma"]))
    outs = tuple(es.empty(R, es.P) for _ in range(3))
    best = es.zeros(R)
    theta = es.openai_generation_batch(dev(fit.reshape(-1)), n, dev(table.view(np.uint8).reshape(R, TRIAL_DTYPE.itemsize)),
                                       tuple(dev(x) for x in state), outs, best=best)
    es.sync()
    return [tuple(host(x[r]).copy() for x in outs) + (host(theta[r * n:(r + 1) * n]).copy(), host(best[r:r + 1]).copy()) for r in range(R)]


def assert_openai_equal(got, want, what):
    for r, (a, b) in enumerate(zip(got, want)):
        for name, x, y in zip(("mu", "m", "v", "theta", "best"), a, b):
            assert_bit_equal(x, y, f"{what}: trial {r}: {name}")


def test_elite_batches_share_a_handle_with_the_other_tails():
    """an elite batch, a solo openai_es generation of as many rows as the batch had in all, an openai_es batch, an elite batch of the
    other strategy, the solo generation again: the elite ids lie where the other tails keep their rank vector and ticket counters,
    so the handle's caches change hands every time.  Everything stays bit-equal to what fresh handles give."""
    from ses import HipES
    es = HANDLES[226](HipES)
    fresh = lambda: HANDLES[226](HipES)
    try:
        want = {}
        for strategy in (EVOLUTION, GENETIC):
            layout, fits, params = chain_case(strategy)
            h = fresh()
            want[strategy] = (layout, fits, run_batch_chain(h, layout, fits, params), run_solo_chain(h, layout, fits, params), params)
            h.close()
        rows = want[EVOLUTION][0].rows_total
        solo_case, batch_case = openai_case(1, rows, 226, 1), openai_case(3, 13, 226, 2)
        h = fresh()
        want_solo = openai_solo(h, *solo_case)
        h.close()
        h = fresh()
        want_batch = openai_solo(h, *batch_case)
        h.close()

        assert_openai_equal(openai_solo(es, *solo_case), want_solo, "solo openai_es generation on the new handle")
        for step, strategy in enumerate((EVOLUTION, GENETIC)):
            layout, fits, fresh_batch, solo_chain, params = want[strategy]
            got = run_batch_chain(es, layout, fits, params)
            assert_chains_equal(got, fresh_batch, layout, fits, f"elite batch {step} on the shared handle against a fresh handle")
            assert_chains_equal(got, solo_chain, layout, fits, f"elite batch {step} on the shared handle against the solo calls")
            assert_openai_equal(openai_solo(es, *solo_case), want_solo, f"solo openai_es generation after elite batch {step}")
            assert_openai_equal(openai_batch(es, *batch_case), want_batch, f"openai_es batch after elite batch {step}")
        layout, fits, fresh_batch, _, params = want[EVOLUTION]
        assert_chains_equal(run_batch_chain(es, layout, fits, params), fresh_batch, layout, fits, "elite batch after the openai_es batch")
    finally:
        es.close()


# ---- limits ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strategy,N,ks", [(EVOLUTION, 1023, (7, 1024)), (GENETIC, 1024, (1, 512))], ids=["evolution", "genetic"])
def test_trials_of_1024_rows(strategy, N, ks):
    from ses import BatchEliteLayout, HipES
    layout = BatchEliteLayout(strategy, N, ks)
    assert tuple(layout.n) == (1024, 1024)
    rng = np.random.RandomState(5)
    fits = [[rng.choice(np.array([-1.5, -0.0, 0.0, 0.5, 2.0, 3.0], np.float32), size=1024) for _ in range(2)]]
    params = [dict(seed=3, gen0=2 + r, sigma=[0.3, 0.2]) for r in range(2)]
    ref, es = HANDLES[226](HipES), HANDLES[226](HipES)
    try:
        # one generation from non-zero parents
        start = (rng.randn(layout.parents_total, 226) * 0.3).astype(np.float32)
        parents = [dev(start), es.empty(layout.parents_total, 226)]
        alias = torch.ones(2, dtype=torch.int32, device=es.device) if layout.evolution else None
        best = es.zeros(2)
        theta, ids = es.elite_generation_batch(dev(np.concatenate(fits[0])), layout, elite_table(layout, params, 0), parents[0], parents[1],
                                               alias_state=alias, best=best, want_ids=True)
        es.sync()
        for r in range(2):
            state = torch.ones(1, dtype=torch.int32, device=ref.device) if layout.evolution else None
            want = solo_generation(ref, layout, r, fits[0][r], params[r], 0, dev(start[parent_rows(layout, r)]), state)
            ref.sync()
            k = int(ks[r])
            assert_bit_equal(host(theta[1024 * r:1024 * (r + 1)]), host(want[0]), f"trial {r}: theta_next")
            assert_bit_equal(host(parents[1][parent_rows(layout, r)]), host(want[1]), f"trial {r}: parents_out")
            assert_bit_equal(host(best[r:r + 1]), host(want[2]), f"trial {r}: best")
            assert_bit_equal(host(ids[r, :k] if layout.evolution else ids[parent_rows(layout, r)]), host(want[3]), f"trial {r}: ids")
            if layout.evolution:
                assert_bit_equal(host(alias[r:r + 1]), host(state), f"trial {r}: alias_state")
    finally:
        ref.close()
        es.close()


def test_refusals_name_the_function():
    from ses import BatchEliteLayout, HipES, SesError, _lib
    es = HANDLES[226](HipES)
    try:
        P = es.P
        layout = BatchEliteLayout(EVOLUTION, 12, (2, 3))
        size = ctypes.sizeof(_lib.SesBatchEliteTrial)
        assert size == 48
        table = dev(np.zeros((2, size), np.uint8))
        a, b = es.zeros(2, P), es.zeros(2, P)
        alias = torch.ones(2, dtype=torch.int32, device=es.device)
        fit = es.zeros(26)
        for kwargs in (dict(parents_out=a), dict(alias_state=None), dict(fitness=es.zeros(25)), dict(parents_in=es.zeros(3, P)),
                       dict(trials=dev(np.zeros((2, 40), np.uint8))), dict(alias_state=torch.ones(3, dtype=torch.int32, device=es.device)),
                       dict(best=es.zeros(3)), dict(theta_next=es.zeros(25, P)), dict(layout=None)):
            args = dict(fitness=fit, layout=layout, trials=table, parents_in=a, parents_out=b, alias_state=alias)
            args.update(kwargs)
            with pytest.raises(SesError, match="elite_generation_batch"):
                es.elite_generation_batch(**args)
        genetic = BatchEliteLayout(GENETIC, 12, (2, 3))
        with pytest.raises(SesError, match="elite_generation_batch"):       # simple_genetic takes no alias_state
            es.elite_generation_batch(es.zeros(24), genetic, table, es.zeros(5, P), es.zeros(5, P), alias_state=alias)

        # the library's own checks of its host arguments, below the front end; the device table is never reached
        lib = _lib.load()
        theta = es.zeros(26 * P)
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

        def raw(strategy=EVOLUTION, R=2, n_max=13, k_max=3, rows_total=26, parents_total=2, pin=a, pout=b, alias_state=alias):
            return lib.ses_elite_generation_batch(es._h, strategy, p(fit), R, p(table), n_max, k_max, rows_total, parents_total, p(pin),
                                                  p(pout), p(alias_state), p(theta), None, None)

        for kwargs in (dict(R=0), dict(n_max=1025, rows_total=2050), dict(k_max=14), dict(pout=a), dict(alias_state=None),
                       dict(n_max=1), dict(k_max=0), dict(rows_total=27), dict(rows_total=3), dict(rows_total=12), dict(parents_total=3),
                       dict(strategy=0), dict(strategy=GENETIC, alias_state=None, parents_total=7),
                       dict(strategy=GENETIC, alias_state=None, parents_total=1), dict(strategy=GENETIC, parents_total=5),
                       dict(rows_total=(1 << 20) + 1, R=65535, n_max=1024)):
            rc = raw(**kwargs)
            assert rc != 0, kwargs
            with pytest.raises(SesError, match="ses_elite_generation_batch"):
                _lib.check(rc, "raw call")
        assert raw(n_max=1025, rows_total=2050) == -2 and "1024" in lib.ses_last_error().decode()        # SES_ERR_UNSUPPORTED
        es.sync()
    finally:
        es.close()


# ---- BatchedRuns against R solo runs ------------------------------------------------------------------------------------------------

def load_conf(name):
    with open(os.path.join(CONF, name)) as f:
        return yaml.load(f, Loader=yaml.FullLoader)


def e2e_configs(which):
    """(configs, generations, episodes): per trial (elite_num, init_sigma, sigma_decay, strategy.seed, env.seed)"""
    if which == "cartpole-evolution":
        base, name, N, E, G = load_conf("cartpole.yaml"), "simple_evolution", 16, 2, 6
        points = [(4, 2, 0.9999, 3, 11), (2, 0.5, 0.99, 3, 12), (16, 1.0, 0.9, 5, 13), (1, 0.3, 0.999, 6, 14)]   # trials 0, 1 share a seed
    elif which == "cartpole-genetic-ragged":                 # 12, 12, 13, 13 rows: the trials' row offsets are no multiple of anything
        base, name, N, E, G = load_conf("cartpole.yaml"), "simple_genetic", 13, 2, 4
        points = [(2, 2, 0.9999, 3, 11), (3, 0.5, 0.99, 3, 12), (13, 1.0, 0.9, 5, 13), (1, 0.3, 0.999, 6, 14)]
    elif which == "cartpole-pomdp-gru-genetic":
        base, name, N, E, G = load_conf("cartpole_pomdp_gru.yaml"), "simple_genetic", 12, 2, 3
        points = [(2, 1.0, 0.995, 1, 4), (3, 0.5, 0.99, 2, 5)]
    elif which == "lunarlander-evolution":
        base, name, N, E, G = load_conf("lunarlander.yaml"), "simple_evolution", 8, 1, 2
        base["env"]["max_step"] = 60
        points = [(2, 2, 0.999, 1, 1), (3, 0.3, 0.99, 2, 7)]
    else:
        base, name, N, E, G = load_conf("bipedalwalker.yaml"), "simple_genetic", 6, 1, 2
        base["env"]["max_step"] = 30
        points = [(2, 2, 0.999, 1, 1), (3, 0.3, 0.99, 2, 7)]
    configs = []
    for elite_num, init_sigma, decay, seed, env_seed in points:
        cfg = copy.deepcopy(base)
        cfg["strategy"] = dict(name=name, init_sigma=init_sigma, sigma_decay=decay, elite_num=elite_num, offspring_num=N, seed=seed)
        cfg["env"]["seed"] = env_seed
        configs.append(cfg)
    return configs, G, E


@pytest.mark.parametrize("which", ["cartpole-evolution", "cartpole-genetic-ragged", "cartpole-pomdp-gru-genetic", "lunarlander-evolution", "bipedalwalker-genetic"])
def test_batched_runs_equal_solo_runs(which, tmp_path, monkeypatch):
    import builder
    from learning_strategies.evolution.batch import BatchedRuns
    monkeypatch.chdir(tmp_path)
    configs, G, E = e2e_configs(which)
    evolution = configs[0]["strategy"]["name"] == "simple_evolution"
    solo = []
    for cfg in configs:
        loop = builder.build_loop(copy.deepcopy(cfg), G, 1, E, False, 10 ** 9)
        loop.run()
        s = loop.offspring_strategy
        torch.cuda.synchronize()
        parents = host(s.mu_model).reshape(-1).copy() if evolution else host(s.elite_models).copy()
        solo.append(dict(best=[b for b, _ in loop.history], parents=parents, curr_sigma=s.curr_sigma,
                         elite=s.get_elite_model().flat().astype(np.float32)))
    runs = BatchedRuns(configs, G, E).run()
    try:
        assert runs.R == len(configs)
        for r, want in enumerate(solo):
            assert len(want["best"]) == G
            print(which, r, runs.history[r], want["best"])
            assert runs.history[r] == want["best"], f"trial {r}: best rewards per generation"
            got = host(runs.parents(r))
            assert got.shape == ((runs.P,) if evolution else (configs[r]["strategy"]["elite_num"], runs.P))
            assert_bit_equal(got, want["parents"], f"trial {r}: final parents")
            assert runs.t[r] == 0
            assert runs.curr_sigma[r] == want["curr_sigma"]
            assert_bit_equal(runs.elite_model(r).flat().astype(np.float32), want["elite"], f"trial {r}: elite model")
            # the final checkpoint, through test.py's loader
            path = os.path.join(runs.save_dirs[r], "saved_models", f"ep_{G}.pt")
            network = builder.build_network(configs[r]["network"])
            network.load_state_dict(torch.load(path))
            assert_bit_equal(network.flat().astype(np.float32), want["elite"], f"trial {r}: checkpoint")
            with open(os.path.join(runs.save_dirs[r], "metrics.jsonl")) as f:
                lines = [json.loads(line) for line in f]
            assert [m["best_reward"] for m in lines] == want["best"] and lines[-1]["curr_sigma"] == want["curr_sigma"]
        assert len(set(runs.save_dirs)) == runs.R
    finally:
        runs.close()


def test_sweep_concurrent_equals_sequential(tmp_path, monkeypatch):
    import sweep_main
    spec = {"method": "grid", "metric": {"name": "ep5_mean_reward", "goal": "maximize"},
            "parameters": {"cfg-path": {"value": os.path.join(CONF, "cartpole.yaml")},
                           "init-sigma": {"values": [0.5, 2.0]}, "elite-num": {"values": [2, 4]},
                           "offspring-num": {"value": 16}, "generation-num": {"value": 5}}}
    sweep = tmp_path / "grid4.yaml"
    sweep.write_text(yaml.safe_dump(spec))
    records = {}
    for concurrent in (1, 4):
        cwd = tmp_path / f"concurrent{concurrent}"
        cwd.mkdir()
        monkeypatch.chdir(cwd)
        monkeypatch.setattr(sys, "argv", ["sweep_main.py", "--sweep", str(sweep), "--eval-ep-num", "2", "--concurrent", str(concurrent)])
        sweep_main.main()
        with open(cwd / "logs" / "sweeps" / "grid4" / "trials.jsonl") as f:
            records[concurrent] = [json.loads(line) for line in f]
    assert len(records[1]) == len(records[4]) == 4
    for a, b in zip(records[1], records[4]):
        assert a.keys() == b.keys()
        for key in ("trial", "params", "ep5_mean_reward", "best_reward", "generations"):
            assert a[key] == b[key], f"trial {a['trial']}: {key}: {b[key]} with --concurrent 4, {a[key]} without"
    assert len({r["log_dir"] for r in records[4]}) == 4
