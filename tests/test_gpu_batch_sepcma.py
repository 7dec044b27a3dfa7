"""The sep_cma_es tail of R trials as one set of launches (ses_sepcma_generation_batch, csrc/ses_batch_sepcma.hip), the host layer
that advances such runs in lockstep (learning_strategies/evolution/batch.py) and the sweep driver's --concurrent for them.

The yardstick is the existing solo path on the same device -- ses_sepcma_generation on a trial's slice (which tests/test_gpu_sep_cma.py
holds to tests/sep_cma_np.py), builder.build_loop(...).run() for a whole run, sweep_main.py --concurrent 1 for a sweep -- and every
comparison is for equal bits: a trial in a batch computes what it computes alone.  One case is held to the numpy restatement
directly, so the check is not self-consistency alone.
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

import sep_cma_np as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = os.path.join(ROOT, "simple-es_amd", "conf")
SHAPES = {226: (4, 2, True, False), 6562: (4, 2, True, True)}       # CartPole MLP (a partial last quad), CartPole POMDP GRU
GENS = 3


@pytest.fixture(scope="module")
def handles():
    from ses import HipES
    made = {}

    def get(P, key=None):
        if (P, key) not in made:
            made[(P, key)] = HipES(None, *SHAPES[P])
            assert made[(P, key)].P == P
        return made[(P, key)]

    yield get
    for h in made.values():
        h.close()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def assert_bit_equal(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.dtype}{got.shape} against {want.dtype}{want.shape}"
    diff = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert diff.size == 0, f"{what}: {diff.size} of {got.size} values differ, first at {diff[0]}"


# ---- the cases ------------------------------------------------------------------------------------------------------------------------

def fitness_vector(kind, n, rng):
    if kind == "random":
        return rng.randn(n).astype(np.float32)
    if kind == "equal":
        return np.full(n, 1.25, np.float32)
    if kind == "zeros":                                                   # +-0 mixed: -0 ranks as +0, the higher index first
        return rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.0, -1.0], np.float32), size=n)
    return rng.choice(np.array([9.0, 10.0, 500.0], np.float32), size=n)  # large ties


KINDS = ("random", "equal", "zeros", "ties")


def tail_case(R, n, P):
    """per trial: elite_num (1 and n among them), seed, the sigma of each population, the limits, the update count its state is
    after, a random state; per generation and trial a fitness vector -- generation 0 gives trials 0 and 1 the same one"""
    rng = np.random.RandomState(1000 * R + n + P)
    mus = [(1, n, max(1, n // 2), 2, n - 1)[r % 5] if R > 1 else n for r in range(R)]
    trials = []
    for r in range(R):
        sigma0 = 0.2 + 0.11 * r
        trials.append(dict(
            mu=mus[r], seed=(1 << 40) + 3 if r == 0 else 5 + r // 2, gen0=(1 << 32) + 5 if r == 1 else 2 * r,
            sigma=[sigma0 * (1.0, 0.97, 0.95)[r % 3] ** g for g in range(GENS + 1)],
            scale_limits=((0.01, 100.0), (0.5, 2.0), (0.9, 1.1))[r % 3], step_limits=((1e-6, 1e6), (0.9, 1.05), (0.1, 10.0))[r % 3],
            t0=r % 4))
    state = [(rng.randn(R, P) * 0.3).astype(np.float32), np.exp(rng.uniform(np.log(0.3), np.log(3.0), (R, P))).astype(np.float32),
             rng.randn(R, P).astype(np.float32), (rng.randn(R, P) * 0.1).astype(np.float32),
             (1.0 + 0.05 * rng.randn(R)).astype(np.float32)]
    fits = [[fitness_vector(KINDS[(r + g) % 4], n, rng) for r in range(R)] for g in range(GENS)]
    if R > 1:
        fits[0][1] = fits[0][0].copy()
    return trials, state, fits


def tables(trials, n, P, g):
    """(the constants blocks, the weight table, the records of generation g) as device tensors, and the constants dicts"""
    from learning_strategies.evolution.batch import SEPCMA_CONSTS_DTYPE, SEPCMA_TRIAL_DTYPE, sepcma_batch_tables
    R = len(trials)
    consts, weights, dicts = sepcma_batch_tables(n, P, [t["mu"] for t in trials], [t["scale_limits"] for t in trials],
                                                 [t["step_limits"] for t in trials])
    table = np.zeros(R, dtype=SEPCMA_TRIAL_DTYPE)
    for r, t in enumerate(trials):
        table[r] = (t["seed"], t["gen0"] + g, t["gen0"] + g + 1, sc.hsig_scale(dicts[r], t["t0"] + g + 1), np.float32(t["sigma"][g]),
                    np.float32(t["sigma"][g + 1]))
    return (dev(consts.view(np.uint8).reshape(R, SEPCMA_CONSTS_DTYPE.itemsize)), dev(weights),
            dev(table.view(np.uint8).reshape(R, SEPCMA_TRIAL_DTYPE.itemsize)), dicts)


def solo_params(c, t):
    from ses import _lib
    return _lib.SesSepcmaParams(c["mu"], 0, c["mueff"], c["c_sigma"], c["d_sigma"], c["c_c"], c["c_1"], c["c_mu"], c["chi"],
                                t["scale_limits"][0], t["scale_limits"][1], t["step_limits"][0], t["step_limits"][1])


def solo_generation(es, t, c, n, g, fit, state_r):
    """ses_sepcma_generation on one trial's slice: host ((mu, C, ps, pc, step)', theta_next, best)"""
    out = tuple(es.empty(x.shape[0]) for x in state_r)
    best = es.zeros(1)
    _, w = sc.constants(n, es.P, t["mu"])
    theta = es.sepcma_generation(dev(fit), t["seed"], t["gen0"] + g, t["sigma"][g], sc.hsig_scale(c, t["t0"] + g + 1), solo_params(c, t),
                                 dev(w), tuple(dev(x) for x in state_r), out, np.float32(t["sigma"][g + 1]), t["gen0"] + g + 1, 0, n,
                                 best=best)
    es.sync()
    return tuple(host(x).copy() for x in out), host(theta).copy(), host(best).copy()


def run_solo_chain(es, trials, state, fits, n):
    """per generation and trial ((mu, C, ps, pc, step)', theta_next, best) from R solo calls per generation"""
    R = len(trials)
    cur = [tuple(np.ascontiguousarray(x[r:r + 1].reshape(-1)) for x in state) for r in range(R)]
    out = []
    for g in range(GENS):
        row = []
        for r, t in enumerate(trials):
            c, _ = sc.constants(n, es.P, t["mu"])
            new, theta, best = solo_generation(es, t, c, n, g, fits[g][r], cur[r])
            cur[r] = new
            row.append((new, theta, best))
        out.append(row)
    return out


def run_batch_chain(es, trials, state, fits, n):
    R, P = len(trials), es.P
    bufs = [tuple(dev(x) for x in state), tuple(es.empty(R, P) for _ in range(4)) + (es.empty(R),)]
    theta = es.zeros(R * n, P)                                            # theta_next is the buffer of the evaluated population
    cur, out = 0, []
    for g in range(GENS):
        consts, weights, table, _ = tables(trials, n, P, g)
        best = es.zeros(R)
        got = es.sepcma_generation_batch(dev(np.concatenate(fits[g])), n, [t["mu"] for t in trials], table, consts, weights, bufs[cur],
                                         bufs[cur ^ 1], theta_next=theta, best=best)
        assert got is theta
        cur ^= 1
        es.sync()
        new = [host(x).copy() for x in bufs[cur]]
        th, b = host(theta).copy(), host(best).copy()
        out.append([(tuple(x[r:r + 1].reshape(-1) for x in new), th[r * n:(r + 1) * n], b[r:r + 1]) for r in range(R)])
    return out


NAMES = ("mu", "C", "p_sigma", "p_c", "step")


def assert_chains_equal(got, want, fits, what):
    for g in range(len(want)):
        for r in range(len(want[g])):
            for name, x, y in zip(NAMES, got[g][r][0], want[g][r][0]):
                assert_bit_equal(x, y, f"{what}: generation {g}, trial {r}: {name}")
            assert_bit_equal(got[g][r][1], want[g][r][1], f"{what}: generation {g}, trial {r}: theta_next")
            assert_bit_equal(got[g][r][2], want[g][r][2], f"{what}: generation {g}, trial {r}: best")
            assert got[g][r][2][0] == fits[g][r].max()


CASES = [(1, 4, 226), (3, 5, 226), (2, 257, 226), (3, 1025, 226), (3, 8, 6562), (16, 16, 226)]


@pytest.mark.parametrize("R,n,P", CASES, ids=[f"R{R}-n{n}-P{P}" for R, n, P in CASES])
def test_batch_tail_equals_solo_calls_on_the_slices(handles, R, n, P):
    es = handles(P)
    trials, state, fits = tail_case(R, n, P)
    mus = [t["mu"] for t in trials]
    assert all(1 <= m <= n for m in mus) and (R == 1 or (1 in mus and n in mus))
    want = run_solo_chain(es, trials, state, fits, n)
    got = run_batch_chain(es, trials, state, fits, n)
    assert_chains_equal(got, want, fits, f"R = {R}, n = {n}, P = {P}")
    for g in range(GENS):                                                 # the trials are not copies of one another
        for r in range(1, R):
            for k in range(4):
                assert not np.array_equal(got[g][r][0][k], got[g][0][0][k]), (g, r, NAMES[k])
            assert not np.array_equal(got[g][r][1], got[g][0][1])
        assert not np.array_equal(got[g][0][0][0], state[0][0]) and not np.array_equal(got[g][0][0][1], state[1][0])
    if R > 1:
        assert np.array_equal(fits[0][0], fits[0][1])                     # one fitness vector, two trials, two different updates


def test_batch_tail_equals_the_numpy_restatement(handles):
    """R = 2, n = 16, P = 226, one generation from a random state, against SepCmaNP.evaluate: mu, C, p_sigma, p_c for equal bits; the
    step within one float32 step (its exp() is the device's own, as in tests/test_gpu_sep_cma.py); the next population for equal bits
    given the device's step"""
    R, n, P = 2, 16, 226
    es = handles(P)
    trials, state, fits = tail_case(R, n, P)
    consts, weights, table, _ = tables(trials, n, P, 0)
    out = tuple(es.empty(R, P) for _ in range(4)) + (es.empty(R),)
    best = es.zeros(R)
    theta = es.sepcma_generation_batch(dev(np.concatenate(fits[0])), n, [t["mu"] for t in trials], table, consts, weights,
                                       tuple(dev(x) for x in state), out, best=best)
    es.sync()
    out, theta, best = [host(x) for x in out], host(theta), host(best)
    for r, t in enumerate(trials):
        ref = sc.SepCmaNP(P, t["sigma"][0], 1.0, n, elite_num=t["mu"], seed=t["seed"], scale_limits=t["scale_limits"],
                          step_limits=t["step_limits"])
        ref.mu, ref.C, ref.ps, ref.pc = (state[k][r].copy() for k in range(4))
        ref.step, ref.t, ref.gen = state[4][r], t["t0"], t["gen0"]
        assert ref.evaluate(fits[0][r]) == best[r]
        for name, got, want in zip(NAMES, out[:4], (ref.mu, ref.C, ref.ps, ref.pc)):
            assert_bit_equal(got[r], want, f"trial {r}: {name}")
        step = out[4][r:r + 1]
        d = abs(int(step.view(np.uint32)[0]) - int(np.array([ref.step], np.float32).view(np.uint32)[0]))
        assert d <= 1, f"trial {r}: step' {step[0]!r} against {ref.step!r}: {d} float32 steps apart"
        assert step[0] != state[4][r]
        assert_bit_equal(theta[r * n:(r + 1) * n], sc.population(ref.mu, ref.C, step[0], t["sigma"][1], t["seed"], t["gen0"] + 1, 0, n),
                         f"trial {r}: theta_next")


# ---- one handle, every kind of call ---------------------------------------------------------------------------------------------------

def adam_a(lr, t):
    return lr * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.99 ** t)             # optimizers.py:43-47


def openai_case(R, n, P):
    rng = np.random.RandomState(100 * R + n)
    fit = rng.choice(np.array([-1.5, 0.25, 0.5, 2.0, 3.0], np.float32), size=(R, n))
    state = ((rng.randn(R, P) * 0.3).astype(np.float32), (rng.randn(R, P) * 1e-3).astype(np.float32),
             (rng.rand(R, P) * 1e-5).astype(np.float32))
    trials = [dict(seed=11 + r, gen=4 + r, lr=0.05 / (r + 1), sigma=0.1 + 0.05 * r, next_sigma=float(np.float32(0.09 + 0.05 * r)),
                   adam_t=2 + r) for r in range(R)]
    return fit, state, trials


def openai_solo(es, fit, state, trials):
    out = []
    for r, t in enumerate(trials):
        outs = tuple(es.empty(es.P) for _ in range(3))
        theta = es.openai_generation(dev(fit[r]), t["seed"], t["gen"], t["lr"], t["sigma"], adam_a(t["lr"], t["adam_t"]),
                                     tuple(dev(x[r]) for x in state), outs, t["next_sigma"], t["gen"] + 1, 0, fit.shape[1])
        es.sync()
        out.append(tuple(host(x).copy() for x in outs) + (host(theta).copy(),))
    return out


def openai_batch(es, fit, state, trials):
    from learning_strategies.evolution.batch import TRIAL_DTYPE
    R, n = fit.shape
    table = np.zeros(R, dtype=TRIAL_DTYPE)
    for r, t in enumerate(trials):
        table[r] = (t["seed"], t["gen"], t["gen"] + 1, adam_a(t["lr"], t["adam_t"]), np.float32(-(t["lr"] / (float(n) * t["sigma"]))),
                    np.float32(t["next_sigma"]))
    outs = tuple(es.empty(R, es.P) for _ in range(3))
    theta = es.openai_generation_batch(dev(fit.reshape(-1)), n, dev(table.view(np.uint8).reshape(R, TRIAL_DTYPE.itemsize)),
                                       tuple(dev(x) for x in state), outs)
    es.sync()
    return [tuple(host(x[r]).copy() for x in outs) + (host(theta[r * n:(r + 1) * n]).copy(),) for r in range(R)]


def test_sepcma_batches_share_a_handle_with_the_other_tails(handles):
    """batch -> solo sepcma_generation of as many rows as the batch had in all -> openai_es batch -> batch on ONE handle: the rank vector
    is left zeroed by every call and changes hands every time.  Everything stays bit-equal to what another handle gives."""
    from ses import HipES
    P, R, n = 226, 3, 5
    ref = handles(P)
    trials, state, fits = tail_case(R, n, P)
    want_batch = run_solo_chain(ref, trials, state, fits, n)
    whole = dict(trials[2], mu=7)                                         # one trial of R n = 15 rows: the batch's rank vector, solo
    whole_fit = [[np.concatenate(fits[g])] for g in range(GENS)]
    whole_state = [x[:1] for x in state]
    want_solo = run_solo_chain(ref, [whole], whole_state, whole_fit, R * n)
    ocase = openai_case(R, n, P)
    want_openai = openai_solo(ref, *ocase)
    es = HipES(None, *SHAPES[P])
    try:
        assert_chains_equal(run_batch_chain(es, trials, state, fits, n), want_batch, fits, "batch on the new handle")
        assert_chains_equal(run_solo_chain(es, [whole], whole_state, whole_fit, R * n), want_solo, whole_fit, "solo call after the batch")
        for r, (a, b) in enumerate(zip(openai_batch(es, *ocase), want_openai)):
            for name, x, y in zip(("mu", "m", "v", "theta"), a, b):
                assert_bit_equal(x, y, f"openai_es batch after the solo call: trial {r}: {name}")
        assert_chains_equal(run_batch_chain(es, trials, state, fits, n), want_batch, fits, "batch after the openai_es batch")
        assert_chains_equal(run_batch_chain(es, trials, state, fits, n), want_batch, fits, "batch after a batch")
    finally:
        es.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_function(handles):
    from ses import SesError, _lib
    es = handles(226)
    P, R, n = es.P, 2, 8
    tsize, csize = ctypes.sizeof(_lib.SesBatchSepcmaTrial), ctypes.sizeof(_lib.SesBatchSepcmaConsts)
    assert (tsize, csize) == (40, 80)
    trials, consts, weights = dev(np.zeros((R, tsize), np.uint8)), dev(np.zeros((R, csize), np.uint8)), es.zeros(R, n)
    sin = tuple(es.zeros(R, P) for _ in range(4)) + (es.zeros(R),)
    sout = tuple(es.zeros(R, P) for _ in range(4)) + (es.zeros(R),)
    fit = es.zeros(R * n)
    base = dict(fitness=fit, n=n, mus=[4, 8], trials=trials, consts=consts, weights=weights, state_in=sin, state_out=sout)
    for kwargs in (dict(trials=dev(np.zeros((0, tsize), np.uint8))),                              # R = 0
                   dict(n=3, fitness=es.zeros(6), weights=es.zeros(R, 3), mus=[1, 1]),
                   dict(n=8193, fitness=es.zeros(2 * 8193), weights=es.zeros(R, 8193)),
                   dict(mus=[0, 8]), dict(mus=[4, 9]), dict(mus=[4]),
                   dict(state_out=sin), dict(state_out=sout[:4] + (sin[4],)), dict(state_out=sout[:4]),
                   dict(trials=dev(np.zeros((R, tsize - 8), np.uint8))), dict(trials=dev(np.zeros((R + 1, tsize), np.uint8))),
                   dict(consts=dev(np.zeros((R - 1, csize), np.uint8))), dict(weights=es.zeros(R, n - 1)), dict(fitness=es.zeros(R * n - 1)),
                   dict(trials=trials.to(torch.int8)), dict(consts=es.zeros(R, csize // 4)), dict(weights=weights.double()),
                   dict(fitness=fit.double()), dict(state_in=sin[:4] + (sin[4].double(),)), dict(best=es.zeros(R + 1)),
                   dict(theta_next=es.zeros(R * n - 1, P))):
        args = dict(base)
        args.update(kwargs)
        with pytest.raises(SesError, match="sepcma_generation_batch"):
            es.sepcma_generation_batch(**args)

    # the library's own checks of its host arguments, below the front end; the device tables are never reached
    lib = _lib.load()
    theta = es.zeros(R * n, P)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def raw(R=R, n=n, mus=(4, 8), sin=sin, sout=sout, trials=trials):
        return lib.ses_sepcma_generation_batch(es._h, p(fit), R, n, (ctypes.c_int32 * len(mus))(*mus), p(trials), p(consts), p(weights),
                                               *[p(t) for t in sin], *[p(t) for t in sout], p(theta), None)

    for kwargs in (dict(R=0), dict(n=3), dict(n=8193), dict(mus=(0, 8)), dict(mus=(4, 9)), dict(sout=sin),
                   dict(sout=sout[:2] + (sin[2],) + sout[3:]), dict(sout=sout[:4] + (sin[4],)), dict(trials=None),
                   dict(R=(1 << 20) // 8 + 1, mus=(1,) * ((1 << 20) // 8 + 1))):
        rc = raw(**kwargs)
        assert rc != 0, kwargs
        with pytest.raises(SesError, match="ses_sepcma_generation_batch"):
            _lib.check(rc, "raw call")
    assert raw(n=8193) == -2 and "8192" in lib.ses_last_error().decode()                         # SES_ERR_UNSUPPORTED
    es.sync()


# ---- BatchedRuns against R solo runs ------------------------------------------------------------------------------------------------

def load_conf(name):
    with open(os.path.join(CONF, name)) as f:
        return yaml.load(f, Loader=yaml.FullLoader)


def e2e_configs(which):
    """per trial (elite_num or None for the default, init_sigma, sigma_decay, strategy.seed, env.seed, limits)"""
    base = load_conf("cartpole_sep_cma.yaml")
    base["env"]["max_step"] = 30
    if which == "cartpole":
        points = [(2, 0.5, 1.0, 3, 11, {}), (8, 0.25, 0.999, 3, 12, dict(scale_limits=[0.5, 2.0])),
                  (None, 1.0, 0.9, 5, 13, dict(step_limits=[0.9, 1.1])), (16, 2.0, 0.99, 6, 14, {})]  # trials 0, 1 share a seed
    else:
        gru = load_conf("cartpole_pomdp_gru.yaml")
        base["network"] = gru["network"]
        base["env"]["pomdp"] = gru["env"]["pomdp"]
        points = [(4, 0.5, 1.0, 1, 4, {}), (None, 0.3, 0.99, 2, 5, {})]
    configs = []
    for elite_num, init_sigma, decay, seed, env_seed, extra in points:
        cfg = copy.deepcopy(base)
        cfg["strategy"] = dict(name="sep_cma_es", init_sigma=init_sigma, sigma_decay=decay, offspring_num=16, seed=seed, **extra)
        if elite_num is not None:
            cfg["strategy"]["elite_num"] = elite_num
        cfg["env"]["seed"] = env_seed
        configs.append(cfg)
    return configs, 4, 2


METRIC_KEYS = ("episode", "best_reward", "curr_sigma", "ep5_mean_reward")


@pytest.mark.parametrize("which", ["cartpole", "cartpole-pomdp-gru"])
def test_batched_runs_equal_solo_runs(which, tmp_path, monkeypatch):
    import builder
    from learning_strategies.evolution.batch import BatchedRuns
    monkeypatch.chdir(tmp_path)
    configs, G, E = e2e_configs(which)
    solo = []
    for cfg in configs:
        loop = builder.build_loop(copy.deepcopy(cfg), G, 1, E, False, 10 ** 9)
        loop.run()
        s = loop.offspring_strategy
        torch.cuda.synchronize()
        with open(os.path.join(loop.save_dir, "metrics.jsonl")) as f:
            lines = [json.loads(line) for line in f]
        solo.append(dict(best=[b for b, _ in loop.history], state=[host(x).copy() for x in (s.mu_model, s.variance, s._ps, s._pc, s.step)],
                         curr_sigma=s.curr_sigma, t=s.t, elite=s.get_elite_model().flat().astype(np.float32),
                         metrics=[{k: m[k] for k in METRIC_KEYS} for m in lines if "episode" in m]))
    runs = BatchedRuns(configs, G, E).run()
    try:
        assert runs.R == len(configs)
        for r, want in enumerate(solo):
            assert len(want["best"]) == G and len(want["metrics"]) == G
            print(which, r, runs.history[r], want["best"])
            assert runs.history[r] == want["best"], f"trial {r}: best rewards per generation"
            got = (runs.mu[r], runs.C[r], runs.p_sigma[r], runs.p_c[r], runs.step[r:r + 1])
            for name, x, y in zip(NAMES, got, want["state"]):
                assert_bit_equal(host(x), y, f"trial {r}: final {name}")
            assert runs.t[r] == want["t"] == G and runs.curr_sigma[r] == want["curr_sigma"]
            assert_bit_equal(runs.elite_model(r).flat().astype(np.float32), want["elite"], f"trial {r}: elite model")
            path = os.path.join(runs.save_dirs[r], "saved_models", f"ep_{G}.pt")
            network = builder.build_network(configs[r]["network"])
            network.load_state_dict(torch.load(path))
            assert_bit_equal(network.flat().astype(np.float32), want["elite"], f"trial {r}: checkpoint")
            with open(os.path.join(runs.save_dirs[r], "metrics.jsonl")) as f:
                lines = [json.loads(line) for line in f]
            assert [{k: m[k] for k in METRIC_KEYS} for m in lines] == want["metrics"], f"trial {r}: metrics.jsonl"
        assert len(set(runs.save_dirs)) == runs.R
        assert not np.array_equal(host(runs.mu[0]), host(runs.mu[1])) and not np.array_equal(host(runs.C[0]), host(runs.C[1]))
        assert not np.all(host(runs.C) == 1.0) and not np.all(host(runs.step) == 1.0)
    finally:
        runs.close()


def test_sweep_concurrent_equals_sequential(tmp_path, monkeypatch):
    import sweep_main
    with open(os.path.join(ROOT, "simple-es_amd", "sweep_config", "cartpole_sep_cma_grid.yaml")) as f:
        spec = yaml.load(f, Loader=yaml.FullLoader)
    params = spec["parameters"]
    assert params["cfg-path"]["value"] == "conf/cartpole_sep_cma.yaml" and len(params["init-sigma"]["values"]) > 1
    params["cfg-path"]["value"] = os.path.join(CONF, "cartpole_sep_cma.yaml")                  # cut small: 4 trials of 16 offspring
    params["init-sigma"]["values"] = params["init-sigma"]["values"][:2]
    params["elite-num"]["values"] = [2, 16]
    params["offspring-num"] = {"value": 16}
    params["generation-num"] = {"value": 4}
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
    assert sorted({r["params"]["elite_num"] for r in records[4]}) == [2, 16]
