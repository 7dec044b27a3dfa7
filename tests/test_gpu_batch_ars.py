"""The ars tail of R trials as one set of launches (ses_ars_generation_batch, csrc/ses_batch_ars.hip), the host layer that advances
such runs in lockstep (learning_strategies/evolution/batch.py) and the sweep driver's --concurrent for them.

The yardstick is the existing solo path on the same device -- ses_ars_generation on a trial's slice (which tests/test_gpu_ars.py holds
to tests/ars_np.py), builder.build_loop(...).run() for a whole run, sweep_main.py --concurrent 1 for a sweep -- and every comparison
is for equal bits: a trial in a batch computes what it computes alone.  One case is held to the numpy restatement directly, so the
check is not self-consistency alone.
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

import ars_np as an

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
    diff = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())      # (a float64 is two words)
    assert diff.size == 0, f"{what}: {diff.size} of {got.view(np.uint32).size} words differ, first at {diff[0]}"


# ---- the cases ------------------------------------------------------------------------------------------------------------------------

def fitness_vector(kind, n, rng):
    if kind == "random":
        return rng.randn(n).astype(np.float32)
    if kind == "equal":                                                   # sigma_R = 0: the step is 0 and mu stays, bit for bit
        return np.full(n, 1.25, np.float32)
    if kind == "zeros":                                                   # +-0 mixed: -0 ranks as +0, the higher index first
        return rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.0, -1.0], np.float32), size=n)
    return rng.choice(np.array([9.0, 10.0, 500.0], np.float32), size=n)  # large ties


KINDS = ("random", "equal", "zeros", "ties")


def kind_of(r, g):
    return KINDS[(r + g) % 4]


def tail_case(R, n, P, bs=None):
    """per trial: b (1, m, m // 2, 2 and m - 1 in turn), seed, the generation key it starts at, learning_rate, the sigma of each
    population; a random mean per trial; per generation and trial a fitness vector -- generation 0 gives trials 0 and 1 the same one"""
    rng = np.random.RandomState(1000 * R + n + P)
    m = n // 2
    if bs is None:
        bs = [min(m, max(1, (1, m, m // 2, 2, m - 1)[r % 5])) for r in range(R)]
    trials = []
    for r in range(R):
        sigma0 = 0.1 + 0.07 * r
        trials.append(dict(
            b=bs[r], seed=(1 << 40) + 3 if r == 0 else 5 + r // 2, gen0=(1 << 32) + 5 if r == 1 else 2 * r, lr=0.2 / (r + 1),
            sigma=[sigma0 * (1.0, 0.97, 0.95)[r % 3] ** g for g in range(GENS + 1)]))
    mu = (rng.randn(R, P) * 0.3).astype(np.float32)
    fits = [[fitness_vector(kind_of(r, g), n, rng) for r in range(R)] for g in range(GENS)]
    if R > 1:
        fits[0][1] = fits[0][0].copy()
    return trials, mu, fits


def table(trials, g):
    """the ses_batch_ars_trial records of generation g as a device tensor"""
    from learning_strategies.evolution.batch import ARS_TRIAL_DTYPE
    rec = np.zeros(len(trials), dtype=ARS_TRIAL_DTYPE)
    for r, t in enumerate(trials):
        rec[r] = (t["seed"], t["gen0"] + g, t["gen0"] + g + 1, t["lr"], np.float32(t["sigma"][g + 1]), t["b"])
    return dev(rec.view(np.uint8).reshape(len(trials), ARS_TRIAL_DTYPE.itemsize))


def solo_generation(es, t, n, g, fit, mu):
    """ses_ars_generation on one trial's slice: host (mu', theta_next, best, G, sigma_R)"""
    out = (es.empty(es.P),)
    best = es.zeros(1)
    theta, G, sr = es.ars_generation(dev(fit), t["b"], t["seed"], t["gen0"] + g, t["sigma"][g], t["lr"], (dev(mu),), out,
                                     np.float32(t["sigma"][g + 1]), t["gen0"] + g + 1, 0, n, best=best, want_sums=True)
    es.sync()
    return host(out[0]).copy(), host(theta).copy(), host(best).copy(), host(G).copy(), host(sr).copy()


def run_solo_chain(es, trials, mu, fits, n):
    """per generation and trial (mu', theta_next, best, G, sigma_R) from R solo calls per generation"""
    cur = [np.ascontiguousarray(mu[r]) for r in range(len(trials))]
    out = []
    for g in range(GENS):
        row = []
        for r, t in enumerate(trials):
            got = solo_generation(es, t, n, g, fits[g][r], cur[r])
            cur[r] = got[0]
            row.append(got)
        out.append(row)
    return out


def run_batch_chain(es, trials, mu, fits, n):
    R, P = len(trials), es.P
    bufs = [(dev(mu),), (es.empty(R, P),)]
    theta = es.zeros(R * n, P)                                            # theta_next is the buffer of the evaluated population
    cur, out = 0, []
    for g in range(GENS):
        best = es.zeros(R)
        got, G, sr = es.ars_generation_batch(dev(np.concatenate(fits[g])), n, [t["b"] for t in trials], table(trials, g), bufs[cur],
                                             bufs[cur ^ 1], theta_next=theta, best=best, want_sums=True)
        assert got is theta
        cur ^= 1
        es.sync()
        new, th, b, G, sr = (host(x).copy() for x in (bufs[cur][0], theta, best, G, sr))
        out.append([(new[r], th[r * n:(r + 1) * n], b[r:r + 1], G[r], sr[r:r + 1]) for r in range(R)])
    return out


NAMES = ("mu", "theta_next", "best", "G", "sigma_R")


def assert_chains_equal(got, want, fits, what):
    for g in range(len(want)):
        for r in range(len(want[g])):
            for name, x, y in zip(NAMES, got[g][r], want[g][r]):
                assert_bit_equal(x, y, f"{what}: generation {g}, trial {r}: {name}")
            assert got[g][r][2][0] == fits[g][r].max()


def check_tail_case(es, R, n, P, bs, what, knob=1):
    trials, mu, fits = tail_case(R, n, P, bs)
    m = n // 2
    got_bs = [t["b"] for t in trials]
    assert all(1 <= b <= m for b in got_bs) and (R < 5 or {1, m, m // 2, 2, m - 1} <= set(got_bs))
    want = run_solo_chain(es, trials, mu, fits, n)
    es.set_tuning("ars_fused_apply_perturb", knob)
    try:
        got = run_batch_chain(es, trials, mu, fits, n)
    finally:
        es.set_tuning("ars_fused_apply_perturb", 1)
    assert_chains_equal(got, want, fits, what)
    prev = [mu[r] for r in range(R)]
    for g in range(GENS):
        for r in range(R):
            if kind_of(r, g) == "equal" and not (g == 0 and r == 1 and R > 1):     # all returns equal: sigma_R = 0 and mu stays
                assert got[g][r][4][0] == 0.0
                assert_bit_equal(got[g][r][0], prev[r], f"{what}: generation {g}, trial {r}: mu under equal returns")
            elif kind_of(r, g) == "random" or (g == 0 and r == 1):
                assert got[g][r][4][0] > 0.0 and not np.array_equal(got[g][r][0], prev[r])
            if r:                                                         # the trials are not copies of one another
                assert not np.array_equal(got[g][r][1], got[g][0][1])
            prev[r] = got[g][r][0]
    if R > 1:                                                             # one fitness vector, two trials, two different updates
        assert np.array_equal(fits[0][0], fits[0][1]) and not np.array_equal(got[0][0][3], got[0][1][3])
    return trials


# (R, n, P, b per trial or None for the cycle 1, m, m // 2, 2, m - 1): the minimum, m = 2, and a partial last quad; every b pattern
# with the fused apply; several workgroups per trial; 3 chunks of selected pairs against 1 in one launch (the ragged chunk count:
# trial 1 must add no zero partial); P > 1024, the unfused five-launch form
CASES = [(1, 4, 226, None), (5, 16, 226, None), (3, 256, 226, None), (2, 4100, 226, (2050, 1)), (3, 16, 6562, None)]


@pytest.mark.parametrize("R,n,P,bs", CASES, ids=[f"R{R}-n{n}-P{P}" for R, n, P, _ in CASES])
def test_batch_tail_equals_solo_calls_on_the_slices(handles, R, n, P, bs):
    check_tail_case(handles(P), R, n, P, bs, f"R = {R}, n = {n}, P = {P}")


def test_batch_tail_with_the_update_as_a_launch_of_its_own(handles):
    """the knob "ars_fused_apply_perturb" = 0 at P = 226: the five-launch form against solo calls in their default form"""
    check_tail_case(handles(226), 5, 16, 226, None, "unfused, R = 5, n = 16, P = 226", knob=0)


def test_batch_tail_equals_the_numpy_restatement(handles):
    """R = 2, n = 16, P = 226, one generation from a random mean, against tests/ars_np.py: sigma_R of the restatement's selection, the
    sum of the restatement's differences in the device's order (at b <= 256 a thread's chain is one fma from 0, which the float64
    emulation rounds once: equal bits), the update and the next population for equal bits; the sum within ars_tolerance of float64"""
    R, n, P = 2, 16, 226
    es = handles(P)
    trials, mu, fits = tail_case(R, n, P)
    assert [t["b"] for t in trials] == [1, 8]
    out = (es.empty(R, P),)
    best = es.zeros(R)
    theta, G, sr = es.ars_generation_batch(dev(np.concatenate(fits[0])), n, [t["b"] for t in trials], table(trials, 0), (dev(mu),), out,
                                           best=best, want_sums=True)
    es.sync()
    mu_out, theta, best, G, sr = (host(x) for x in (out[0], theta, best, G, sr))
    for r, t in enumerate(trials):
        fit, b, gen = fits[0][r], t["b"], t["gen0"]
        sel = an.select(fit, b)
        assert len(sel) == b and best[r] == fit.max() == an.pair_scores(fit)[sel[0]]
        want_sr = an.sigma_r(fit, sel)
        assert_bit_equal(sr[r:r + 1], np.array([want_sr]), f"trial {r}: sigma_R")
        d64, d32 = an.differences(fit, sel)
        z = an.selected_noise(sel, t["seed"], gen, P)
        assert_bit_equal(G[r], an.emulate_device_sum(d32, z), f"trial {r}: G in the device's order")
        want_mu = an.update(mu[r], G[r], want_sr, t["lr"], b)
        assert_bit_equal(mu_out[r], want_mu, f"trial {r}: mu'")
        assert not np.array_equal(want_mu, mu[r])
        assert_bit_equal(theta[r * n:(r + 1) * n], an.population(want_mu, t["sigma"][1], t["seed"], gen + 1, 0, n), f"trial {r}: theta_next")
        ref_sel, ref_sr, g64, tol = an.ars_reference(fit, b, t["seed"], gen, P)
        assert np.array_equal(ref_sel, sel) and ref_sr == want_sr
        err = np.abs(G[r].astype(np.float64) - g64)
        assert np.all(err <= tol), f"trial {r}: G: worst |err| / tol = {np.max(err / np.maximum(tol, 1e-300)):.3f}"


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


def openai_batch(es, fit, state, trials):
    from learning_strategies.evolution.batch import TRIAL_DTYPE
    R, n = fit.shape
    rec = np.zeros(R, dtype=TRIAL_DTYPE)
    for r, t in enumerate(trials):
        rec[r] = (t["seed"], t["gen"], t["gen"] + 1, adam_a(t["lr"], t["adam_t"]), np.float32(-(t["lr"] / (float(n) * t["sigma"]))),
                  np.float32(t["next_sigma"]))
    outs = tuple(es.empty(R, es.P) for _ in range(3))
    theta = es.openai_generation_batch(dev(fit.reshape(-1)), n, dev(rec.view(np.uint8).reshape(R, TRIAL_DTYPE.itemsize)),
                                       tuple(dev(x) for x in state), outs)
    es.sync()
    return [host(x).copy() for x in outs] + [host(theta).copy()]


def pgpe_call(es, fit, mu):
    """a pgpe generation of len(fit) rows: host (mu', m', v', scale', theta_next)"""
    P = es.P
    state = (dev(mu), es.zeros(P), es.zeros(P), dev(np.ones(P, np.float32)))
    outs = tuple(es.empty(P) for _ in range(4))
    theta = es.pgpe_generation(dev(fit), 77, 3, 0.1, 1e-3, 0.2, 0.2, (0.01, 100.0), state, outs, 0.1, 4, 0, len(fit))
    es.sync()
    return [host(x).copy() for x in outs] + [host(theta).copy()]


def test_ars_batches_share_a_handle_with_the_other_tails(handles):
    """batch -> solo ars_generation of R n rows (as many pair scores as the batch had in all) -> a pgpe generation of exactly R m rows
    (its rank vector lies where the batch's does, entry for entry) -> openai_es batch -> batch, on ONE handle: the rank vector is left
    zeroed by every call and changes hands every time.  Everything stays bit-equal to what a handle gives that runs each call alone."""
    from ses import HipES
    P, R, n = 226, 3, 16
    m = n // 2
    ref = handles(P)
    trials, mu, fits = tail_case(R, n, P)
    want_batch = run_batch_chain(handles(P, "batch alone"), trials, mu, fits, n)
    assert_chains_equal(want_batch, run_solo_chain(ref, trials, mu, fits, n), fits, "the batch alone")
    whole = dict(trials[2], b=R * m - 1)                                  # one trial of R n = 48 rows: R m = 24 pair scores, solo
    whole_fit = [[np.concatenate(fits[g])] for g in range(GENS)]
    want_solo = run_solo_chain(ref, [whole], mu[:1], whole_fit, R * n)
    pgpe_fit = fitness_vector("random", R * m, np.random.RandomState(8))
    want_pgpe = pgpe_call(ref, pgpe_fit, mu[1])
    ocase = openai_case(R, n, P)
    want_openai = openai_batch(handles(P, "openai alone"), *ocase)
    es = HipES(None, *SHAPES[P])
    try:
        assert_chains_equal(run_batch_chain(es, trials, mu, fits, n), want_batch, fits, "batch on the new handle")
        assert_chains_equal(run_solo_chain(es, [whole], mu[:1], whole_fit, R * n), want_solo, whole_fit, "solo call after the batch")
        for name, x, y in zip(("mu", "m", "v", "scale", "theta"), pgpe_call(es, pgpe_fit, mu[1]), want_pgpe):
            assert_bit_equal(x, y, f"pgpe generation of R m rows after the solo call: {name}")
        for name, x, y in zip(("mu", "m", "v", "theta"), openai_batch(es, *ocase), want_openai):
            assert_bit_equal(x, y, f"openai_es batch after the pgpe generation: {name}")
        assert_chains_equal(run_batch_chain(es, trials, mu, fits, n), want_batch, fits, "batch after the openai_es batch")
        assert_chains_equal(run_batch_chain(es, trials, mu, fits, n), want_batch, fits, "batch after a batch")
    finally:
        es.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals_name_the_function(handles):
    """argument checks only: nothing is launched"""
    from ses import SesError, _lib
    es = handles(226)
    P, R, n = es.P, 2, 8
    tsize = ctypes.sizeof(_lib.SesBatchArsTrial)
    assert tsize == 40
    trials = dev(np.zeros((R, tsize), np.uint8))
    sin, sout = (es.zeros(R, P),), (es.zeros(R, P),)
    fit = es.zeros(R * n)
    base = dict(fitness=fit, n=n, bs=[2, 4], trials=trials, state_in=sin, state_out=sout)
    for kwargs in (dict(trials=dev(np.zeros((0, tsize), np.uint8))),                              # R = 0
                   dict(n=7, fitness=es.zeros(14)), dict(n=2, fitness=es.zeros(4), bs=[1, 1]),
                   dict(n=16386, fitness=es.zeros(2 * 16386)),
                   dict(bs=[0, 4]), dict(bs=[2, 5]), dict(bs=[2]),
                   dict(state_out=sin), dict(state_out=()),
                   dict(trials=dev(np.zeros((R, tsize - 8), np.uint8))), dict(trials=dev(np.zeros((R + 1, tsize), np.uint8))),
                   dict(fitness=es.zeros(R * n - 1)), dict(trials=trials.to(torch.int8)), dict(fitness=fit.double()),
                   dict(state_in=(sin[0].double(),)), dict(best=es.zeros(R + 1)), dict(theta_next=es.zeros(R * n - 1, P))):
        args = dict(base)
        args.update(kwargs)
        with pytest.raises(SesError, match="ars_generation_batch"):
            es.ars_generation_batch(**args)

    # the library's own checks of its host arguments, below the front end; the device table is never reached
    lib = _lib.load()
    theta = es.zeros(R * n, P)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())

    def raw(R=R, n=n, bs=(2, 4), mu_in=sin[0], mu_out=sout[0], trials=trials, fit=fit):
        return lib.ses_ars_generation_batch(es._h, p(fit), R, n, (ctypes.c_int32 * len(bs))(*bs), p(trials), p(mu_in), p(mu_out),
                                            p(theta), None, None, None)

    many = (1 << 20) // 8 + 1
    for kwargs in (dict(R=0), dict(n=7), dict(n=2, bs=(1, 1)), dict(n=16386), dict(bs=(0, 4)), dict(bs=(2, 5)), dict(mu_out=sin[0]),
                   dict(trials=None), dict(fit=None), dict(R=many, bs=(1,) * many)):
        rc = raw(**kwargs)
        assert rc != 0, kwargs
        with pytest.raises(SesError, match="ses_ars_generation_batch"):
            _lib.check(rc, "raw call")
    assert raw(n=16386) == -2 and "16384" in lib.ses_last_error().decode()                        # SES_ERR_UNSUPPORTED
    assert raw(R=many, bs=(1,) * many) == -1 and str(1 << 20) in lib.ses_last_error().decode()
    es.sync()


# ---- BatchedRuns against R solo runs ------------------------------------------------------------------------------------------------

def load_conf(name):
    with open(os.path.join(CONF, name)) as f:
        return yaml.load(f, Loader=yaml.FullLoader)


def e2e_configs(which):
    """4 trials that differ in init_sigma, sigma_decay, learning_rate, elite_num (None: the default) and both seeds"""
    base = load_conf("cartpole_ars.yaml")
    base["env"]["max_step"] = 50
    if which != "cartpole":
        gru = load_conf("cartpole_pomdp_gru.yaml")
        base["network"] = gru["network"]
        base["env"]["pomdp"] = gru["env"]["pomdp"]
    points = [(1, 0.1, 1.0, 0.2, 3, 11), (8, 0.25, 0.97, 0.05, 3, 12), (None, 0.5, 0.9, 0.4, 5, 13), (3, 0.05, 0.99, 1.0, 6, 14)]
    configs = []
    for elite_num, init_sigma, decay, lr, seed, env_seed in points:      # trials 0, 1 share a strategy seed
        cfg = copy.deepcopy(base)
        cfg["strategy"] = dict(name="ars", init_sigma=init_sigma, sigma_decay=decay, learning_rate=lr, offspring_num=16, seed=seed)
        if elite_num is not None:
            cfg["strategy"]["elite_num"] = elite_num
        cfg["env"]["seed"] = env_seed
        configs.append(cfg)
    return configs, 6, 2


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
        solo.append(dict(best=[b for b, _ in loop.history], mu=host(s.mu_model).copy(), curr_sigma=s.curr_sigma, b=s.elite_num,
                         elite=s.get_elite_model().flat().astype(np.float32),
                         metrics=[{k: m[k] for k in METRIC_KEYS} for m in lines if "episode" in m]))
    runs = BatchedRuns(configs, G, E).run()
    try:
        assert runs.R == len(configs) == 4 and [s.elite_num for s in runs.schedules] == [w["b"] for w in solo] == [1, 8, 4, 3]
        for r, want in enumerate(solo):
            assert len(want["best"]) == G and len(want["metrics"]) == G
            print(which, r, runs.history[r], want["best"])
            assert runs.history[r] == want["best"], f"trial {r}: best rewards per generation"
            assert_bit_equal(host(runs.mu[r]), want["mu"], f"trial {r}: final mu")
            assert runs.curr_sigma[r] == want["curr_sigma"]
            assert_bit_equal(runs.elite_model(r).flat().astype(np.float32), want["elite"], f"trial {r}: elite model")
            assert_bit_equal(want["elite"], want["mu"], f"trial {r}: a solo run checkpoints mu")
            path = os.path.join(runs.save_dirs[r], "saved_models", f"ep_{G}.pt")
            network = builder.build_network(configs[r]["network"])
            network.load_state_dict(torch.load(path))
            assert_bit_equal(network.flat().astype(np.float32), want["elite"], f"trial {r}: checkpoint")
            with open(os.path.join(runs.save_dirs[r], "metrics.jsonl")) as f:
                lines = [json.loads(line) for line in f]
            assert [{k: m[k] for k in METRIC_KEYS} for m in lines] == want["metrics"], f"trial {r}: metrics.jsonl"
        assert len(set(runs.save_dirs)) == runs.R
        assert not np.array_equal(host(runs.mu[0]), host(runs.mu[1])) and np.abs(host(runs.mu)).max() > 0
    finally:
        runs.close()


def test_sweep_concurrent_equals_sequential(tmp_path, monkeypatch):
    import sweep_main
    with open(os.path.join(ROOT, "simple-es_amd", "sweep_config", "cartpole_ars_grid.yaml")) as f:
        spec = yaml.load(f, Loader=yaml.FullLoader)
    params = spec["parameters"]
    assert params["cfg-path"]["value"] == "conf/cartpole_ars.yaml"
    assert params["learning-rate"]["values"] == [0.05, 0.1, 0.2, 0.4] and params["elite-num"]["values"] == [8, 32, 64, 128]
    params["cfg-path"]["value"] = os.path.join(CONF, "cartpole_ars.yaml")                       # a 2 x 2 cut: 4 trials
    params["learning-rate"]["values"] = params["learning-rate"]["values"][:2]
    params["elite-num"]["values"] = params["elite-num"]["values"][:2]
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
    assert sorted({r["params"]["elite_num"] for r in records[4]}) == [8, 32]
    assert sorted({r["params"]["learning_rate"] for r in records[4]}) == [0.05, 0.1]
