"""The openai_es tail of R trials as one set of launches (ses_openai_generation_batch, csrc/ses_batch.hip), the host layer that
advances R runs in lockstep (learning_strategies/evolution/batch.py) and the sweep driver's --concurrent.

The yardstick throughout is the existing solo path on the same device -- ses_openai_generation on a trial's slice, builder.build_loop
(...).run() for a whole run, sweep_main.py --concurrent 1 for a sweep -- never the batch code itself, and every comparison is for
equal bits: a trial in a batch computes what it computes alone.
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


def adam_a(lr, t):
    return lr * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.99 ** t)             # optimizers.py:43-47


HANDLES = {
    226: lambda HipES: HipES(None, 4, 2, True, False),                                              # CartPole MLP: a ragged last quad
    581: lambda HipES: HipES("simple_spread", 12, 5, True, False, max_step=25, n_agents=2),         # simple_spread, 2 agents
    6562: lambda HipES: HipES(None, 4, 2, True, True),                                              # CartPole GRU: P > 1024
}


def make_case(R, n, P, salt=0):
    """fitness with ties everywhere (trial 0 all equal, one trial with -0.0 and +0.0), random state, and per trial its own
    (seed, lr, sigma, next_sigma, adam_t); two trials share a seed, trial 0's generation key lies above 2^32"""
    rng = np.random.RandomState(1000 * R + n + P + salt)
    fit = rng.choice(np.array([-1.5, 0.25, 0.5, 2.0, 3.0], np.float32), size=(R, n))
    fit[0, :] = 1.25
    z = R - 1 if R > 1 else 0
    fit[z, :] = rng.choice(np.array([-0.0, 0.0, 1.0], np.float32), size=n)
    fit[z, 0], fit[z, n - 1] = -0.0, 0.0
    state = ((rng.randn(R, P) * 0.3).astype(np.float32), (rng.randn(R, P) * 1e-3).astype(np.float32),
             (rng.rand(R, P) * 1e-5).astype(np.float32))
    trials = []
    for r in range(R):
        sigma = 0.1 + 0.07 * r
        trials.append(dict(seed=7 if r < 2 else 7 + r, gen=(1 << 32) + 5 if r == 0 else 3 + r, lr=0.05 / (r + 1), sigma=sigma,
                           next_sigma=float(np.float32(sigma * (0.99 - 0.01 * r))), adam_t=2 + 3 * r))
    for t in trials:
        t["next_gen"] = t["gen"] + 1
    return fit, state, trials


def trial_table(trials, n):
    from learning_strategies.evolution.batch import TRIAL_DTYPE
    table = np.zeros(len(trials), dtype=TRIAL_DTYPE)
    for r, t in enumerate(trials):
        uf = -(t["lr"] / (float(n) * t["sigma"]))
        table[r] = (t["seed"], t["gen"], t["next_gen"], adam_a(t["lr"], t["adam_t"]), np.float32(uf), np.float32(t["next_sigma"]))
    return dev(table.view(np.uint8).reshape(len(trials), TRIAL_DTYPE.itemsize))


def solo_reference(es, fit, state, trials):
    """R ses_openai_generation calls on the slices: (mu, m, v)[R, P], theta_next[R n, P], best[R] on the host"""
    R, n = fit.shape
    outs, thetas, bests = [], [], []
    for r, t in enumerate(trials):
        cur = tuple(dev(x[r]) for x in state)
        out = tuple(es.empty(es.P) for _ in range(3))
        best = es.zeros(1)
        theta = es.openai_generation(dev(fit[r]), t["seed"], t["gen"], t["lr"], t["sigma"], adam_a(t["lr"], t["adam_t"]), cur, out,
                                     t["next_sigma"], t["next_gen"], 0, n, best=best)
        es.sync()
        outs.append(tuple(host(x).copy() for x in out))
        thetas.append(host(theta).copy())
        bests.append(host(best).copy())
    return (tuple(np.stack([o[k] for o in outs]) for k in range(3)), np.concatenate(thetas), np.concatenate(bests))


def batch_call(es, fit, state, trials):
    R, n = fit.shape
    out = tuple(es.empty(R, es.P) for _ in range(3))
    best = es.zeros(R)
    theta = es.openai_generation_batch(dev(fit.reshape(-1)), n, trial_table(trials, n), tuple(dev(x) for x in state), out, best=best)
    es.sync()
    return tuple(host(x).copy() for x in out), host(theta).copy(), host(best).copy()


def assert_same(got, want, what):
    for name, a, b in zip(("mu_out", "m_out", "v_out"), got[0], want[0]):
        assert_bit_equal(a, b, f"{what}: {name}")
    assert_bit_equal(got[1], want[1], f"{what}: theta_next")
    assert_bit_equal(got[2], want[2], f"{what}: best")


TAIL_CASES = [(1, 2, 226), (3, 5, 226), (2, 255, 226), (3, 257, 226), (3, 1024, 226), (3, 1025, 226), (2, 2049, 226),
              (3, 257, 581), (2, 37, 6562), (2, 1025, 6562)]


@pytest.mark.parametrize("R,n,P", TAIL_CASES, ids=[f"{R}x{n}x{P}" for R, n, P in TAIL_CASES])
def test_batch_tail_equals_solo_calls_on_the_slices(R, n, P):
    from ses import HipES
    fit, state, trials = make_case(R, n, P)
    ref, es = HANDLES[P](HipES), HANDLES[P](HipES)
    try:
        assert es.P == P
        want = solo_reference(ref, fit, state, trials)
        got = batch_call(es, fit, state, trials)
        assert_same(got, want, f"R = {R}, n = {n}, P = {P}")
        assert np.array_equal(got[2], fit.max(axis=1)), "best[r] is the maximum of trial r's fitness"
    finally:
        ref.close()
        es.close()


def test_batch_and_solo_calls_alternate_on_one_handle():
    """three batch generations of 257, 64, 257 rows per trial, a solo generation of as many rows as the last batch had in all,
    a batch again: the rank vector's "known to be zero" cache and the scratch layout change hands every time"""
    from ses import HipES
    ref, es = HANDLES[226](HipES), HANDLES[226](HipES)
    try:
        for step, n in enumerate((257, 64, 257)):
            fit, state, trials = make_case(3, n, 226, salt=step)
            assert_same(batch_call(es, fit, state, trials), solo_reference(ref, fit, state, trials), f"batch step {step}, n = {n}")
        fit, state, trials = make_case(1, 3 * 257, 226, salt=9)
        solo_fresh = solo_reference(ref, fit, state, trials)
        assert_same(solo_reference(es, fit, state, trials), solo_fresh, "solo generation on the handle the batches used")
        fit, state, trials = make_case(3, 64, 226, salt=10)
        assert_same(batch_call(es, fit, state, trials), solo_reference(ref, fit, state, trials), "batch after the solo generation")
    finally:
        ref.close()
        es.close()


def test_refusals_name_the_function():
    from ses import HipES, SesError, _lib
    es = HANDLES[226](HipES)
    try:
        P = es.P

        def call(R, n, alias=False, fit_rows=None, state_rows=None):
            rows = R * n if fit_rows is None else fit_rows
            table = dev(np.zeros((max(R, 0), ctypes.sizeof(_lib.SesBatchTrial)), np.uint8))
            a = tuple(es.zeros(R if state_rows is None else state_rows, P) for _ in range(3))
            b = a if alias else tuple(es.zeros(R, P) for _ in range(3))
            return es.openai_generation_batch(es.zeros(rows), n, table, a, b)

        for kwargs in (dict(R=2, n=1), dict(R=2, n=8193), dict(R=0, n=4), dict(R=2, n=4, alias=True), dict(R=2, n=4, fit_rows=7),
                       dict(R=2, n=4, state_rows=3)):
            with pytest.raises(SesError, match="openai_generation_batch"):
                call(**kwargs)
        with pytest.raises(SesError, match="openai_generation_batch"):
            es.openai_generation_batch(es.zeros(8), 4, dev(np.zeros((2, 39), np.uint8)), tuple(es.zeros(2, P) for _ in range(3)),
                                       tuple(es.zeros(2, P) for _ in range(3)))

        # the library's own checks, below the front end
        lib = _lib.load()
        buf = [es.zeros(2 * P) for _ in range(6)]
        fit, theta, table = es.zeros(16), es.zeros(16 * P), dev(np.zeros((2, ctypes.sizeof(_lib.SesBatchTrial)), np.uint8))
        p = lambda t: ctypes.c_void_p(t.data_ptr())

        def raw(R, n, outs=None):
            outs = buf[3:] if outs is None else outs
            return lib.ses_openai_generation_batch(es._h, p(fit), R, n, p(table), *[p(t) for t in buf[:3]], *[p(t) for t in outs],
                                                   p(theta), None)

        for R, n, outs in ((2, 1, None), (2, 8193, None), (0, 4, None), (2, 4, buf[:3]), (1 << 19, 4, None)):
            rc = raw(R, n, outs)
            assert rc != 0
            with pytest.raises(SesError, match="ses_openai_generation_batch"):
                _lib.check(rc, "raw call")
        rc = raw(2, 8193)
        assert "8192" in lib.ses_last_error().decode()
    finally:
        es.close()


# ---- BatchedRuns against R solo runs ------------------------------------------------------------------------------------------

def load_conf(name):
    with open(os.path.join(CONF, name)) as f:
        return yaml.load(f, Loader=yaml.FullLoader)


def openai_block(n, init_sigma, sigma_decay, learning_rate, seed):
    return dict(name="openai_es", init_sigma=init_sigma, sigma_decay=sigma_decay, learning_rate=learning_rate, offspring_num=n, seed=seed)


def e2e_configs(which):
    if which == "cartpole-mlp":
        base, n, E, G = load_conf("cartpole_openai.yaml"), 64, 2, 6
        points = [(0.1, 0.999, 0.05, 3, 11), (0.3, 0.99, 0.1, 3, 12), (0.2, 0.9999, 0.02, 5, 13)]     # trials 0 and 1 share strategy.seed
    elif which == "cartpole-pomdp-gru":
        base, n, E, G = load_conf("cartpole_pomdp_gru.yaml"), 16, 2, 3
        points = [(1.0, 0.995, 0.05, 1, 4), (0.5, 0.99, 0.1, 2, 5)]
    else:
        base, n, E, G = load_conf("lunarlander_openai.yaml"), 8, 1, 2
        base["env"]["max_step"] = 60
        points = [(0.168, 0.9999, 0.087, 1, 1), (0.3, 0.999, 0.02, 2, 7)]
    configs = []
    for init_sigma, decay, lr, seed, env_seed in points:
        cfg = copy.deepcopy(base)
        cfg["strategy"] = openai_block(n, init_sigma, decay, lr, seed)
        cfg["env"]["seed"] = env_seed
        configs.append(cfg)
    return configs, G, E


@pytest.mark.parametrize("which", ["cartpole-mlp", "cartpole-pomdp-gru", "lunarlander-pomdp-gru"])
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
        solo.append(dict(best=[b for b, _ in loop.history], mu=host(s.mu_model).reshape(-1).copy(), m=host(s.optimizer.m).reshape(-1).copy(),
                         v=host(s.optimizer.v).reshape(-1).copy(), t=s.t, curr_sigma=s.curr_sigma))
    runs = BatchedRuns(configs, G, E).run()
    try:
        assert runs.R == len(configs)
        for r, want in enumerate(solo):
            assert len(want["best"]) == G
            print(which, r, runs.history[r], want["best"])
            assert runs.history[r] == want["best"], f"trial {r}: best rewards per generation"
            for name, got in (("mu", runs.mu[r]), ("m", runs.m[r]), ("v", runs.v[r])):
                assert_bit_equal(host(got), want[name], f"trial {r}: final {name}")
            assert runs.t[r] == want["t"] == G
            assert runs.curr_sigma[r] == want["curr_sigma"]
            # the final checkpoint, through test.py's loader
            path = os.path.join(runs.save_dirs[r], "saved_models", f"ep_{G}.pt")
            network = builder.build_network(configs[r]["network"])
            network.load_state_dict(torch.load(path))
            assert_bit_equal(network.flat().astype(np.float32), want["mu"].reshape(-1), f"trial {r}: checkpoint")
        assert len(set(runs.save_dirs)) == runs.R
    finally:
        runs.close()


def test_sweep_concurrent_equals_sequential(tmp_path, monkeypatch):
    import sweep_main
    spec = {"method": "grid", "metric": {"name": "ep5_mean_reward", "goal": "maximize"},
            "parameters": {"cfg-path": {"value": os.path.join(CONF, "cartpole_openai.yaml")},
                           "init-sigma": {"values": [0.1, 0.3]}, "learning-rate": {"values": [0.05, 0.1]},
                           "offspring-num": {"value": 32}, "generation-num": {"value": 5}}}
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
