"""ses_run_generations with "fused_perturb_rollout" at 1 against 0, bit for bit.

With the knob at 1 the launch that ends an openai_es generation (k_es_apply_perturb: Adam on the mean + the rows of the next
population) is not made between two generations of one call: the rollout kernel of the next generation
(k_rollout_cartpole_mlp_handover_perturb) applies the update in every workgroup and draws the rows its own waves run.  It acts
where the light + heavy pair kernel runs: fixed-length CartPole MLP populations of 16 384 < n x E <= 20 480 envs (n = 3277 ...
4096 at E = 5, 4097 ... 5120 at E = 4, 2049 ... 2560 at E = 8).  Every case runs the same state through both knob values on
handles of their own and compares fitness, best, mu, m, v and the whole population after the call as bit patterns, and asserts
through ses_launch_counts which kernels ran -- so that a later change of the split model cannot turn a case into knob 0
against knob 0.

Eligibility clauses and the case that falls back for each:
  * the knob itself, and k = 1 (the call's last generation always launches k_es_apply_perturb);
  * the replicated tail with the fused update launch: "fused_apply_perturb" = 0, "es_final_max_chunks" = 4;
  * the pair kernel: a population one row below its range, episodic mode, the hand-over knob that deselects it
    ("rollout_heavy_prio_steps" = 0 with no hand-over step);
  * chunks <= 16 and the LDS budget (rows per workgroup): inside the pair kernel's range both fail together and only at E = 1
    (more than 16 384 rows; 80 rows per workgroup) -- one case, n = 20 000 at E = 1;
  * P <= 1024 cannot fail for the CartPole MLP (P = 226), and the one-GPU clause is `world == 1` in the C loop: the sharded
    runs of test_gpu_multirank.py / test_gpu_device_loop_world8.py go through it with the knob at its default.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR = 0.05
FIXED, EPISODIC = 1, 0
T = 500


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_bit_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {bad.sum()} of {bad.size} elements differ, first at {at}: {got[at]!r} vs {want[at]!r}")


def start_state(kind, n, P, sigma, rng):
    """(mu, theta, m, v, adam_t, gen0): `young` -- generation 0 from the zero network, as ESLoop starts; `trained` -- a mean that
    keeps the pole up for a while (hidden unit 0 reads 0.3 theta + dtheta, action 1 follows its sign; the cart drifts out after
    ~130 steps) with Adam moments of a run under way; `cap` -- one that also reads the cart (0.05 x + 0.26 dx + 1.5 theta + dtheta)
    and holds it for the whole horizon"""
    if kind == "young":
        mu, m, v, adam_t, gen0 = np.zeros(P, np.float32), np.zeros(P, np.float32), np.zeros(P, np.float32), 0, 0
    else:
        mu = np.zeros(P, np.float32)
        mu[:4] = [0.05, 0.26, 1.5, 1.0] if kind == "cap" else [0.0, 0.0, 0.3, 1.0]
        mu[32 * 4 + 32 + 32] = 1.0
        if kind == "trained":
            mu += (rng.randn(P) * 0.01).astype(np.float32)
        m, v, adam_t, gen0 = (rng.randn(P) * 1e-3).astype(np.float32), (rng.rand(P) * 1e-5).astype(np.float32), 3, 5
    theta = mu[None] + np.float32(sigma) * rng.randn(n, P).astype(np.float32)
    theta[0] = mu
    return mu, theta.astype(np.float32), m, v, adam_t, gen0


class Run:
    """one ses_gen_state on one GPU (openai_es), as _GenerationBatch lays it out"""

    def __init__(self, n, E, knob, kind="trained", shared=True, mode=FIXED, sigma=0.05, tuning=(), seed=11):
        from ses import HipES, _lib
        self.es = es = HipES("CartPole-v1", 4, 2, True, False, max_step=T, eval_ep_num=E)
        es.set_tuning("fused_perturb_rollout", knob)
        for name, value in tuning:
            es.set_tuning(name, value)
        P = es.P
        mu, theta, m, v, adam_t, gen0 = start_state(kind, n, P, sigma, np.random.RandomState(n + E))
        st = self.st = _lib.SesGenState()
        st.strategy, st.n, st.mode, st.elite_num = 0, n, mode, 0
        st.shared_init, st.init_width = int(shared), es.init_dim
        st.init_lo, st.init_hi = es.init_range
        st.seed, st.env_seed = seed, 3
        st.learning_rate, st.sigma_decay = LR, 0.99
        st.sigma = st.pop_sigma = sigma
        st.pop_gen, st.adam_t, st.cur = gen0, adam_t, 0
        self.keep = keep = {"theta": [dev(theta), es.empty(n, P)], "parents": [dev(mu[None]), es.empty(1, P)],
                            "m": [dev(m), es.empty(P)], "v": [dev(v), es.empty(P)], "fitness": es.zeros(n),
                            "init": es.zeros(1 if shared else n, E, es.init_dim)}
        st.fitness, st.init = keep["fitness"].data_ptr(), keep["init"].data_ptr()
        for i in (0, 1):
            st.theta[i], st.parents[i] = keep["theta"][i].data_ptr(), keep["parents"][i].data_ptr()
            st.adam_m[i], st.adam_v[i] = keep["m"][i].data_ptr(), keep["v"][i].data_ptr()
        self.best = []

    def run(self, k):
        best = self.es.empty(k)
        best.fill_(float("nan"))
        self.es.run_generations(self.st, k, best)
        self.es.sync()
        self.best += list(host(best))
        return self

    def state(self):
        cur = self.st.cur
        return {"theta": host(self.keep["theta"][cur]), "mu": host(self.keep["parents"][cur]), "m": host(self.keep["m"][cur]),
                "v": host(self.keep["v"][cur]), "fitness": host(self.keep["fitness"]), "best": np.array(self.best, np.float32),
                "scalars": (self.st.sigma, self.st.pop_sigma, int(self.st.pop_gen), int(self.st.adam_t))}

    def counts(self):
        return self.es.launch_counts()                     # (pair-kernel rollouts, of them with the prologue, k_es_apply_perturb)

    def close(self):
        self.es.close()


def same(a, b, what):
    for name in ("fitness", "best", "mu", "m", "v", "theta"):
        assert_bit_equal(a[name], b[name], f"{what}: {name}")
    assert a["scalars"] == b["scalars"], (what, a["scalars"], b["scalars"])


def both_knobs(n, E, calls, **kw):
    """the same state through knob 1 and knob 0; returns (state, launch counts) of each"""
    out = {}
    for knob in (1, 0):
        r = Run(n, E, knob, **kw)
        try:
            for k in calls:
                r.run(k)
            out[knob] = (r.state(), r.counts())
        finally:
            r.close()
    same(out[1][0], out[0][0], f"n={n} E={E} calls={calls} {kw}: fused_perturb_rollout 1 vs 0")
    return out


def assert_fused(out, calls):
    """knob 1: every generation ran the pair kernel, all but the first of each call with the prologue, one k_es_apply_perturb per
    call; knob 0: the pair kernel without it, one k_es_apply_perturb per generation"""
    gens = sum(calls)
    assert out[1][1] == (gens, gens - len(calls), len(calls)), out[1][1]
    assert out[0][1] == (gens, 0, gens), out[0][1]


# (n, E, shared resets): both ends of the range at E = 5; 3277 x 5 = 16 385 envs leave ONE heavy env, so every workgroup but the
# first has no heavy envs; 3700 x 5 = 18 500: 14 404 heavy envs = 225 workgroups + 4 envs, a ragged last one and 30 without;
# one end each at E = 4 and E = 8
IN_RANGE = [(3277, 5, True), (4096, 5, True), (4096, 5, False), (3700, 5, False), (4097, 4, True), (2560, 8, False)]


@pytest.mark.parametrize("n,E,shared", IN_RANGE, ids=[f"n{n}-E{E}-{'shared' if s else 'own'}" for n, E, s in IN_RANGE])
def test_populations_in_the_pair_kernels_range(n, E, shared):
    calls = [3]
    out = both_knobs(n, E, calls, shared=shared)
    assert_fused(out, calls)
    fit = out[1][0]["fitness"]
    print(f"n={n} E={E}: fitness min {fit.min()} mean {fit.mean():.1f} max {fit.max()}")
    assert len(np.unique(fit)) > 1, "the returns should not all tie"


def test_young_population_from_the_zero_network():
    """generations 0 - 3: episodes terminate long before the horizon, so the fixed-length loop's step count is what the alive
    mask makes it"""
    calls = [4]
    out = both_knobs(4096, 5, calls, kind="young", sigma=0.1)
    assert_fused(out, calls)
    fit = out[1][0]["fitness"]
    print(f"young: fitness min {fit.min()} mean {fit.mean():.1f} max {fit.max()}")
    assert fit.min() < T / 2 and len(np.unique(fit)) > 16, (fit.min(), len(np.unique(fit)))


def test_population_at_the_cap():
    """a mean that balances and a small sigma: most offspring run to the horizon, no env terminates in their waves"""
    calls = [3]
    out = both_knobs(4096, 5, calls, kind="cap", sigma=0.02)
    assert_fused(out, calls)
    fit = out[1][0]["fitness"]
    print(f"cap: share at the cap {(fit == T).mean():.3f}, min {fit.min()}")
    assert (fit == T).mean() > 0.5, (fit == T).mean()


@pytest.mark.parametrize("k", [1, 2])
def test_short_calls(k):
    """k = 1: no fused launch at all; k = 2: exactly one"""
    out = both_knobs(4096, 5, [k])
    assert out[1][1] == (k, k - 1, 1), out[1][1]
    assert out[0][1] == (k, 0, k), out[0][1]


def test_one_call_of_eight_generations_equals_eight_calls():
    a = Run(4096, 5, 1, shared=False)
    b = Run(4096, 5, 1, shared=False)
    try:
        a.run(8)
        for _ in range(8):
            b.run(1)
        same(a.state(), b.state(), "k = 8 vs 8 x k = 1")
        assert a.counts() == (8, 7, 1) and b.counts() == (8, 0, 8), (a.counts(), b.counts())
    finally:
        a.close()
        b.close()


def test_a_call_after_a_call_continues_the_same_run():
    """3 + 2 generations in two calls against 5 in one, knob 1 on both: the state a call leaves is complete"""
    a = Run(3700, 5, 1)
    b = Run(3700, 5, 1)
    try:
        a.run(3).run(2)
        b.run(5)
        same(a.state(), b.state(), "3 + 2 vs 5")
        assert a.counts() == (5, 3, 2) and b.counts() == (5, 4, 1), (a.counts(), b.counts())
    finally:
        a.close()
        b.close()


# what makes a run ineligible -> (n, E, Run arguments, pair-kernel rollouts expected in 3 generations)
INELIGIBLE = {
    "separate-update-launch": (4096, 5, dict(tuning=(("fused_apply_perturb", 0),)), 3),
    "update-inside-the-gradient-kernel": (4096, 5, dict(tuning=(("es_final_max_chunks", 4),)), 3),
    "one-row-below-the-pair-range": (3276, 5, dict(), 0),
    "episodic-mode": (4096, 5, dict(mode=EPISODIC), 0),
    "pair-kernel-deselected": (4096, 5, dict(tuning=(("rollout_heavy_prio_steps", 0),)), 0),
    "more-than-16-chunks-and-80-rows-per-workgroup": (20000, 1, dict(), 3),
}


@pytest.mark.parametrize("why", list(INELIGIBLE))
def test_ineligible_runs_fall_back(why):
    n, E, kw, pairs = INELIGIBLE[why]
    out = both_knobs(n, E, [3], **kw)
    for knob in (1, 0):
        got = out[knob][1]
        assert got[0] == pairs and got[1] == 0, (why, knob, got)
    assert out[1][1] == out[0][1], (why, out[1][1], out[0][1])
