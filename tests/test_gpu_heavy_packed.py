"""The packed step in the heavy wave of the light + heavy pair kernels: "rollout_heavy_packed" at 1 against 0, bit for bit.

With the knob at 1 the heavy wave of k_rollout_cartpole_mlp_handover / k_rollout_cartpole_mlp_handover_perturb (fixed-length CartPole
MLP populations of 16 384 < n x E <= 20 480 envs) runs MlpSlicePk<4> and rollout_cartpole_mlp_loop_pk (csrc/ses_policy_pk.h): two
IEEE operations per v_pk_* instruction, each the operation the scalar form performs, in its order.  A wave with an env outside the
small-angle range keeps the scalar loop.  So nothing may change: every case runs the same inputs through both knob values on handles
of their own and compares bit patterns -- ep_return / ep_steps / fitness of one rollout (also against the C oracle), and fitness,
best, mu, m, v and the whole population after several generations of ses_run_generations, through the pair kernel with the prologue
("fused_perturb_rollout" = 1) and without it (0).  ses_launch_counts says that the pair kernels ran."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

FIXED = 1
T = 500
LR = 0.05


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


def test_the_knob_takes_minus_one_to_one():
    from ses import HipES, _lib
    es = HipES("CartPole-v1", 4, 2, True, False, max_step=T, eval_ep_num=5)
    try:
        for v in (-1, 0, 1):
            es.set_tuning("rollout_heavy_packed", v)
        for v in (-2, 2):
            with pytest.raises(_lib.SesError):
                es.set_tuning("rollout_heavy_packed", v)
    finally:
        es.close()


# ---- one rollout: ep_return, ep_steps, fitness --------------------------------------------------------------------------------

def population(n, E, seed, scale=0.6):
    rng = np.random.RandomState(seed)
    theta = (rng.randn(n, 226) * scale).astype(np.float32)
    init = rng.uniform(-0.05, 0.05, (n, E, 4)).astype(np.float32)
    return theta, init


def rollout(theta, init, E, max_step, knob, pomdp=False, tuning=()):
    from ses import HipES
    h = HipES("CartPole-v1", 4, 2, True, False, pomdp=pomdp, max_step=max_step, eval_ep_num=E)
    try:
        h.set_tuning("rollout_heavy_packed", knob)
        for name, value in tuning:
            h.set_tuning(name, value)
        fit, ep_ret, ep_steps = h.rollout(dev(theta), dev(init), mode=FIXED, want_episodes=True)
        out = host(fit), host(ep_ret), host(ep_steps)
        assert h.launch_counts()[0] == 1, "the pair kernel should have run this population"
        return out
    finally:
        h.close()


def both_rollouts(theta, init, E, max_step, what, obs_mask=0, **kw):
    """knob 1 == knob 0 == the C oracle"""
    got = {knob: rollout(theta, init, E, max_step, knob, **kw) for knob in (1, 0)}
    want = co.rollout_cartpole(theta, init, E, max_step, mode=co.MODE_FIXED_LENGTH, obs_mask=obs_mask)
    for i, name in enumerate(("fitness", "ep_return", "ep_steps")):
        assert_bit_equal(got[1][i], got[0][i], f"{what}: {name}, rollout_heavy_packed 1 vs 0")
        assert_bit_equal(got[1][i], want[i], f"{what}: {name}, rollout_heavy_packed 1 vs the oracle")
    return got[1]


# (n, E): the headline; both ends of the pair kernel's range at E = 2 and E = 8; 3277 x 5 = 16 385 envs leave ONE heavy env;
# 3700 x 5 = 18 500: 14 404 heavy envs = 900 heavy waves + 4 envs, a ragged last pair and pairs without a heavy wave
SHAPES = [(4096, 5), (8193, 2), (10240, 2), (2049, 8), (2560, 8), (3277, 5), (3700, 5)]


@pytest.mark.parametrize("n,E", SHAPES, ids=[f"n{n}-E{E}" for n, E in SHAPES])
def test_rollout_returns(n, E):
    theta, init = population(n, E, n + E)
    max_step = T if (n, E) == (4096, 5) else 160
    fit, _, ep_steps = both_rollouts(theta, init, E, max_step, f"n={n} E={E}")
    print(f"n={n} E={E}: episode lengths {ep_steps.min()} ... {ep_steps.max()}, {len(np.unique(fit))} distinct returns")
    assert len(np.unique(fit)) > 16, "the returns should not all tie"


@pytest.mark.parametrize("n,E", [(4096, 5), (3700, 5)])
def test_masked_observations(n, E):
    """obs_mask != 0 (POMDP CartPole hides the two velocities): the MASKED variant of the packed loop"""
    theta, init = population(n, E, 13)
    both_rollouts(theta, init, E, 200, f"pomdp n={n}", obs_mask=0b1010, pomdp=True)


@pytest.mark.parametrize("prio_steps,handover", [(1, 1 << 20), (250, 1 << 20), (300, 137), (0, 57)])
def test_priority_segments_and_handover(prio_steps, handover):
    """the packed loop runs in two segments (s_setprio 1, then 0) and leaves its state for the hand-over's second phase"""
    theta, init = population(4096, 5, 7)
    both_rollouts(theta, init, 5, 300, f"prio_steps={prio_steps} handover={handover}",
                  tuning=(("rollout_heavy_prio_steps", prio_steps), ("rollout_handover_step", handover)))


def test_initial_angle_outside_the_small_range_falls_back_to_the_scalar_loop():
    """one heavy env starts at 1.5 rad (> 0.78): its wave runs the general scalar loop under either knob value, every other heavy
    wave the packed one"""
    theta, init = population(4096, 5, 17)
    env = 4096 + 16 * 3 + 11                                   # a heavy env: the light waves take envs 0 ... 4095
    init[env // 5, env % 5, 2] = 1.5
    init[env // 5, env % 5, 3] = -60.0
    both_rollouts(theta, init, 5, 300, "wild heavy env")
    both_rollouts(theta, init, 5, 300, "wild heavy env, hand-over at 100", tuning=(("rollout_handover_step", 100),))


# ---- several generations of ses_run_generations: fitness, best, mu, m, v, theta ---------------------------------------------------

def start_state(n, P, sigma, rng):
    """a mean that keeps the pole up for a while (hidden unit 0 reads 0.3 theta + dtheta, action 1 follows its sign) with Adam
    moments of a run under way: episode lengths spread from a few steps to the horizon"""
    mu = np.zeros(P, np.float32)
    mu[:4] = [0.0, 0.0, 0.3, 1.0]
    mu[32 * 4 + 32 + 32] = 1.0
    mu += (rng.randn(P) * 0.01).astype(np.float32)
    m, v = (rng.randn(P) * 1e-3).astype(np.float32), (rng.rand(P) * 1e-5).astype(np.float32)
    theta = mu[None] + np.float32(sigma) * rng.randn(n, P).astype(np.float32)
    theta[0] = mu
    return mu, theta.astype(np.float32), m, v


class Run:
    """one ses_gen_state on one GPU (openai_es)"""

    def __init__(self, n, E, heavy_packed, fused, shared=True, sigma=0.05, pomdp=False):
        from ses import HipES, _lib
        self.es = es = HipES("CartPole-v1", 4, 2, True, False, pomdp=pomdp, max_step=T, eval_ep_num=E)
        es.set_tuning("rollout_heavy_packed", heavy_packed)
        es.set_tuning("fused_perturb_rollout", fused)
        P = es.P
        mu, theta, m, v = start_state(n, P, sigma, np.random.RandomState(n + E))
        st = self.st = _lib.SesGenState()
        st.strategy, st.n, st.mode, st.elite_num = 0, n, FIXED, 0
        st.shared_init, st.init_width = int(shared), es.init_dim
        st.init_lo, st.init_hi = es.init_range
        st.seed, st.env_seed = 11, 3
        st.learning_rate, st.sigma_decay = LR, 0.99
        st.sigma = st.pop_sigma = sigma
        st.pop_gen, st.adam_t, st.cur = 5, 3, 0
        self.keep = keep = {"theta": [dev(theta), es.empty(n, P)], "parents": [dev(mu[None]), es.empty(1, P)],
                            "m": [dev(m), es.empty(P)], "v": [dev(v), es.empty(P)], "fitness": es.zeros(n),
                            "init": es.zeros(1 if shared else n, E, es.init_dim)}
        st.fitness, st.init = keep["fitness"].data_ptr(), keep["init"].data_ptr()
        for i in (0, 1):
            st.theta[i], st.parents[i] = keep["theta"][i].data_ptr(), keep["parents"][i].data_ptr()
            st.adam_m[i], st.adam_v[i] = keep["m"][i].data_ptr(), keep["v"][i].data_ptr()

    def run(self, k):
        best = self.es.empty(k)
        best.fill_(float("nan"))
        self.es.run_generations(self.st, k, best)
        self.es.sync()
        cur = self.st.cur
        state = {"theta": host(self.keep["theta"][cur]), "mu": host(self.keep["parents"][cur]), "m": host(self.keep["m"][cur]),
                 "v": host(self.keep["v"][cur]), "fitness": host(self.keep["fitness"]), "best": host(best)}
        return state, (self.st.sigma, self.st.pop_sigma, int(self.st.pop_gen), int(self.st.adam_t)), self.es.launch_counts()

    def close(self):
        self.es.close()


GENS = 4


def generations(n, E, fused, **kw):
    out = {}
    for knob in (1, 0):
        r = Run(n, E, knob, fused, **kw)
        try:
            out[knob] = r.run(GENS)
        finally:
            r.close()
    what = f"n={n} E={E} fused_perturb_rollout={fused} {kw}: rollout_heavy_packed 1 vs 0"
    for name in ("fitness", "best", "mu", "m", "v", "theta"):
        assert_bit_equal(out[1][0][name], out[0][0][name], f"{what}: {name}")
    assert out[1][1] == out[0][1], (what, out[1][1], out[0][1])
    # every generation ran a pair kernel; with the prologue (fused = 1) all but the first of the call -- where the tail is eligible
    # for it, which test_gpu_fused_perturb_rollout.py establishes for E = 4, 5, 8; the E = 2 populations (more than 8192 rows) take
    # whichever the tail allows, the same under both knob values
    assert out[1][2] == out[0][2], (what, out[1][2], out[0][2])
    counts = out[1][2]
    print(f"{what}: launch counts {counts}")
    assert counts[0] == GENS, (what, counts)
    if E != 2:
        assert counts[1] == (GENS - 1 if fused else 0), (what, counts)
    else:
        assert counts[1] in ((0, GENS - 1) if fused else (0,)), (what, counts)
    return out[1][0]


GEN_SHAPES = [(4096, 5, True), (4096, 5, False), (10240, 2, True), (8193, 2, False), (2560, 8, False), (3277, 5, True),
              (3700, 5, False)]


@pytest.mark.parametrize("fused", [1, 0], ids=["prologue", "plain"])
@pytest.mark.parametrize("n,E,shared", GEN_SHAPES, ids=[f"n{n}-E{E}-{'shared' if s else 'own'}" for n, E, s in GEN_SHAPES])
def test_generations(n, E, shared, fused):
    state = generations(n, E, fused, shared=shared)
    fit = state["fitness"]
    print(f"n={n} E={E} fused={fused}: fitness min {fit.min()} mean {fit.mean():.1f} max {fit.max()}")
    assert len(np.unique(fit)) > 1, "the returns should not all tie"


@pytest.mark.parametrize("fused", [1, 0], ids=["prologue", "plain"])
def test_generations_with_masked_observations(fused):
    generations(4096, 5, fused, pomdp=True)
