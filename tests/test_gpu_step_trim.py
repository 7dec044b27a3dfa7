"""The fused CartPole MLP rollouts find their tanh entries by byte offset (csrc/ses_math.h tanh_offset_scaled, the staged form in
csrc/ses_policy_pk.h): returns and episode lengths against the C oracle, bit for bit.

The oracle converts the pre-activation to an integer index, so equality is the proof that the offset names the same entry at the
same fraction.  The populations are made so that envs die at every age and, in fixed-length mode, step on past their end for
hundreds of steps beside live lanes of the same wave, with states that sit on the clamps of the physics: a hand-made balancer with
sigma = 0.3 around it -- about a third of its episodes end before step 50, a third in 50 .. 499 and a quarter at the cap (asserted
below on the oracle's own output) -- and sigma = 1.0 around the zero network, where nearly every episode is over by step 50.
(The same cases were written for a step without those clamps, which measured slower and is not in the tree: NOTES.md, round 13.)

Every form the launcher has runs the same rows: lone waves at 16 / 8 / 4 lanes per env, scalar and packed; the mix; the pair kernel
with its heavy wave packed and scalar, with and without the hand-over; the prologue form inside ses_run_generations.  Fixed length and
episodic, fully observed and with the velocities masked.  The oracle runs once per (population, E, mode, mask); a form that needs
fewer rows compares a prefix (the resets are shared, so a row's result depends on nothing but the row).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

T = 500
P = 226
FIXED, EPISODIC = 1, 0
ORACLE_MODE = {FIXED: co.MODE_FIXED_LENGTH, EPISODIC: co.MODE_EPISODIC}
MASK = 0b1010                                # POMDP CartPole hides the two velocities
N_SMALL = 256                                # rows of the lone-wave cases
N_PAIR = {5: 1640, 2: 4100}                  # 8200 envs: with "rollout_waves8" = 512 the mix / pair kernels' range is 8193 .. 10 240
WAVES = 512


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()        # (the shared inputs are read-only arrays: hand torch a copy)


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


def balancer():
    mean = np.zeros(P, np.float32)
    mean[:4] = [0.1, 0.5, 3.0, 1.0]          # hidden unit 0 reads 0.1 x + 0.5 xd + 3 th + thd
    mean[160] = -1.0                         # W2[0][0]
    mean[192] = 1.0                          # W2[1][0]: action 1 follows the unit's sign
    return mean


@functools.lru_cache(maxsize=None)
def population(kind):
    """all the rows any case needs; a case takes a prefix"""
    n = max(N_PAIR.values())
    if kind == "balancer":
        theta = co.perturb(balancer()[None], None, 0.3, 1, 0, 0, n)
    else:
        theta = co.perturb(np.zeros((1, P), np.float32), None, 1.0, 1, 0, 0, n)
    theta.setflags(write=False)
    return theta


@functools.lru_cache(maxsize=None)
def resets():
    init = np.random.RandomState(0).uniform(-0.05, 0.05, (5, 4)).astype(np.float32)
    init.setflags(write=False)
    return init


@functools.lru_cache(maxsize=None)
def oracle(kind, n, E, mode, mask):
    """(fitness, ep_return, ep_steps) of the first n rows; computed once per key and never written to"""
    out = co.rollout_cartpole(population(kind)[:n], resets()[:E], E, T, mode=ORACLE_MODE[mode], obs_mask=mask)
    for a in out:
        a.setflags(write=False)
    return out


# rows the oracle evaluates per (population, E, mode, mask): the mix / pair kernels' populations where a case runs them, else N_SMALL
FULL = {("balancer", 5, FIXED, 0): N_PAIR[5], ("balancer", 5, FIXED, MASK): N_PAIR[5], ("balancer", 5, EPISODIC, 0): N_PAIR[5],
        ("balancer", 5, EPISODIC, MASK): N_PAIR[5], ("balancer", 2, FIXED, 0): N_PAIR[2]}


def want_rows(kind, n, E, mode, mask):
    """the oracle's rows [0, n), from the one run of the key, so that no row is evaluated twice"""
    full = FULL.get((kind, E, mode, mask), N_SMALL)
    assert n <= full, (n, full)
    return tuple(a[:n] for a in oracle(kind, full, E, mode, mask))


def gpu_rollout(kind, n, E, mode, mask, lanes=0, tuning=(), pair=None):
    from ses import HipES
    h = HipES("CartPole-v1", 4, 2, True, False, pomdp=bool(mask), max_step=T, eval_ep_num=E, lanes_per_env=lanes)
    try:
        for name, value in tuning:
            h.set_tuning(name, value)
        fit, ep_ret, ep_steps = h.rollout(dev(population(kind)[:n]), dev(resets()[:E]), mode=mode, want_episodes=True)
        out = host(fit), host(ep_ret), host(ep_steps)
        if pair is not None:
            assert h.launch_counts()[0] == (1 if pair else 0), ("pair kernel launches", h.launch_counts(), pair)
        return out
    finally:
        h.close()


def compare(kind, n, E, mode, mask, what, **kw):
    got = gpu_rollout(kind, n, E, mode, mask, **kw)
    want = want_rows(kind, n, E, mode, mask)
    for i, name in enumerate(("fitness", "ep_return", "ep_steps")):
        assert_bit_equal(got[i], want[i], f"{what}: {name} vs the oracle")
    return got


def classes(ep_steps):
    s = np.asarray(ep_steps).reshape(-1)
    return np.array([(s < 50).mean(), ((s >= 50) & (s < T)).mean(), (s >= T).mean()])


# ---- what the inputs are worth -------------------------------------------------------------------------------------------------

def test_the_balancer_population_dies_at_every_age():
    """the test's own precondition, on the oracle's output: at least 20 % of the episodes end before step 50, in 50 .. 499, and
    at the cap; otherwise no dead lane runs on beside a live one and the comparisons below prove nothing"""
    fit, _, ep_steps = want_rows("balancer", N_SMALL, 5, FIXED, 0)
    share = classes(ep_steps)
    print(f"balancer, {N_SMALL} rows x 5: early / middle / cap = {share.round(3)}, {len(np.unique(fit))} distinct fitness values")
    assert (share >= 0.20).all(), share
    share0 = classes(want_rows("zero", N_SMALL, 5, FIXED, 0)[2])
    print(f"zero network, sigma 1: early / middle / cap = {share0.round(3)}")
    assert share0[0] >= 0.80, share0


# ---- lone waves ------------------------------------------------------------------------------------------------------------------

LONE = [(16, 0), (16, 1), (8, 0), (8, 1), (4, 0)]         # (lanes per env, "rollout_packed"); 4 lanes per env has no packed lone form


@pytest.mark.parametrize("mask", [0, MASK], ids=["observed", "masked"])
@pytest.mark.parametrize("mode", [FIXED, EPISODIC], ids=["fixed", "episodic"])
@pytest.mark.parametrize("E", [5, 2])
@pytest.mark.parametrize("lanes,packed", LONE, ids=[f"lpe{l}-{'packed' if p else 'scalar'}" for l, p in LONE])
def test_lone_waves(lanes, packed, E, mode, mask):
    for kind in ("balancer", "zero"):
        compare(kind, N_SMALL, E, mode, mask, f"{kind} lpe={lanes} packed={packed} E={E} mode={mode} mask={mask}", lanes=lanes,
                tuning=(("rollout_packed", packed),))


# ---- the mix and the pair kernels --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask", [0, MASK], ids=["observed", "masked"])
@pytest.mark.parametrize("mode", [FIXED, EPISODIC], ids=["fixed", "episodic"])
def test_mix(mode, mask):
    """16 lanes per env on the first waves, 4 on the rest, as single-wave workgroups: episodic populations of the pair kernel's size,
    and fixed-length ones with the priority and the hand-over off"""
    tuning = (("rollout_waves8", WAVES), ("rollout_heavy_prio_steps", 0), ("rollout_handover_step", 1 << 20))
    compare("balancer", N_PAIR[5], 5, mode, mask, f"mix, mode={mode}, mask={mask}", tuning=tuning, pair=False)


PAIRS = [(1, 1 << 20), (0, 1 << 20), (1, 137), (0, 137)]  # ("rollout_heavy_packed", "rollout_handover_step")


@pytest.mark.parametrize("mask", [0, MASK], ids=["observed", "masked"])
@pytest.mark.parametrize("heavy_packed,handover", PAIRS, ids=[f"{'packed' if p else 'scalar'}-{'handover' if s < T else 'whole'}"
                                                               for p, s in PAIRS])
def test_pair_kernel(heavy_packed, handover, mask):
    got = compare("balancer", N_PAIR[5], 5, FIXED, mask, f"pairs heavy_packed={heavy_packed} handover={handover} mask={mask}",
                  tuning=(("rollout_waves8", WAVES), ("rollout_heavy_packed", heavy_packed), ("rollout_handover_step", handover)),
                  pair=True)
    share = classes(got[2])
    print(f"pairs heavy_packed={heavy_packed} handover={handover} mask={mask}: early / middle / cap = {share.round(3)}")


def test_pair_kernel_two_episodes():
    compare("balancer", N_PAIR[2], 2, FIXED, 0, "pairs, E = 2", tuning=(("rollout_waves8", WAVES),), pair=True)


# ---- the prologue form: one ses_run_generations call -------------------------------------------------------------------------------

def test_device_loop_prologue_form_against_the_update_launch():
    """three generations in one call at the headline's shape: the prologue form of the pair kernel (knob 1) against rows read from
    theta behind k_es_apply_perturb (knob 0), on the bits of fitness, best, mu, m, v and theta -- the protocol of
    test_gpu_prologue_rows.py"""
    import test_gpu_fused_perturb_rollout as fpr
    out = fpr.both_knobs(4096, 5, [3])
    assert out[1][1] == (3, 2, 1), out[1][1]
    assert out[0][1] == (3, 0, 3), out[0][1]
    assert len(np.unique(out[1][0]["fitness"])) > 1, "the returns should not all tie"


# ---- saturation and exact zeros ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [0, 16, 8, 4])
def test_saturated_and_zero_preactivations(lanes):
    """first layer times 64: pre-activations pass the table's end (|x| >= 10 reads the last entry at the clamped fraction); units
    whose weights are all zero read entry 0 at fraction 0"""
    n = 64
    theta = population("balancer")[:n].copy()
    theta[:, :160] *= 64.0                                   # W1 (32 x 4) and b1
    w1, b1 = theta[:, :128].reshape(n, 32, 4), theta[:, 128:160]
    w1[n // 2:, 8:16] = 0.0
    b1[n // 2:, 8:16] = 0.0
    from ses import HipES
    for mode in (FIXED, EPISODIC):
        want = co.rollout_cartpole(theta, resets(), 5, T, mode=ORACLE_MODE[mode], obs_mask=0)
        h = HipES("CartPole-v1", 4, 2, True, False, max_step=T, eval_ep_num=5, lanes_per_env=lanes)
        try:
            got = h.rollout(dev(theta), dev(resets()), mode=mode, want_episodes=True)
            for i, name in enumerate(("fitness", "ep_return", "ep_steps")):
                assert_bit_equal(host(got[i]), want[i], f"saturated, lanes={lanes} mode={mode}: {name} vs the oracle")
        finally:
            h.close()
    assert len(np.unique(want[0])) > 1, "the returns should not all tie"
