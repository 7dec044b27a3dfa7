"""The (16, 4) mixed CartPole MLP split with a hand-over (k_rollout_cartpole_mlp_handover, fixed-length mode).

At 16 385 ... 20 480 envs every SIMD runs one light wave (16 lanes per env) and one heavy wave (4 lanes per env); the heavy
wave hands half of its envs to the light wave at step `rollout_handover_step` and both finish at 8 lanes per env.  The state
crosses as raw bits and every lanes-per-env form evaluates the same canonical arithmetic, so ep_return / ep_steps must be the
bits of the schedule without a hand-over (rollout_handover_step >= max_step) and of the C oracle, whatever the step.  The heavy
wave's s_setprio (rollout_heavy_prio_steps, what the default actually uses) changes only the order of issue."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

FIXED = 1


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def population(n, E, seed, scale=0.6):
    rng = np.random.RandomState(seed)
    theta = (rng.randn(n, 226) * scale).astype(np.float32)
    init = rng.uniform(-0.05, 0.05, (n, E, 4)).astype(np.float32)
    return theta, init


def run(theta, init, E, max_step, handover=None, pomdp=False, prio_steps=None):
    from ses import HipES
    h = HipES("CartPole-v1", 4, 2, True, False, pomdp=pomdp, max_step=max_step, eval_ep_num=E)
    try:
        if handover is not None:
            h.set_tuning("rollout_handover_step", handover)
        if prio_steps is not None:
            h.set_tuning("rollout_heavy_prio_steps", prio_steps)
        fit, ep_ret, ep_steps = h.rollout(dev(theta), dev(init), mode=FIXED, want_episodes=True)
        return host(fit), host(ep_ret), host(ep_steps)
    finally:
        h.close()


def assert_same(got, want, what):
    for g, w, name in zip(got, want, ("fitness", "ep_return", "ep_steps")):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.ascontiguousarray(g).view(np.uint8) != np.ascontiguousarray(w).view(np.uint8)
        assert not bad.any(), f"{what}: {name} differs in {int(bad.sum())} bytes"


def oracle(theta, init, E, max_step, obs_mask=0):
    return co.rollout_cartpole(theta, init, E, max_step, mode=co.MODE_FIXED_LENGTH, obs_mask=obs_mask)


@pytest.fixture(scope="module")
def headline():
    theta, init = population(4096, 5, 7)
    return theta, init, oracle(theta, init, 5, 500)


@pytest.mark.parametrize("handover", [0, 1, 137, None, 499, 500])
def test_headline_population_any_handover_step(headline, handover):
    """4096 offspring x 5 episodes x 500 steps, hand-over at the first step, the last one, off and the default (off)."""
    theta, init, want = headline
    assert_same(run(theta, init, 5, 500, handover), want, f"handover={handover}")


def test_handover_off_is_the_old_schedule(headline):
    theta, init, _ = headline
    assert_same(run(theta, init, 5, 500, 190), run(theta, init, 5, 500, 1 << 20), "190 vs off")


@pytest.mark.parametrize("prio_steps,handover", [(0, 1 << 20), (1, 1 << 20), (250, 1 << 20), (499, 1 << 20), (0, 137), (300, 137),
                                                 (300, 400)])
def test_heavy_priority_steps(headline, prio_steps, handover):
    """The heavy wave's first prio_steps steps at s_setprio 1 (all of them by default): a matter of speed only.  (0, off) is
    the plain mix kernel; with a hand-over the priority covers at most the first phase."""
    theta, init, want = headline
    assert_same(run(theta, init, 5, 500, handover, prio_steps=prio_steps), want, f"prio_steps={prio_steps} handover={handover}")


@pytest.mark.parametrize("max_step,handover", [(1, 0), (1, 1), (2, 0), (2, 1), (2, 2)])
def test_tiny_horizons(max_step, handover):
    theta, init = population(4096, 5, 11)
    assert_same(run(theta, init, 5, max_step, handover), oracle(theta, init, 5, max_step), f"{max_step}/{handover}")


@pytest.mark.parametrize("handover", [0, 60, 199])
def test_pomdp_mask(handover):
    theta, init = population(4096, 5, 13)
    want = oracle(theta, init, 5, 200, obs_mask=0b1010)
    assert_same(run(theta, init, 5, 200, handover, pomdp=True), want, f"pomdp handover={handover}")


@pytest.mark.parametrize("wild_side", ["light", "heavy"])
def test_wild_initial_state_in_one_wave_of_a_pair(wild_side):
    """One env outside the small-angle range: its wave (light: envs 0-4095, heavy: the rest) runs the general loop; in the
    heavy case both phase-2 waves of that pair must run it too, while every other wave keeps the shortcut."""
    theta, init = population(4096, 5, 17)
    env = 5 if wild_side == "light" else 4096 + 16 * 3 + 11          # heavy: pair 3, an env the light wave takes over
    init[env // 5, env % 5, 2] = 1.5
    init[env // 5, env % 5, 3] = -60.0
    want = oracle(theta, init, 5, 300)
    for handover in (0, 100, 299):
        assert_same(run(theta, init, 5, 300, handover), want, f"{wild_side} handover={handover}")


@pytest.mark.parametrize("n,E", [(3277, 5), (3500, 5), (4000, 5), (16385, 1), (18000, 1), (20480, 1)])
def test_population_edges_of_the_mix(n, E):
    """16 385 ... 20 480 envs take the (16, 4) mix: ragged last heavy waves (3277 x 5: one env in the last one), pairs without a
    heavy wave, a single episode per offspring."""
    theta, init = population(n, E, n + E)
    want = oracle(theta, init, E, 120)
    for handover in (None, 0, 57):
        assert_same(run(theta, init, E, 120, handover), want, f"n={n} E={E} handover={handover}")


def test_shared_initial_states():
    """init_per_offspring = 0: one set of E initial states for every offspring."""
    from ses import HipES
    theta, init = population(4096, 5, 19)
    shared = init[0]
    want = co.rollout_cartpole(theta, shared, 5, 150, mode=co.MODE_FIXED_LENGTH)
    h = HipES("CartPole-v1", 4, 2, True, False, max_step=150, eval_ep_num=5)
    try:
        h.set_tuning("rollout_handover_step", 40)
        fit, ep_ret, ep_steps = h.rollout(dev(theta), dev(shared), mode=FIXED, want_episodes=True)
        assert_same((host(fit), host(ep_ret), host(ep_steps)), want, "shared init")
    finally:
        h.close()
