"""The plan is what runs: where ses_rollout_plan says "pair", one rollout raises ses_launch_counts' pair_rollouts by exactly one, and
by nothing elsewhere.  CartPole MLP with max_step 8, so that even the pair kernel's smallest population -- 16 385 envs -- is a
sub-millisecond launch; the returns are held to the C oracle on the way."""
import numpy as np
import pytest
import torch

from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

EPISODIC, FIXED = 0, 1
MAX_STEP = 8
# (n_rows, E, mode): the benchmark population in both modes, a pure split, the pair kernel's smallest population
CASES = [(4096, 5, FIXED), (4096, 5, EPISODIC), (3072, 5, FIXED), (16385, 1, FIXED)]


def one_rollout(n_rows, E, mode, **knobs):
    """(the plan's family, what pair_rollouts and perturb_rollouts rose by) of one rollout on a handle of its own"""
    from ses import HipES
    rng = np.random.RandomState(n_rows + E + mode)
    theta = (rng.randn(n_rows, 226) * 0.6).astype(np.float32)
    init = rng.uniform(-0.05, 0.05, (n_rows, E, 4)).astype(np.float32)
    es = HipES("CartPole-v1", 4, 2, True, False, max_step=MAX_STEP, eval_ep_num=E)
    try:
        for name, value in knobs.items():
            es.set_tuning(name, value)
        before = es.launch_counts()
        fit = es.rollout(torch.from_numpy(theta).cuda(), torch.from_numpy(init).cuda(), mode=mode)
        es.sync()
        after = es.launch_counts()
        family = es.rollout_plan(n_rows, mode, **knobs).family
    finally:
        es.close()
    want = co.rollout_cartpole(theta, init, E, MAX_STEP, mode=mode)[0]
    assert np.array_equal(fit.cpu().numpy(), want), "the returns differ from the oracle"
    return family, after[0] - before[0], after[1] - before[1]


@pytest.mark.parametrize("n_rows, E, mode", CASES, ids=[f"n{n}-E{E}-{'fixed' if m else 'episodic'}" for n, E, m in CASES])
def test_the_pair_kernel_runs_exactly_where_the_plan_says(n_rows, E, mode):
    from ses import _lib
    family, pair_rollouts, perturb_rollouts = one_rollout(n_rows, E, mode)
    # (the host suite pins which of them the plan calls a pair: tests/test_rollout_plan_host.py)
    assert family == {(4096, 5, FIXED): _lib.PLAN_CARTPOLE_MLP_PAIR, (4096, 5, EPISODIC): _lib.PLAN_CARTPOLE_MLP_MIX,
                      (3072, 5, FIXED): _lib.PLAN_CARTPOLE_MLP_PURE, (16385, 1, FIXED): _lib.PLAN_CARTPOLE_MLP_PAIR}[(n_rows, E, mode)]
    assert pair_rollouts == (1 if family == _lib.PLAN_CARTPOLE_MLP_PAIR else 0)
    assert perturb_rollouts == 0


def test_a_knob_on_the_handle_and_in_the_plan_say_the_same():
    from ses import _lib
    family, pair_rollouts, perturb_rollouts = one_rollout(4096, 5, FIXED, rollout_heavy_prio_steps=0)
    assert family == _lib.PLAN_CARTPOLE_MLP_MIX and pair_rollouts == 0 and perturb_rollouts == 0
