"""The checker of the recurrent simple_spread rollout (tests/spread_gru_np.py) against the C oracle, and the evidence that the
inputs of the GPU tests can see the two faults such a rollout typically has."""
import numpy as np
import pytest

from oracle import c_oracle as co

import spread_gru_np as sg


@pytest.mark.parametrize("n_agents", [2, 3])
def test_the_checker_without_gru_is_the_oracle_rollout(n_agents):
    rng = np.random.RandomState(10 + n_agents)
    n, E = 12, 3
    theta = (rng.randn(n, co.param_count(6 * n_agents, 5, False)) * rng.choice([0.2, 1.0, 3.0], size=(n, 1))).astype(np.float32)
    init = co.init_states_uniform(7, 3, 100, n, E, 4 * n_agents, False, -1.0, 1.0)
    for rows, cycles in ((init, 25), (init[0], 10)):                   # per-offspring and shared resets
        fit, ep = sg.rollout(theta, rows, E, n_agents, cycles, gru=False)
        o_fit, o_ep = co.rollout_spread(theta, rows, E, n_agents, cycles)
        assert np.array_equal(ep.view(np.uint64), o_ep.view(np.uint64))
        assert np.array_equal(fit.view(np.uint32), o_fit.view(np.uint32))


@pytest.mark.parametrize("n_agents", [2, 3])
def test_the_gpu_population_sees_shared_and_kept_hidden_states(n_agents):
    """One hidden state for all agents, or hidden states kept across the episode boundary, must change most returns of the
    population the GPU tests use -- otherwise a kernel with either fault would pass them."""
    n, E = 40, 3
    theta, init = sg.population(n_agents, n, E)
    _, want = sg.rollout(theta, init, E, n_agents)
    _, shared = sg.rollout(theta, init, E, n_agents, shared_hidden=True)
    _, kept = sg.rollout(theta, init, E, n_agents, keep_hidden=True)
    d_shared = int((shared.view(np.uint64) != want.view(np.uint64)).sum())
    d_kept = int((kept[:, 1:].view(np.uint64) != want[:, 1:].view(np.uint64)).sum())
    print(f"n_agents={n_agents}: shared hidden changes {d_shared}/{n * E} returns, kept hidden {d_kept}/{n * (E - 1)} of episodes >= 1")
    assert np.array_equal(kept[:, 0].view(np.uint64), want[:, 0].view(np.uint64))     # episode 0 starts from zeros either way
    assert d_shared > n * E // 2
    assert d_kept > n * (E - 1) // 2
