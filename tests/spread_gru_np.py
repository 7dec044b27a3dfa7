"""The reference's simple_spread rollout with one policy copy per agent, stated as a Python loop over the C oracle's pieces
(oracle/c_oracle.py: spread_obs, spread_step, policy_forward).  It imports no product code.

For offspring row theta[P] and every episode: the init row [4 NA] is agent positions then landmark positions, velocities zero;
every agent a gets its own hidden state h_a[32] = 0 (GymEnvModel.reset() of its deep copy).  Each cycle t < max_cycles every agent
observes the state BEFORE the step, one policy forward on (obs_a, h_a) updates h_a and gives the 5 logits, the action is their
first argmax; then the world steps once and the team reward is added, ret += (double)r, in cycle order.  fitness is the episode
mean, summed in double in episode order and rounded to float32.

Oracle state layout: float32[6 NA] = positions, velocities, landmarks.

shared_hidden / keep_hidden exist for the sensitivity test only: ONE hidden state that the agents update in turn, and hidden
states that survive the episode boundary -- the two ways a recurrent multi-agent rollout typically goes wrong."""
import numpy as np

from oracle import c_oracle as co

HIDDEN = 32


def population(n_agents, n, E):
    """The inputs of the GPU tests: theta float32[n, P] = randn x one of {0.2, 1.0, 3.0} per row (seed = n_agents), and the reset rows
    float32[n, E, 4 NA] that ses_init_states_uniform(seed 7, generation 3, first row 100) draws in U(-1, 1)."""
    rng = np.random.RandomState(n_agents)
    P = co.param_count(6 * n_agents, 5, True)
    theta = (rng.randn(n, P) * rng.choice([0.2, 1.0, 3.0], size=(n, 1))).astype(np.float32)
    init = co.init_states_uniform(7, 3, 100, n, E, 4 * n_agents, False, -1.0, 1.0)
    return theta, init


def rollout(theta, init, E, n_agents, max_cycles=25, *, gru=True, shared_hidden=False, keep_hidden=False):
    """theta float32[N, P]; init float32[E, 4 NA] (shared) or [N, E, 4 NA].  Returns (fitness float32[N], ep_return float64[N, E])."""
    theta = np.atleast_2d(np.ascontiguousarray(theta, dtype=np.float32))
    init = np.ascontiguousarray(init, dtype=np.float32)
    N, NA, S = theta.shape[0], n_agents, 6 * n_agents
    assert init.shape[-2:] == (E, 4 * NA) and (init.ndim == 2 or init.shape[0] == N), init.shape
    ep_return = np.empty((N, E), np.float64)
    fitness = np.empty(N, np.float32)
    n_h = 1 if shared_hidden else NA
    for i in range(N):
        row = theta[i:i + 1]
        h = np.zeros((n_h, HIDDEN), np.float32)
        total = 0.0
        for ep in range(E):
            u = init[i, ep] if init.ndim == 3 else init[ep]
            state = np.zeros(6 * NA, np.float32)
            state[:2 * NA] = u[:2 * NA]
            state[4 * NA:] = u[2 * NA:]
            if not keep_hidden:
                h[:] = 0.0
            ret = 0.0
            for _ in range(max_cycles):
                action = np.empty(NA, np.int32)
                for a in range(NA):                                   # every agent sees the state before the step
                    obs = co.spread_obs(NA, state, a)
                    k = 0 if shared_hidden else a
                    act, _, _, h_next = co.policy_forward(S, 5, True, gru, row, obs[None, :], h[k:k + 1] if gru else None)
                    if gru:
                        h[k] = h_next[0]
                    action[a] = act[0]
                ret += float(np.float32(co.spread_step(NA, state, action)))
            ep_return[i, ep] = ret
            total += ret
        fitness[i] = np.float32(total / float(E))
    return fitness, ep_return
