"""LunarLander-v2 rollouts composed from the existing oracle only -- the yardstick of the discrete lander's tests.

Per episode: LanderSim.reset(16 uniforms), mask the observation, c_oracle.policy_forward(8, 4, discrete, gru, ...), take the action
table, LanderSim.step(a0, a1); the return accumulates in a Python float, the episode ends on `done` or at max_step, and
fitness = float32(total / E).  With discrete=False the harness feeds act[0], act[1] instead and must then equal
c_oracle.rollout_lander bit for bit (tests/test_lander_discrete_host.py), which is what makes it a reference.

gym 0.18-0.21 lunar_lander.py, continuous=False: 0 = no-op, 1 = left orientation engine, 2 = main engine, 3 = right orientation
engine; the continuous env computes exactly the discrete env's engine powers for these inputs."""
import numpy as np

from oracle import c_oracle as co

ACTION_TABLE = np.array([[0.0, 0.0], [0.0, -1.0], [1.0, 0.0], [0.0, 1.0]], np.float32)
POMDP_MASK = 0b101100                     # obs 2, 3, 5


def population(gru, pomdp, n, E):
    """theta[n, P], init[n, E, 16]: the generator of tests/test_gpu_lander.py"""
    rng = np.random.RandomState(2 * int(gru) + int(pomdp))
    P = co.param_count(8, 4, gru)
    theta = (rng.randn(n, P) * rng.choice([0.05, 0.3, 1.0], size=(n, 1))).astype(np.float32)
    init = co.init_states_uniform(11, 2, 50, n, E, 16, False, 0.0, 1.0)
    return theta, init


def episode(sim, theta_row, u16, max_step, gru, obs_mask, discrete=True, trace=None):
    """(return as a Python float, steps); trace: a list that receives (action or None, reward) per step"""
    obs = sim.reset(u16)
    h, total, steps, done = None, 0.0, 0, False
    while steps < max_step and not done:
        o = obs.copy()
        for k in range(8):
            if (obs_mask >> k) & 1:
                o[k] = 0.0
        action, _logits, act, h = co.policy_forward(8, 4, discrete, gru, theta_row, o, h)
        if discrete:
            a0, a1 = ACTION_TABLE[int(action[0])]
        else:
            a0, a1 = act[0, 0], act[0, 1]
        obs, r, done = sim.step(float(a0), float(a1))
        total += r
        steps += 1
        if trace is not None:
            trace.append((int(action[0]) if discrete else None, r))
    return total, steps


def rollout(theta, init, E, max_step, gru, obs_mask, discrete=True):
    """(fitness[N] f32, ep_return[N, E] f64, ep_steps[N, E] i32, action histogram[4]) -- init is [N, E, 16]"""
    N = theta.shape[0]
    ep_ret = np.zeros((N, E), np.float64)
    ep_steps = np.zeros((N, E), np.int32)
    fit = np.zeros(N, np.float32)
    hist = np.zeros(4, np.int64)
    sim = co.LanderSim()
    for n in range(N):
        total = 0.0
        for e in range(E):
            trace = []
            ep_ret[n, e], ep_steps[n, e] = episode(sim, theta[n], init[n, e], max_step, gru, obs_mask, discrete, trace)
            total += ep_ret[n, e]
            if discrete:
                hist += np.bincount([a for a, _ in trace], minlength=4)
        fit[n] = np.float32(total / E)
    return fit, ep_ret, ep_steps, hist


_cache = {}


def reference(gru, pomdp, E, n=22, max_step=120):
    """the harness result of the tests' population, computed once per (gru, pomdp, E) and handed out read-only"""
    key = (bool(gru), bool(pomdp), E, n, max_step)
    if key not in _cache:
        theta, init = population(gru, pomdp, n, E)
        out = (theta, init) + rollout(theta, init, E, max_step, gru, POMDP_MASK if pomdp else 0)
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]
