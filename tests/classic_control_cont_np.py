"""Independent numpy float64 restatement of Pendulum-v1 and MountainCarContinuous-v0 (the equations of DESIGN.md 7),
vectorised over envs.  It imports no product code: sin / cos come from classic_control_np (the numpy port of the library's
fma-free float64 routine, held to 2 ulp there), the float mod is np.remainder (Python's %: exact), squares are x * x, and
every other operation is one correctly rounded IEEE add, sub, mul or compare in the written left-to-right order.  The
action is the policy's float32 tanh output widened to float64; rewards are float64."""
import numpy as np

from classic_control_np import cos, sincos

PI = np.pi


def clip(x, lo, hi):
    """min(max(x, lo), hi)"""
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def _action(a):
    """float32[n] or float32[n, 1] -> float64[n]: the widened float32 action"""
    return np.asarray(a, dtype=np.float32).reshape(-1).astype(np.float64)


# ---- Pendulum-v1 -----------------------------------------------------------------------------------------------------------
def pendulum_step(s, a):
    """s: float64[2, n] (theta, dtheta), a: float32[n] or [n, 1] -> (s', obs float32[n, 3], reward float64[n], done[n])."""
    th, w = np.asarray(s, dtype=np.float64)
    a = _action(a)
    u = clip(a, -2.0, 2.0)
    an = np.remainder(th + PI, 2 * PI) - PI
    cost = (an * an + 0.1 * (w * w)) + 0.001 * (u * u)
    w = w + ((15.0 * sincos(th)[0]) + (3.0 * u)) * 0.05
    w = clip(w, -8.0, 8.0)
    th = th + w * 0.05
    ns = np.stack([th, w])
    return ns, pendulum_obs(ns), -cost, np.zeros(th.shape, bool)


def pendulum_obs(s):
    sn, cs = sincos(s[0])
    return np.stack([cs, sn, s[1]], axis=1).astype(np.float32)


def pendulum_reset(init):
    """init: float32[n, 2] uniforms in (-1, 1) -> float64[2, n]: theta = u0 * pi, dtheta = u1"""
    u = np.asarray(init, dtype=np.float32).astype(np.float64)
    return np.stack([u[:, 0] * PI, u[:, 1]])


# ---- MountainCarContinuous-v0 ----------------------------------------------------------------------------------------------
def mountaincar_cont_step(s, a):
    """s: float64[2, n] (position, velocity), a: float32[n] or [n, 1] -> (s', obs float32[n, 2], reward float64[n], done[n]).
    The reward charges the unclipped action; the new state is rounded to float32 and widened again."""
    p, v = np.asarray(s, dtype=np.float64)
    a = _action(a)
    f = clip(a, -1.0, 1.0)
    v = v + (f * 0.0015 - 0.0025 * cos(3.0 * p))
    v = clip(v, -0.07, 0.07)
    p = p + v
    p = clip(p, -1.2, 0.6)
    v = np.where((p == -1.2) & (v < 0), 0.0, v)
    done = (p >= 0.45) & (v >= 0)
    reward = np.where(done, 100.0, 0.0) - (a * a) * 0.1
    ns = np.stack([p.astype(np.float32).astype(np.float64), v.astype(np.float32).astype(np.float64)])
    return ns, mountaincar_cont_obs(ns), reward, done


def mountaincar_cont_obs(s):
    return np.stack([s[0], s[1]], axis=1).astype(np.float32)


def mountaincar_cont_reset(init):
    """init: float32[n, 1] -> float64[2, n] (velocity 0)"""
    p = np.asarray(init, dtype=np.float32)[:, 0].astype(np.float64)
    return np.stack([p, np.zeros_like(p)])


ENVS = {
    "Pendulum-v1": dict(reset=pendulum_reset, step=pendulum_step, obs=pendulum_obs, S=3, A=1, init_dim=2, init_range=(-1.0, 1.0),
                        state_dim=2, time_limit=200),
    "MountainCarContinuous-v0": dict(reset=mountaincar_cont_reset, step=mountaincar_cont_step, obs=mountaincar_cont_obs, S=2, A=1,
                                     init_dim=1, init_range=(-0.6, -0.4), state_dim=2, time_limit=999),
}


def rollout(name, theta, init, E, max_step, policy):
    """Host loop of the fused rollout: theta[N, P], init[N or 1, E, W]; policy(theta_rows, obs, h) -> (act float32[n, 1], h')
    on the envs still running (h: the GRU's hidden state of those envs, None for an MLP).  Returns (fitness float32[N],
    ep_return float64[N, E], ep_steps int32[N, E]) with the kernels' accumulation: the return is the float64 sum of the
    float64 rewards in step order, a finished env is frozen, fitness = (sum over the episodes in order) / E in float64, cast
    to float32."""
    env = ENVS[name]
    N = theta.shape[0]
    init = np.broadcast_to(init, (N, E, init.shape[-1])).reshape(N * E, -1)
    rows = np.repeat(np.arange(N), E)
    s = env["reset"](init)
    obs = env["obs"](s)
    h = None
    ret = np.zeros(N * E)
    steps = np.zeros(N * E, np.int32)
    live = np.arange(N * E)
    for _ in range(max_step):
        if live.size == 0:
            break
        act, h = policy(theta[rows[live]], obs[live], h)
        ns, nobs, r, d = env["step"](s[:, live], act)
        s[:, live] = ns
        obs[live] = nobs
        ret[live] = ret[live] + r
        steps[live] += 1
        keep = ~d
        live = live[keep]
        h = None if h is None else h[keep]
    ep_ret = ret.reshape(N, E)
    fit = np.zeros(N)
    for e in range(E):
        fit = fit + ep_ret[:, e]
    return (fit / E).astype(np.float32), ep_ret, steps.reshape(N, E)
