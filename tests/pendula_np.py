"""Independent numpy float64 restatement of the inverted-pendulum family modelled on pybullet_envs (InvertedPendulumBulletEnv-v0,
InvertedPendulumSwingupBulletEnv-v0, InvertedDoublePendulumBulletEnv-v0), written from the equations of DESIGN.md 7 and
vectorised over envs.  It imports no product code: sin / cos come from classic_control_np (the numpy port of the library's
fma-free float64 routine), squares are x * x, and every other operation is one correctly rounded IEEE add, sub, mul, div or
compare in the order DESIGN.md 7 writes it.  The action is the policy's float32 tanh output widened to float64; rewards are
float64.  `step` takes dt as a parameter (the device has the constant only) so that tests/test_pendula_host.py can watch the
energy error shrink with it, and `force` to switch the motor off."""
import numpy as np

from classic_control_np import sincos

DT = 0.0165
G = 9.8
CART_M = 10.472
FOUR_THIRDS = 4.0 / 3.0

# the single pendulum
POLE_M = 5.0186
POLE_L = 0.3                                          # half-length
TOTAL_M = CART_M + POLE_M
POLE_ML = POLE_M * POLE_L

# the double pendulum
ROD_M = 4.1987
ROD_LEN = 0.6
ROD_L = 0.3                                           # half-length
D1 = (CART_M + ROD_M) + ROD_M
D2 = (FOUR_THIRDS * ROD_M) * (ROD_L * ROD_L) + ROD_M * (ROD_LEN * ROD_LEN)
D3 = (FOUR_THIRDS * ROD_M) * (ROD_L * ROD_L)
D4 = ROD_M * ROD_L + ROD_M * ROD_LEN
D5 = ROD_M * ROD_L
D6 = (ROD_M * ROD_LEN) * ROD_L
R1 = 1.0 / D1


def clip(x, lo, hi):
    """min(max(x, lo), hi)"""
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def _action(a):
    """float32[n] or float32[n, 1] -> float64[n]: the widened float32 action"""
    return np.asarray(a, dtype=np.float32).reshape(-1).astype(np.float64)


def rail(x, v):
    """x clipped to [-1, 1]; where it was clipped, a velocity pointing outward becomes 0"""
    hi, lo = x > 1.0, x < -1.0
    v = np.where(hi & (v > 0.0), 0.0, v)
    v = np.where(lo & (v < 0.0), 0.0, v)
    x = np.where(hi, 1.0, np.where(lo, -1.0, x))
    return x, v


# ---- the single pendulum (balance and swing-up share the transition) ---------------------------------------------------------
def pole_obs(s):
    sn, cs = sincos(s[2])
    return np.stack([s[0], s[1], cs, sn, s[3]], axis=1).astype(np.float32)


def pole_transition(s, a, dt=DT, force=100.0):
    x, v, th, w = np.asarray(s, dtype=np.float64)
    f = force * clip(_action(a), -1.0, 1.0)
    sn, cs = sincos(th)
    temp = (f + (POLE_ML * (w * w)) * sn) / TOTAL_M
    thacc = (G * sn - cs * temp) / (POLE_L * (FOUR_THIRDS - (POLE_M * (cs * cs)) / TOTAL_M))
    xacc = temp - ((POLE_ML * thacc) * cs) / TOTAL_M
    v = v + dt * xacc
    w = w + dt * thacc
    x = x + dt * v
    th = th + dt * w
    x, v = rail(x, v)
    return np.stack([x, v, th, w])


def balance_step(s, a, dt=DT, force=100.0):
    """s: float64[4, n] (x, v, theta, omega), a: float32[n] or [n, 1] -> (s', obs float32[n, 5], reward float64[n], done[n])"""
    ns = pole_transition(s, a, dt, force)
    done = (ns[2] > 0.2) | (ns[2] < -0.2)
    return ns, pole_obs(ns), np.ones(ns.shape[1]), done


def swingup_step(s, a, dt=DT, force=100.0):
    ns = pole_transition(s, a, dt, force)
    return ns, pole_obs(ns), sincos(ns[2])[1], np.zeros(ns.shape[1], bool)


def balance_reset(init):
    """init: float32[n, 1] uniforms in (-0.1, 0.1) -> float64[4, n]: theta = u, everything else 0"""
    u = np.asarray(init, dtype=np.float32)[:, 0].astype(np.float64)
    z = np.zeros_like(u)
    return np.stack([z, z, u, z])


def swingup_reset(init):
    u = np.asarray(init, dtype=np.float32)[:, 0].astype(np.float64)
    z = np.zeros_like(u)
    return np.stack([z, z, 3.1415 + u, z])


# ---- the double pendulum -------------------------------------------------------------------------------------------------------
def double_trig(s):
    """(s1, c1, s2, c2, sb, cb): sin / cos of theta1, theta2 and, by the addition formulas, of beta = theta1 + theta2"""
    s1, c1 = sincos(s[2])
    s2, c2 = sincos(s[4])
    return s1, c1, s2, c2, s1 * c2 + c1 * s2, c1 * c2 - s1 * s2


def double_tip(s, tr):
    """(x2, y2): the centre of the second rod"""
    s1, c1, _, _, sb, cb = tr
    return (s[0] + ROD_LEN * s1) + ROD_L * sb, ROD_LEN * c1 + ROD_L * cb


def double_obs(s):
    tr = double_trig(s)
    s1, c1, s2, c2, _, _ = tr
    x2, _ = double_tip(s, tr)
    return np.stack([s[0], s[1], x2, c1, s1, s[3], c2, s2, s[5]], axis=1).astype(np.float32)


def double_step(s, a, dt=DT, force=200.0):
    """s: float64[6, n] (x, v, theta1, omega1, theta2, omega2) -> (s', obs float32[n, 9], reward float64[n], done[n])"""
    x, v, th1, w1, th2, w2 = np.asarray(s, dtype=np.float64)
    f = force * clip(_action(a), -1.0, 1.0)
    s1, c1, s2, c2, sb, cb = double_trig(s)
    wa, wb = w1, w1 + w2
    wa2, wb2 = wa * wa, wb * wb
    a12, a13, a23 = D4 * c1, D5 * cb, D6 * c2
    b1 = (f + (D4 * wa2) * s1) + (D5 * wb2) * sb
    b2 = (G * D4) * s1 + (D6 * wb2) * s2
    b3 = (G * D5) * sb - (D6 * wa2) * s2
    m2, m3 = a12 * R1, a13 * R1
    e22, e23, f2 = D2 - m2 * a12, a23 - m2 * a13, b2 - m2 * b1
    e33, f3 = D3 - m3 * a13, b3 - m3 * b1
    r2 = 1.0 / e22
    m32 = e23 * r2
    g33, h3 = e33 - m32 * e23, f3 - m32 * f2
    bacc = h3 / g33
    aacc = (f2 - e23 * bacc) * r2
    xacc = ((b1 - a12 * aacc) - a13 * bacc) * R1
    v = v + dt * xacc
    w1 = w1 + dt * aacc
    w2 = w2 + dt * (bacc - aacc)
    x = x + dt * v
    th1 = th1 + dt * w1
    th2 = th2 + dt * w2
    x, v = rail(x, v)
    ns = np.stack([x, v, th1, w1, th2, w2])
    x2, y2 = double_tip(ns, double_trig(ns))
    h = y2 + 0.3
    d = h - 2.0
    reward = (10.0 - 0.01 * (x2 * x2)) - d * d
    return ns, double_obs(ns), reward, h <= 1.0


def double_reset(init):
    """init: float32[n, 2] uniforms in (-0.1, 0.1) -> float64[6, n]: theta1 = u0, theta2 = u1, everything else 0"""
    u = np.asarray(init, dtype=np.float32).astype(np.float64)
    z = np.zeros_like(u[:, 0])
    return np.stack([z, z, u[:, 0], z, u[:, 1], z])


ENVS = {
    "InvertedPendulumBulletEnv-v0": dict(reset=balance_reset, step=balance_step, obs=pole_obs, S=5, A=1, init_dim=1,
                                         init_range=(-0.1, 0.1), state_dim=4, time_limit=1000, terminates=True),
    "InvertedPendulumSwingupBulletEnv-v0": dict(reset=swingup_reset, step=swingup_step, obs=pole_obs, S=5, A=1, init_dim=1,
                                                init_range=(-0.1, 0.1), state_dim=4, time_limit=1000, terminates=False),
    "InvertedDoublePendulumBulletEnv-v0": dict(reset=double_reset, step=double_step, obs=double_obs, S=9, A=1, init_dim=2,
                                               init_range=(-0.1, 0.1), state_dim=6, time_limit=1000, terminates=True),
}


def rollout(name, theta, init, E, max_step, policy, on_step=None):
    """Host loop of the fused rollout: theta[N, P], init[N or 1, E, W]; policy(theta_rows, obs, h) -> (act float32[n, 1], h')
    on the envs still running (h: the GRU's hidden state of those envs, None for an MLP).  Returns (fitness float32[N],
    ep_return float64[N, E], ep_steps int32[N, E]) with the kernels' accumulation: the return is the float64 sum of the
    float64 rewards in step order, a finished env is frozen, fitness = (sum over the episodes in order) / E in float64, cast
    to float32.  on_step(live, new_states) sees every transition."""
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
        if on_step is not None:
            on_step(live, ns)
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
