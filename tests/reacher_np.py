"""Independent numpy float64 restatement of ReacherBulletEnv-v0 as DESIGN.md 7 defines it (the build's own two-link arm
modelled on pybullet's Reacher), vectorised over envs.  It imports no product code: sin / cos come from classic_control_np (the
numpy port of the library's fma-free float64 routine), squares are x * x, np.sqrt is the correctly rounded square root, and
every other operation is one correctly rounded IEEE add, sub, mul, div or compare in the order DESIGN.md 7 writes it.  The
actions are the policy's float32 tanh outputs widened to float64; rewards are float64.  `step` takes dt and the damping as
parameters (the device has the constants only) so that tests/test_reacher_host.py can watch the energy error shrink with dt on
the undamped arm.

The state is float64[7, n]: th, w1, g, w2, target x, target y, pot."""
import numpy as np

from classic_control_np import sincos

DT = 0.0165
L1, L2 = 0.1, 0.11
M1, M2 = 0.0356, 0.0393
LC1, LC2 = 0.05, 0.055
I1 = (M1 * (L1 * L1)) / 12.0
I2 = (M2 * (L2 * L2)) / 12.0
ARMATURE = 0.002
DAMPING = 0.01
TORQUE = 0.05
LIMIT = 3.0
PI = 3.141592653589793
TARGET = 0.27
CA = (M2 * L1) * LC2
C2A = 2.0 * CA
M12C = I2 + M2 * (LC2 * LC2)
M11C = (((I1 + I2) + M1 * (LC1 * LC1)) + M2 * (L1 * L1 + LC2 * LC2)) + ARMATURE
M22 = M12C + ARMATURE
R22 = 1.0 / M22
S, A, INIT_DIM, INIT_RANGE, STATE_DIM, TIME_LIMIT = 9, 2, 4, (-1.0, 1.0), 7, 150


def clip(x, lo, hi):
    """min(max(x, lo), hi)"""
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def _action(a):
    """float32[n, 2] -> two float64[n]: the widened, clipped float32 actions"""
    a = np.asarray(a, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    return clip(a[:, 0], -1.0, 1.0), clip(a[:, 1], -1.0, 1.0)


def trig(s):
    """(st, ct, sg, cg, sb, cb): sin / cos of th, g and, by the addition formulas, of th + g"""
    st, ct = sincos(s[0])
    sg, cg = sincos(s[2])
    return st, ct, sg, cg, st * cg + ct * sg, ct * cg - st * sg


def to_target(s, tr):
    """fingertip - target"""
    st, ct, _, _, sb, cb = tr
    return (L1 * ct + L2 * cb) - s[4], (L1 * st + L2 * sb) - s[5]


def potential(s, tr):
    dx, dy = to_target(s, tr)
    return -100.0 * np.sqrt(dx * dx + dy * dy)


def obs_of(s):
    tr = trig(s)
    dx, dy = to_target(s, tr)
    return np.stack([s[4], s[5], dx, dy, tr[1], tr[0], s[1], s[2], s[3]], axis=1).astype(np.float32)


def limit(g, w2):
    """g clipped to [-3, 3]; where it was clipped, a rate pointing outward becomes 0"""
    hi, lo = g > LIMIT, g < -LIMIT
    w2 = np.where(hi & (w2 > 0.0), 0.0, w2)
    w2 = np.where(lo & (w2 < 0.0), 0.0, w2)
    return np.where(hi, LIMIT, np.where(lo, -LIMIT, g)), w2


def step(s, a, dt=DT, damping=DAMPING):
    """s: float64[7, n], a: float32[n, 2] -> (s', obs float32[n, 9], reward float64[n], done[n] (never))"""
    th, w1, g, w2, tx, ty, pot = np.asarray(s, dtype=np.float64)
    a0, a1 = _action(a)
    _, _, sg, cg, _, _ = trig(s)
    tau1, tau2 = TORQUE * a0, TORQUE * a1
    m11 = M11C + C2A * cg
    m12 = M12C + CA * cg
    h = CA * sg
    b1 = (tau1 - damping * w1) + h * ((2.0 * w1) * w2 + w2 * w2)
    b2 = (tau2 - damping * w2) - h * (w1 * w1)
    m = m12 * R22
    e11, f1 = m11 - m * m12, b1 - m * b2
    acc1 = f1 / e11
    acc2 = (b2 - m12 * acc1) * R22
    w1 = w1 + dt * acc1
    w2 = w2 + dt * acc2
    th = th + dt * w1
    g = g + dt * w2
    g, w2 = limit(g, w2)
    ns = np.stack([th, w1, g, w2, tx, ty, pot])
    new_pot = potential(ns, trig(ns))
    r = new_pot - pot
    r = r - 0.10 * (np.abs(a0 * w1) + np.abs(a1 * w2))
    r = r - 0.01 * (np.abs(a0) + np.abs(a1))
    r = np.where(np.abs(np.abs(g) - 1.0) < 0.01, r - 0.1, r)
    ns[6] = new_pot
    return ns, obs_of(ns), r, np.zeros(ns.shape[1], bool)


def reset(init):
    """init: float32[n, 4] uniforms in (-1, 1) -> float64[7, n]: target = 0.27 (u0, u1), th = pi u2, g = 3 u3, rates 0"""
    u = np.asarray(init, dtype=np.float32).astype(np.float64)
    z = np.zeros_like(u[:, 0])
    s = np.stack([PI * u[:, 2], z, LIMIT * u[:, 3], z, TARGET * u[:, 0], TARGET * u[:, 1], z])
    s[6] = potential(s, trig(s))
    return s


def kinetic_energy(s):
    """From first principles: each rod's centre-of-mass translation plus its rotation about the centre, plus the armature
    (a rotor inertia J on each joint coordinate: J w1^2 / 2 + J w2^2 / 2)."""
    th, w1, g, w2 = s[0], s[1], s[2], s[3]
    b, wb = th + g, w1 + w2
    v1x, v1y = -LC1 * w1 * np.sin(th), LC1 * w1 * np.cos(th)
    v2x = -L1 * w1 * np.sin(th) - LC2 * wb * np.sin(b)
    v2y = L1 * w1 * np.cos(th) + LC2 * wb * np.cos(b)
    return (0.5 * M1 * (v1x * v1x + v1y * v1y) + 0.5 * (M1 * L1 ** 2 / 12.0) * w1 * w1 +
            0.5 * M2 * (v2x * v2x + v2y * v2y) + 0.5 * (M2 * L2 ** 2 / 12.0) * wb * wb +
            0.5 * ARMATURE * w1 * w1 + 0.5 * ARMATURE * w2 * w2)


def rollout(theta, init, E, max_step, policy, on_step=None):
    """Host loop of the fused rollout: theta[N, P], init[N or 1, E, 4]; policy(theta_rows, obs, h) -> (act float32[n, 2], h')
    (h: the GRU's hidden state, None for an MLP).  Returns (fitness float32[N], ep_return float64[N, E], ep_steps int32[N, E])
    with the kernels' accumulation: the return is the float64 sum of the float64 rewards in step order, every episode is
    max_step steps, fitness = (sum over the episodes in order) / E in float64, cast to float32.  on_step(new_states) sees every
    transition."""
    N = theta.shape[0]
    init = np.broadcast_to(init, (N, E, init.shape[-1])).reshape(N * E, -1)
    rows = np.repeat(np.arange(N), E)
    s = reset(init)
    obs = obs_of(s)
    h = None
    ret = np.zeros(N * E)
    for _ in range(max_step):
        act, h = policy(theta[rows], obs, h)
        s, obs, r, _ = step(s, act)
        if on_step is not None:
            on_step(s)
        ret = ret + r
    ep_ret = ret.reshape(N, E)
    fit = np.zeros(N)
    for e in range(E):
        fit = fit + ep_ret[:, e]
    return (fit / E).astype(np.float32), ep_ret, np.full((N, E), max_step, np.int32)
