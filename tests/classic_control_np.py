"""Independent numpy float64 restatement of Acrobot-v1 and MountainCar-v0 (gym 0.21, classic_control) in gym's order of
operations, vectorised over envs.  It imports no product code: the sin / cos are a numpy port of the library's
fma-free float64 routine (Cephes polynomials, three-part Cody-Waite reduction by pi/2), and every other operation is a
correctly rounded IEEE add, sub, mul, div or compare in the order Python evaluates gym's expressions.  numpy evaluates
each array operation element by element with one rounding, so the device's transitions are reproduced bit for bit."""
import numpy as np

TWO_OVER_PI = float.fromhex("0x1.45f306dc9c883p-1")
PIO2_1 = float.fromhex("0x1.921fb544p+0")
PIO2_2 = float.fromhex("0x1.0b4611a6p-34")
PIO2_3 = float.fromhex("0x1.3198a2e037073p-69")
SIN_COEF = (1.58962301576546568060E-10, -2.50507477628578072866E-8, 2.75573136213857245213E-6,
            -1.98412698295895385996E-4, 8.33333333332211858878E-3, -1.66666666666666307295E-1)
COS_COEF = (-1.13585365213876817300E-11, 2.08757008419747316778E-9, -2.75573141792967388112E-7,
            2.48015872888517045348E-5, -1.38888888888730564116E-3, 4.16666666666665929218E-2)


def sincos(x):
    """(sin x, cos x) of a float64 array, operation for operation as csrc/ses_classic.h sincos_ieee."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        k = np.rint(x * TWO_OVER_PI)
        r = x - k * PIO2_1
        r = r - k * PIO2_2
        r = r - k * PIO2_3
        z = r * r
        ps = np.full_like(z, SIN_COEF[0])
        for c in SIN_COEF[1:]:
            ps = ps * z + c
        s = r + r * (z * ps)
        pc = np.full_like(z, COS_COEF[0])
        for c in COS_COEF[1:]:
            pc = pc * z + c
        c = (1.0 - 0.5 * z) + (z * z) * pc
        kc = np.clip(np.nan_to_num(k, nan=0.0), -1.0e9, 1.0e9)
        q = kc.astype(np.int64) & 3
    sv = np.where(q & 1, c, s)
    cv = np.where(q & 1, s, c)
    return np.where(q & 2, -sv, sv), np.where((q + 1) & 2, -cv, cv)


def cos(x):
    return sincos(x)[1]


# ---- Acrobot-v1 ------------------------------------------------------------------------------------------------------------
AC_DT = 0.2
M1 = M2 = L1 = I1 = I2 = 1.0
LC1 = LC2 = 0.5
G = 9.8
PI = np.pi
MAX_VEL_1, MAX_VEL_2 = 4 * PI, 9 * PI
AVAIL_TORQUE = np.array([-1.0, 0.0, 1.0])


def acrobot_dsdt(th1, th2, w1, w2, a):
    s2, c2 = sincos(th2)
    d1 = M1 * LC1 ** 2 + M2 * (L1 ** 2 + LC2 ** 2 + 2 * L1 * LC2 * c2) + I1 + I2
    d2 = M2 * (LC2 ** 2 + L1 * LC2 * c2) + I2
    phi2 = M2 * LC2 * G * cos(th1 + th2 - PI / 2.)
    phi1 = - M2 * L1 * LC2 * w2 ** 2 * s2 - 2 * M2 * L1 * LC2 * w2 * w1 * s2 + (M1 * LC1 + M2 * L1) * G * cos(th1 - PI / 2) + phi2
    dd2 = (a + d2 / d1 * phi1 - M2 * L1 * LC2 * w1 ** 2 * s2 - phi2) / (M2 * LC2 ** 2 + I2 - d2 ** 2 / d1)
    dd1 = -(d1 * dd2 + phi1) / d1
    return np.stack([w1, w2, dd1, dd2])


def wrap(x, m=-PI, M=PI):
    x = np.array(x, dtype=np.float64)
    diff = M - m
    for _ in range(4096):
        hi = x > M
        if not hi.any():
            break
        x = np.where(hi, x - diff, x)
    for _ in range(4096):
        lo = x < m
        if not lo.any():
            break
        x = np.where(lo, x + diff, x)
    return x


def bound(x, m, M):
    return np.where(x < m, m, np.where(x > M, M, x))


def acrobot_terminal(s):
    return -cos(s[0]) - cos(s[1] + s[0]) > 1.0


def acrobot_step(s, a):
    """s: float64[4, n] (theta1, theta2, dtheta1, dtheta2), a: int[n] -> (s', obs float32[n, 6], reward float32[n], done[n])."""
    s = np.asarray(s, dtype=np.float64)
    tau = AVAIL_TORQUE[np.clip(np.asarray(a), 0, 2)]
    dt = AC_DT - 0
    dt2 = dt / 2.0
    y0 = s
    k1 = acrobot_dsdt(*y0, tau)
    k2 = acrobot_dsdt(*(y0 + dt2 * k1), tau)
    k3 = acrobot_dsdt(*(y0 + dt2 * k2), tau)
    k4 = acrobot_dsdt(*(y0 + dt * k3), tau)
    y = y0 + dt / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    ns = np.stack([wrap(y[0]), wrap(y[1]), bound(y[2], -MAX_VEL_1, MAX_VEL_1), bound(y[3], -MAX_VEL_2, MAX_VEL_2)])
    done = acrobot_terminal(ns)
    reward = np.where(done, 0.0, -1.0).astype(np.float32)
    return ns, acrobot_obs(ns), reward, done


def acrobot_obs(s):
    s1, c1 = sincos(s[0])
    s2, c2 = sincos(s[1])
    return np.stack([c1, s1, c2, s2, s[2], s[3]], axis=1).astype(np.float32)


def acrobot_reset(init):
    """init: float32[n, 4] -> float64[4, n]"""
    return np.asarray(init, dtype=np.float32).astype(np.float64).T.copy()


# ---- MountainCar-v0 --------------------------------------------------------------------------------------------------------
FORCE, GRAVITY, MAX_SPEED = 0.001, 0.0025, 0.07
MIN_POS, MAX_POS, GOAL_POS, GOAL_VEL = -1.2, 0.6, 0.5, 0


def mountaincar_step(s, a):
    """s: float64[2, n] (position, velocity), a: int[n] -> (s', obs float32[n, 2], reward float32[n], done[n])."""
    p, v = np.asarray(s, dtype=np.float64)
    a = np.clip(np.asarray(a), 0, 2)
    v = v + ((a - 1) * FORCE + cos(3 * p) * (-GRAVITY))
    v = bound(v, -MAX_SPEED, MAX_SPEED)
    p = p + v
    p = bound(p, MIN_POS, MAX_POS)
    v = np.where((p == MIN_POS) & (v < 0), 0.0, v)
    done = (p >= GOAL_POS) & (v >= GOAL_VEL)
    ns = np.stack([p, v])
    return ns, mountaincar_obs(ns), np.full(p.shape, -1.0, np.float32), done


def mountaincar_obs(s):
    return np.stack([s[0], s[1]], axis=1).astype(np.float32)


def mountaincar_reset(init):
    """init: float32[n, 1] -> float64[2, n] (velocity 0)"""
    p = np.asarray(init, dtype=np.float32)[:, 0].astype(np.float64)
    return np.stack([p, np.zeros_like(p)])


ENVS = {
    "Acrobot-v1": dict(reset=acrobot_reset, step=acrobot_step, obs=acrobot_obs, S=6, A=3, init_dim=4, init_range=(-0.1, 0.1),
                       state_dim=4, time_limit=500),
    "MountainCar-v0": dict(reset=mountaincar_reset, step=mountaincar_step, obs=mountaincar_obs, S=2, A=3, init_dim=1,
                           init_range=(-0.6, -0.4), state_dim=2, time_limit=200),
}


def rollout(name, theta, init, E, max_step, policy):
    """Host loop of the fused rollout: theta[N, P], init[N or 1, E, W]; policy(theta_rows, obs, h) -> (action, h') on the
    envs still running (h: the GRU's hidden state of those envs, None for an MLP).  Returns (fitness float32[N], ep_return
    float64[N, E], ep_steps int32[N, E]) with the kernels' accumulation: the return is a float64 sum of the float32
    rewards, a finished env is frozen, fitness = (sum over the episodes in order) / E in float64, cast to float32."""
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
        action, h = policy(theta[rows[live]], obs[live], h)
        ns, nobs, r, d = env["step"](s[:, live], action)
        s[:, live] = ns
        obs[live] = nobs
        ret[live] = ret[live] + r.astype(np.float64)
        steps[live] += 1
        keep = ~d
        live = live[keep]
        h = None if h is None else h[keep]
    ep_ret = ret.reshape(N, E)
    fit = np.zeros(N)
    for e in range(E):
        fit = fit + ep_ret[:, e]
    return (fit / E).astype(np.float32), ep_ret, steps.reshape(N, E)
