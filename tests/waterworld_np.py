"""waterworld restated in numpy float64 -- the yardstick of the waterworld tests (DESIGN.md 7 is the specification).

Independent of the product: it imports no product code and takes from the oracle only `policy_forward`, `philox_raw` and
`init_states_uniform`.  Every operation is an elementwise + - * /, np.sqrt or a comparison (np.where / argmin select, they do not
compute): one correctly rounded IEEE operation each, in the order the specification writes them -- no np.dot, @, linalg.norm,
hypot or multi-term float sum, which may contract or reorder.  The state of B envs is held side by side ([B, 20] arrays: objects
0..4 pursuers, 5..9 evaders, 10..19 poisons); the envs never interact.  `counts` tallies what happened, so that the tests can
assert that their inputs reach every branch.
"""
import numpy as np

from oracle import c_oracle as co

N_PURSUERS, N_EVADERS, N_POISONS, N_OBJ = 5, 5, 10, 20
N_SENSORS, OBS, INIT_W, MAX_CYCLES = 30, 242, 72, 500
P = 32 * OBS + 32 + 2 * 32 + 2
R = 0.015
R_EV = 2.0 * R
R_PO = 0.75 * R
R_OB = 0.2
SPEED = 0.01
MAX_ACCEL = 0.01
L = 0.2
TOUCH_EV = (3.0 * R) * (3.0 * R)
TOUCH_PO = (1.75 * R) * (1.75 * R)
FOOD, ENCOUNTER, POISON, THRUST = 10.0, 0.01, -1.0, -0.5
PHILOX_TAG = 0x57415452
RADIUS = np.array([R] * N_PURSUERS + [R_EV] * N_EVADERS + [R_PO] * N_POISONS, np.float64)

# (cos, sin)(k * (6.283185307179586 / 30.0)) as hex floats: the table is the definition, the same literals as csrc/ses_waterworld.h
SENSOR_HEX = [
    ("0x1.0000000000000p+0", "0x0.0p+0"),
    ("0x1.f4cfc327a0080p-1", "0x1.a9cd9ac4258f5p-3"),
    ("0x1.d3bc3aeff7f95p-1", "0x1.a07f921061ad0p-2"),
    ("0x1.9e3779b97f4a8p-1", "0x1.2cf2304755a5ep-1"),
    ("0x1.5698496e20bd8p-1", "0x1.7c7d7a833bec1p-1"),
    ("0x1.0000000000001p-1", "0x1.bb67ae8584caap-1"),
    ("0x1.3c6ef372fe950p-2", "0x1.e6f0e134454ffp-1"),
    ("0x1.ac2609b3c577bp-4", "0x1.fd31f94f867c6p-1"),
    ("-0x1.ac2609b3c5762p-4", "0x1.fd31f94f867c7p-1"),
    ("-0x1.3c6ef372fe94ep-2", "0x1.e6f0e13445500p-1"),
    ("-0x1.ffffffffffffcp-2", "0x1.bb67ae8584cabp-1"),
    ("-0x1.5698496e20bd5p-1", "0x1.7c7d7a833bec4p-1"),
    ("-0x1.9e3779b97f4a7p-1", "0x1.2cf2304755a5fp-1"),
    ("-0x1.d3bc3aeff7f94p-1", "0x1.a07f921061ad5p-2"),
    ("-0x1.f4cfc327a007fp-1", "0x1.a9cd9ac425904p-3"),
    ("-0x1.0000000000000p+0", "0x1.1a62633145c07p-53"),
    ("-0x1.f4cfc327a0080p-1", "-0x1.a9cd9ac4258ecp-3"),
    ("-0x1.d3bc3aeff7f97p-1", "-0x1.a07f921061acap-2"),
    ("-0x1.9e3779b97f4a9p-1", "-0x1.2cf2304755a5dp-1"),
    ("-0x1.5698496e20bdap-1", "-0x1.7c7d7a833bec0p-1"),
    ("-0x1.0000000000004p-1", "-0x1.bb67ae8584ca8p-1"),
    ("-0x1.3c6ef372fe952p-2", "-0x1.e6f0e134454ffp-1"),
    ("-0x1.ac2609b3c57a3p-4", "-0x1.fd31f94f867c6p-1"),
    ("0x1.ac2609b3c5749p-4", "-0x1.fd31f94f867c7p-1"),
    ("0x1.3c6ef372fe94cp-2", "-0x1.e6f0e13445500p-1"),
    ("0x1.ffffffffffff4p-2", "-0x1.bb67ae8584caep-1"),
    ("0x1.5698496e20bd4p-1", "-0x1.7c7d7a833bec5p-1"),
    ("0x1.9e3779b97f4a7p-1", "-0x1.2cf2304755a60p-1"),
    ("0x1.d3bc3aeff7f92p-1", "-0x1.a07f921061adep-2"),
    ("0x1.f4cfc327a007fp-1", "-0x1.a9cd9ac425909p-3"),
]
SENSORS = np.array([[float.fromhex(c), float.fromhex(s)] for c, s in SENSOR_HEX], np.float64)

EVENTS = ("catches", "lone_touches", "poison_touches", "wall_clips", "wall_bounces", "obstacle_rebounds", "tries_refused",
          "reset_respawns")


def _clip01(x):
    return np.where(x < 0.0, 0.0, np.where(x > 1.0, 1.0, x))


def _direction(u, v, speed):
    dx, dy = u - 0.5, v - 0.5
    n = np.sqrt(dx * dx + dy * dy)
    with np.errstate(all="ignore"):
        ox = np.where(n == 0.0, speed, (dx / n) * speed)
        oy = np.where(n == 0.0, 0.0, (dy / n) * speed)
    return ox, oy


def _clear(x, y, rho):
    dx, dy, lim = x - 0.5, y - 0.5, R_OB + rho
    return dx * dx + dy * dy > lim * lim


class Waterworld:
    """B independent envs; init: float32[B, 72]"""

    def __init__(self, init, counts=None):
        init = np.ascontiguousarray(init, np.float32).reshape(-1, INIT_W)
        B = self.B = init.shape[0]
        self.counts = counts if counts is not None else dict.fromkeys(EVENTS, 0)
        u = init.astype(np.float64)
        self.px, self.py = np.zeros((B, N_OBJ)), np.zeros((B, N_OBJ))
        self.vx, self.vy = np.zeros((B, N_OBJ)), np.zeros((B, N_OBJ))
        self.px[:, :N_PURSUERS] = u[:, 0:10:2]
        self.py[:, :N_PURSUERS] = u[:, 1:10:2]
        o = u[:, 10:70].reshape(B, N_EVADERS + N_POISONS, 4)
        self.px[:, N_PURSUERS:], self.py[:, N_PURSUERS:] = o[:, :, 0], o[:, :, 1]
        self.vx[:, N_PURSUERS:], self.vy[:, N_PURSUERS:] = _direction(o[:, :, 2], o[:, :, 3], SPEED)
        self.key = init[:, 70:72].copy().view(np.uint32)
        self.ctr = np.zeros(B, np.uint32)
        self.touch_ev = np.zeros((B, N_PURSUERS), bool)
        self.touch_po = np.zeros((B, N_PURSUERS), bool)
        for i in range(N_OBJ):
            for b in np.nonzero(~_clear(self.px[:, i], self.py[:, i], RADIUS[i]))[0]:
                self.counts["reset_respawns"] += 1
                self._respawn(b, i)

    def _respawn(self, b, i):
        rho = RADIUS[i]
        ok = False
        for t in range(8):
            w = co.philox_raw([self.ctr[b], t, 0, PHILOX_TAG], self.key[b])
            u = (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
            ok = bool(_clear(u[0], u[1], rho))
            if ok:
                break
            self.counts["tries_refused"] += 1
        self.px[b, i] = u[0] if ok else u[0] * 0.25
        self.py[b, i] = u[1] if ok else u[1] * 0.25
        if i >= N_PURSUERS:
            self.vx[b, i], self.vy[b, i] = _direction(u[2], u[3], SPEED)
        self.ctr[b] += np.uint32(1)

    def _rebound(self, i, rho):
        px, py, vx, vy = self.px[:, i], self.py[:, i], self.vx[:, i], self.vy[:, i]
        dx, dy = px - 0.5, py - 0.5
        dist = np.sqrt(dx * dx + dy * dy)
        lim = rho + R_OB
        hit = dist <= lim
        scale = lim - dist
        qx, qy = px + scale * dx, py + scale * dy
        nx, ny = qx - 0.5, qy - 0.5
        with np.errstate(all="ignore"):
            k = (vx * nx + vy * ny) / (nx * nx + ny * ny)
        projx, projy = k * nx, k * ny
        perpx, perpy = vx - projx, vy - projy
        self.px[:, i], self.py[:, i] = np.where(hit, qx, px), np.where(hit, qy, py)
        self.vx[:, i], self.vy[:, i] = np.where(hit, perpx - projx, vx), np.where(hit, perpy - projy, vy)
        self.counts["obstacle_rebounds"] += int(hit.sum())

    def step(self, action):
        """action: float32[B, 5, 2], already scaled by float32(0.001).  Returns the team reward float64[B]."""
        action = np.asarray(action, np.float32).reshape(self.B, N_PURSUERS, 2)
        thrust = np.zeros((self.B, N_PURSUERS))
        for a in range(N_PURSUERS):
            ax, ay = action[:, a, 0].astype(np.float64), action[:, a, 1].astype(np.float64)
            m = np.sqrt(ax * ax + ay * ay)
            big = m > MAX_ACCEL
            with np.errstate(all="ignore"):
                ax, ay = np.where(big, (ax / m) * MAX_ACCEL, ax), np.where(big, (ay / m) * MAX_ACCEL, ay)
            m = np.where(big, np.sqrt(ax * ax + ay * ay), m)
            self.vx[:, a] = self.vx[:, a] + ax
            self.vy[:, a] = self.vy[:, a] + ay
            self.px[:, a] = self.px[:, a] + self.vx[:, a]
            self.py[:, a] = self.py[:, a] + self.vy[:, a]
            thrust[:, a] = THRUST * m
            for p, v in ((self.px, self.vx), (self.py, self.vy)):
                lo, hi = p[:, a] < 0.0, p[:, a] > 1.0
                p[:, a] = np.where(lo, 0.0, np.where(hi, 1.0, p[:, a]))
                v[:, a] = np.where(lo | hi, 0.0, v[:, a])
                self.counts["wall_clips"] += int((lo | hi).sum())
            self._rebound(a, R)
        for i in range(N_PURSUERS, N_OBJ):
            self.px[:, i] = self.px[:, i] + self.vx[:, i]
            self.py[:, i] = self.py[:, i] + self.vy[:, i]
            for p, v in ((self.px, self.vx), (self.py, self.vy)):
                hi = p[:, i] >= 1.0
                lo = ~hi & (p[:, i] <= 0.0)
                p[:, i] = np.where(hi, 1.0, np.where(lo, 0.0, p[:, i]))
                v[:, i] = np.where(hi | lo, -v[:, i], v[:, i])
                self.counts["wall_bounces"] += int((hi | lo).sum())
            self._rebound(i, RADIUS[i])
        ev, po = slice(N_PURSUERS, N_PURSUERS + N_EVADERS), slice(N_PURSUERS + N_EVADERS, N_OBJ)
        cx, cy = self.px[:, :N_PURSUERS, None], self.py[:, :N_PURSUERS, None]
        dx, dy = cx - self.px[:, None, ev], cy - self.py[:, None, ev]
        tev = dx * dx + dy * dy <= TOUCH_EV                                   # [B, pursuer, evader]
        dx, dy = cx - self.px[:, None, po], cy - self.py[:, None, po]
        tpo = dx * dx + dy * dy <= TOUCH_PO                                   # [B, pursuer, poison]
        caught = np.count_nonzero(tev, axis=1) >= 2                           # [B, evader]
        nc = np.count_nonzero(tev & caught[:, None, :], axis=2).astype(np.float64)
        ne = np.count_nonzero(tev, axis=2).astype(np.float64)
        npo = np.count_nonzero(tpo, axis=2).astype(np.float64)
        r = ((thrust + FOOD * nc) + ENCOUNTER * ne) + POISON * npo
        team = (((r[:, 0] + r[:, 1]) + r[:, 2]) + r[:, 3]) + r[:, 4]
        poisoned = tpo.any(axis=1)                                            # [B, poison]
        self.counts["catches"] += int(caught.sum())
        self.counts["lone_touches"] += int((tev.any(axis=1) & ~caught).sum())
        self.counts["poison_touches"] += int(poisoned.sum())
        self.touch_ev, self.touch_po = ne > 0.0, npo > 0.0
        for b, e in np.argwhere(caught):
            self._respawn(b, N_PURSUERS + e)
        for b, j in np.argwhere(poisoned):
            self._respawn(b, N_PURSUERS + N_EVADERS + j)
        return team

    def _sense(self, first, count, rho, skip_self):
        """(distance feature, speed feature) [B, pursuer, sensor] of the nearest seen object of [first, first + count)"""
        idx = slice(first, first + count)
        cx, cy = self.px[:, :N_PURSUERS, None, None], self.py[:, :N_PURSUERS, None, None]
        wx, wy = self.vx[:, :N_PURSUERS, None, None], self.vy[:, :N_PURSUERS, None, None]
        skx, sky = SENSORS[None, None, :, 0, None], SENSORS[None, None, :, 1, None]
        relx, rely = self.px[:, None, None, idx] - cx, self.py[:, None, None, idx] - cy
        proj = skx * relx + sky * rely                                        # [B, pursuer, sensor, object]
        seen = (proj >= 0.0) & (proj - rho <= L) & ((relx * relx + rely * rely) - proj * proj <= rho * rho)
        if skip_self:
            seen &= ~np.eye(N_PURSUERS, dtype=bool)[None, :, None, :]
        masked = np.where(seen, proj, np.inf)
        who = np.argmin(masked, axis=3)[..., None]                            # the first minimum: a tie goes to the lower index
        best = np.take_along_axis(masked, who, 3)[..., 0]
        any_seen = seen.any(axis=3)
        with np.errstate(all="ignore"):
            d = best / L
        dist = np.where(any_seen, np.where(1.0 < d, 1.0, d), 1.0)
        ovx = np.take_along_axis(np.broadcast_to(self.vx[:, None, None, idx], proj.shape), who, 3)
        ovy = np.take_along_axis(np.broadcast_to(self.vy[:, None, None, idx], proj.shape), who, 3)
        speed = (skx * (ovx - wx) + sky * (ovy - wy))[..., 0]
        return dist, np.where(any_seen, speed, 0.0)

    def observe(self):
        """float32[B, 5, 242]"""
        B = self.B
        cx, cy = self.px[:, :N_PURSUERS, None], self.py[:, :N_PURSUERS, None]
        skx, sky = SENSORS[None, None, :, 0], SENSORS[None, None, :, 1]
        f = np.zeros((B, N_PURSUERS, N_SENSORS, 8))
        relx, rely = 0.5 - cx, 0.5 - cy
        proj = skx * relx + sky * rely
        seen = (proj >= 0.0) & (proj - R_OB <= L) & ((relx * relx + rely * rely) - proj * proj <= R_OB * R_OB)
        d = proj / L
        f[..., 0] = np.where(seen, np.where(1.0 < d, 1.0, d), 1.0)
        lx, ly = skx * L, sky * L
        vecx, vecy = _clip01(cx + lx) - cx, _clip01(cy + ly) - cy
        with np.errstate(all="ignore"):
            ratx = np.where(np.abs(lx) > 1e-8, vecx / lx, 1.0)
            raty = np.where(np.abs(ly) > 1e-8, vecy / ly, 1.0)
        f[..., 1] = _clip01(np.where(raty < ratx, raty, ratx))
        f[..., 2], f[..., 3] = self._sense(N_PURSUERS, N_EVADERS, R_EV, False)
        f[..., 4], f[..., 5] = self._sense(N_PURSUERS + N_EVADERS, N_POISONS, R_PO, False)
        f[..., 6], f[..., 7] = self._sense(0, N_PURSUERS, R, True)
        obs = np.zeros((B, N_PURSUERS, OBS), np.float32)
        obs[:, :, :8 * N_SENSORS] = f.reshape(B, N_PURSUERS, 8 * N_SENSORS).astype(np.float32)
        obs[:, :, 240] = self.touch_ev
        obs[:, :, 241] = self.touch_po
        return obs


def policy_actions(theta_rows, obs):
    """theta_rows float32[B, P] (one row per env), obs float32[B, 5, 242] -> the scaled actions float32[B, 5, 2]: the policy's two
    tanh outputs, each multiplied in float32 by float32(0.001)"""
    B = obs.shape[0]
    th = np.repeat(np.ascontiguousarray(theta_rows, np.float32).reshape(B, P), N_PURSUERS, axis=0)
    _, _, act, _ = co.policy_forward(OBS, 2, False, False, th, obs.reshape(B * N_PURSUERS, OBS))
    return (np.float32(act) * np.float32(0.001)).reshape(B, N_PURSUERS, 2)


def rollout(theta, init, E, max_step, counts=None):
    """theta float32[n, P]; init float32[n, E, 72] or [E, 72] (shared) -> (fitness float32[n], ep_return float64[n, E], counts)"""
    theta = np.ascontiguousarray(theta, np.float32)
    n = theta.shape[0]
    init = np.ascontiguousarray(init, np.float32)
    if init.ndim == 2:
        init = np.broadcast_to(init[None], (n, E, INIT_W))
    env = Waterworld(init.reshape(n * E, INIT_W), counts)
    rows = np.repeat(theta, E, axis=0)
    ret = np.zeros(n * E, np.float64)
    for _ in range(min(int(max_step), MAX_CYCLES)):
        ret = ret + env.step(policy_actions(rows, env.observe()))
    ep = ret.reshape(n, E)
    total = np.zeros(n, np.float64)
    for e in range(E):
        total = total + ep[:, e]
    return (total / float(E)).astype(np.float32), ep, env.counts


# ---- the inputs the tests share (tests/test_waterworld_host.py asserts that they reach every event; tests/test_gpu_waterworld.py
# ---- runs the kernels on exactly them) ---------------------------------------------------------------------------------------
def craft(pursuers=(), evaders=(), poisons=()):
    """One init row: everything parked out of everybody's way -- pursuers down the left side, evaders down the right side heading
    up, poisons along the top heading right -- except the objects given as {index: (x, y)} / {index: (x, y, u, v)}."""
    row = np.zeros(INIT_W, np.float32)
    for a in range(N_PURSUERS):
        row[2 * a:2 * a + 2] = (0.05, 0.1 + 0.2 * a)
    for e in range(N_EVADERS):
        row[10 + 4 * e:14 + 4 * e] = (0.95, 0.1 + 0.2 * e, 0.5, 1.0)
    for j in range(N_POISONS):
        row[30 + 4 * j:34 + 4 * j] = (0.15 + 0.07 * j, 0.95, 1.0, 0.5)
    for a, v in dict(pursuers).items():
        row[2 * a:2 * a + 2] = v
    for e, v in dict(evaders).items():
        row[10 + 4 * e:14 + 4 * e] = v
    for j, v in dict(poisons).items():
        row[30 + 4 * j:34 + 4 * j] = v
    row[70:72] = (0.123, 0.456)
    return row


CRAFTED = {
    "catch": craft(pursuers={0: (0.30, 0.10), 1: (0.31, 0.10)}, evaders={0: (0.30, 0.10, 0.5, 1.0)}),
    "lone_touch": craft(pursuers={0: (0.30, 0.10)}, evaders={0: (0.30, 0.10, 0.5, 1.0)}),
    "poison": craft(pursuers={0: (0.30, 0.10)}, poisons={0: (0.30, 0.10, 0.5, 1.0)}),
    "wall_bounce": craft(evaders={0: (0.995, 0.30, 1.0, 0.5)}),
    "obstacle": craft(poisons={0: (0.285, 0.5, 1.0, 0.5)}),
    "wall_clip": craft(pursuers={0: (0.001, 0.30)}),
    "in_obstacle": craft(pursuers={2: (0.5, 0.45)}, evaders={1: (0.55, 0.5, 0.2, 0.9)}, poisons={3: (0.4, 0.6, 0.7, 0.1)}),
}


def crafted_rows():
    return np.stack(list(CRAFTED.values()))


def thetas(n, seed):
    """randn x {0.2, 1, 3} per row"""
    rng = np.random.RandomState(seed)
    return (rng.randn(n, P) * rng.choice([0.2, 1.0, 3.0], size=(n, 1))).astype(np.float32)


STEPWISE_CYCLES = 40


def stepwise_inputs():
    """(init[15, 72], theta[15, P]): the crafted rows and 8 random ones, a policy each"""
    rows = np.concatenate([crafted_rows(), co.init_states_uniform(5, 1, 0, 8, 1, INIT_W, False, 0.0, 1.0)[:, 0]])
    return rows, thetas(rows.shape[0], 21)


# (E, n, max_step, one init row set per offspring): a partial tile, the reference's 5, a full tile, one episode past it, three tiles;
# 1, 3 and 70 offspring; 1, 12 and 40 cycles; none above 2 000 env-cycles
FUSED_CASES = [(1, 70, 12, True), (5, 3, 40, True), (6, 1, 40, False), (7, 3, 12, True), (13, 3, 40, True), (5, 70, 1, False),
               (13, 1, 1, True), (5, 3, 12, False)]


def fused_inputs(E, n, max_step, per):
    theta = thetas(n, 100 * E + n)
    init = co.init_states_uniform(7, E, 3, n if per else 1, E, INIT_W, False, 0.0, 1.0)
    flat = init.reshape(-1, INIT_W)
    crafted = crafted_rows()
    for i in range(min(len(crafted), (flat.shape[0] + 1) // 2)):            # every second (offspring, episode) slot, while they last
        flat[2 * i] = crafted[(i + E) % len(crafted)]
    return theta, (init if per else init[0])


_cache = {}


def fused_reference(case):
    """(theta, init, fitness, ep_return, counts) of a case, computed once and handed out read-only"""
    if case not in _cache:
        E, n, max_step, per = case
        assert E * n * min(max_step, MAX_CYCLES) <= 2000
        theta, init = fused_inputs(*case)
        fit, ep, counts = rollout(theta, init, E, max_step)
        for a in (theta, init, fit, ep):
            a.setflags(write=False)
        _cache[case] = (theta, init, fit, ep, dict(counts))
    return _cache[case]


def stepwise_reference():
    """(init, theta, obs[T + 1][B, 5, 242], actions[T][B, 5, 2], reward[T][B] float32, counts): reset and STEPWISE_CYCLES policy cycles"""
    if "stepwise" not in _cache:
        init, theta = stepwise_inputs()
        env = Waterworld(init)
        obs, acts, rews = [env.observe()], [], []
        for _ in range(STEPWISE_CYCLES):
            acts.append(policy_actions(theta, obs[-1]))
            rews.append(env.step(acts[-1]).astype(np.float32))
            obs.append(env.observe())
        _cache["stepwise"] = (init, theta, obs, acts, rews, dict(env.counts))
    return _cache["stepwise"]
