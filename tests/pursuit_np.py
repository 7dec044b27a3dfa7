"""pursuit restated in numpy -- the yardstick of the pursuit tests (DESIGN.md 7 is the specification).

Independent of the product: it imports no product code and takes from the oracle only `policy_forward`, `philox_raw` and
`init_states_uniform`.  The env is integers; its only floating point is the float64 reward, every operation of which is ONE
elementwise + * / in the order the specification writes them (no np.sum, np.mean or dot, which may reorder), and the counts of
the observation cast to float32.  The state of B envs is held side by side; the envs never interact.  `counts` tallies what
happened, so that the tests can assert that their inputs reach every branch.
"""
import numpy as np

from oracle import c_oracle as co

GRID, N_PURSUERS, N_EVADERS, RANGE = 16, 8, 30, 7
OBS, INIT_W, MAX_CYCLES, N_ACTIONS = RANGE * RANGE * 3, 40, 500, 5
P = 32 * OBS + 32 + N_ACTIONS * 32 + N_ACTIONS
BLOCK_X, BLOCK_Y = (5, 11), (4, 12)                     # the obstacle block, bounds inclusive
TAG, CATCH, URGENCY = 0.01, 5.0, -0.1
MOVE_TAG = 2                                            # stream tag of the evader moves: counter word 3 = tag << 24
MOVES = np.array([(-1, 0), (1, 0), (0, 1), (0, -1), (0, 0)], np.int64)
NEIGHBOURS = MOVES[:4]

BLOCKED = np.zeros((GRID, GRID), bool)
BLOCKED[BLOCK_X[0]:BLOCK_X[1] + 1, BLOCK_Y[0]:BLOCK_Y[1] + 1] = True
FREE = np.array([(x, y) for x in range(GRID) for y in range(GRID) if not BLOCKED[x, y]], np.int64)      # ascending (x, y)

EVENTS = ("catches", "pursuer_moves_refused", "evader_moves_refused", "out_of_range_actions", "shared_cells", "episodes_ended")


def is_free(x, y):
    """elementwise: the cell is on the grid and outside the block"""
    x, y = np.asarray(x), np.asarray(y)
    on = (x >= 0) & (x < GRID) & (y >= 0) & (y < GRID)
    return on & ~BLOCKED[np.clip(x, 0, GRID - 1), np.clip(y, 0, GRID - 1)]


def cell_index(u):
    """float32 init entries -> indices into FREE: min(192, (int)(u * 193.0f)), negatives and NaN at 0"""
    v = np.asarray(u, np.float32) * np.float32(193.0)
    with np.errstate(invalid="ignore"):
        t = np.where(v >= np.float32(192.0), np.float32(192.0), v)
        return np.where(~(v >= np.float32(0.0)), 0, np.trunc(np.where(v >= np.float32(0.0), t, 0.0)).astype(np.int64))


def evader_moves(key, cycle):
    """The 30 moves that the stream of `key` (two uint32 words) holds for `cycle`: ONE Philox draw, counter (0, 0, cycle, tag << 24);
    evader e's move is base-5 digit e & 7 of word e >> 3."""
    w = co.philox_raw([0, 0, int(cycle), MOVE_TAG << 24], key).astype(np.int64)
    e = np.arange(N_EVADERS)
    return (w[e >> 3] // 5 ** (e & 7)) % 5


def _step_cells(x, y, move):
    """applies moves (indices into MOVES; 4 = stay) where the target is free; returns (x, y, refused)"""
    nx, ny = x + MOVES[move, 0], y + MOVES[move, 1]
    ok = is_free(nx, ny)
    return np.where(ok, nx, x), np.where(ok, ny, y), ~ok


class Pursuit:
    """B independent envs; init: float32[B, 40]"""

    def __init__(self, init, counts=None):
        init = np.ascontiguousarray(init, np.float32).reshape(-1, INIT_W)
        B = self.B = init.shape[0]
        self.counts = counts if counts is not None else dict.fromkeys(EVENTS, 0)
        cells = FREE[cell_index(init[:, :N_PURSUERS + N_EVADERS])]                      # [B, 38, 2]
        self.px, self.py = cells[:, :N_PURSUERS, 0].copy(), cells[:, :N_PURSUERS, 1].copy()
        self.ex, self.ey = cells[:, N_PURSUERS:, 0].copy(), cells[:, N_PURSUERS:, 1].copy()
        self.alive = ~(init[:, N_PURSUERS:N_PURSUERS + N_EVADERS] < np.float32(0.0))     # [B, 30]
        self.key = init[:, 38:40].copy().view(np.uint32)
        self.cycle = np.zeros(B, np.int64)
        self.frozen = np.zeros(B, bool)          # set by the rollout for episodes that have ended: step() leaves them alone

    def step(self, action):
        """action: int[B, 8].  Returns (team reward float64[B], done bool[B]); frozen envs do not change and return (0, True)."""
        action = np.asarray(action).reshape(self.B, N_PURSUERS).astype(np.int64)
        run = ~self.frozen
        # 1. the pursuers
        bad = (action < 0) | (action > 4)
        move = np.where(bad, 4, action)
        px, py, refused = _step_cells(self.px, self.py, move)
        self.counts["out_of_range_actions"] += int((bad & run[:, None]).sum())
        self.counts["pursuer_moves_refused"] += int((refused & run[:, None]).sum())
        self.px, self.py = np.where(run[:, None], px, self.px), np.where(run[:, None], py, self.py)
        # 2. the live evaders
        em = np.full((self.B, N_EVADERS), 4, np.int64)
        for b in np.nonzero(run & self.alive.any(axis=1))[0]:
            em[b] = evader_moves(self.key[b], self.cycle[b])
        ex, ey, refused = _step_cells(self.ex, self.ey, em)
        moving = self.alive & run[:, None]
        self.counts["evader_moves_refused"] += int((refused & moving).sum())
        self.ex, self.ey = np.where(moving, ex, self.ex), np.where(moving, ey, self.ey)
        # 3. catches, all at once on the positions after all moves
        caught = self.alive.copy()
        for dx, dy in NEIGHBOURS:
            nx, ny = self.ex + dx, self.ey + dy                                          # [B, 30]
            held = ((self.px[:, None, :] == nx[:, :, None]) & (self.py[:, None, :] == ny[:, :, None])).any(axis=2)
            caught &= ~is_free(nx, ny) | held
        # 4. rewards, float64
        dist = np.abs(self.ex[:, None, :] - self.px[:, :, None]) + np.abs(self.ey[:, None, :] - self.py[:, :, None])   # [B, 8, 30]
        n_tag = np.count_nonzero(self.alive[:, None, :] & (dist <= 1), axis=2).astype(np.float64)
        n_catch = np.count_nonzero(caught[:, None, :] & (dist == 1), axis=2).astype(np.float64)
        r = (TAG * n_tag + CATCH * n_catch) + URGENCY                                    # [B, 8]
        total = r[:, 0]
        for i in range(1, N_PURSUERS):
            total = total + r[:, i]
        mean = total / 8.0
        team = mean
        for i in range(1, N_PURSUERS):
            team = team + mean
        # 5. removal, 6. done
        caught &= run[:, None]
        self.counts["catches"] += int(caught.sum())
        self.alive = self.alive & ~caught
        self.cycle = self.cycle + run
        done = ~self.alive.any(axis=1)
        return np.where(run, team, 0.0), done | self.frozen

    def observe(self):
        """float32[B, 8, 147]: [dx][dy][wall, pursuers in the cell, live evaders in the cell]"""
        B, pad = self.B, RANGE // 2
        grids = np.zeros((2, B, GRID + 2 * pad, GRID + 2 * pad), np.float32)
        b = np.arange(B)[:, None]
        np.add.at(grids[0], (np.broadcast_to(b, self.px.shape), self.px + pad, self.py + pad), 1.0)
        eb = np.broadcast_to(b, self.ex.shape)[self.alive]
        np.add.at(grids[1], (eb, self.ex[self.alive] + pad, self.ey[self.alive] + pad), 1.0)
        self.counts["shared_cells"] += int((grids[0] > 1).sum() + (grids[1] > 1).sum())
        wall = np.ones((GRID + 2 * pad, GRID + 2 * pad), np.float32)
        wall[pad:pad + GRID, pad:pad + GRID] = BLOCKED
        wx = self.px[:, :, None, None] + np.arange(RANGE)[None, None, :, None]           # padded coordinates [B, 8, 7, 1]
        wy = self.py[:, :, None, None] + np.arange(RANGE)[None, None, None, :]
        obs = np.zeros((B, N_PURSUERS, RANGE, RANGE, 3), np.float32)
        obs[..., 0] = wall[wx, wy]
        obs[..., 1] = grids[0][b[:, :, None, None], wx, wy]
        obs[..., 2] = grids[1][b[:, :, None, None], wx, wy]
        return obs.reshape(B, N_PURSUERS, OBS)


def policy_actions(theta_rows, obs):
    """theta_rows float32[B, P] (one row per env), obs float32[B, 8, 147] -> the moves int32[B, 8] (first-maximum argmax)"""
    B = obs.shape[0]
    th = np.repeat(np.ascontiguousarray(theta_rows, np.float32).reshape(B, P), N_PURSUERS, axis=0)
    action, _, _, _ = co.policy_forward(OBS, N_ACTIONS, True, False, th, obs.reshape(B * N_PURSUERS, OBS))
    return action.reshape(B, N_PURSUERS)


def rollout(theta, init, E, max_step, counts=None):
    """theta float32[n, P]; init float32[n, E, 40] or [E, 40] (shared) -> (fitness float32[n], ep_return float64[n, E],
    ep_steps int32[n, E], counts): every episode runs until no evader is left or min(max_step, 500) cycles"""
    theta = np.ascontiguousarray(theta, np.float32)
    n = theta.shape[0]
    init = np.ascontiguousarray(init, np.float32)
    if init.ndim == 2:
        init = np.broadcast_to(init[None], (n, E, INIT_W))
    env = Pursuit(init.reshape(n * E, INIT_W), counts)
    rows = np.repeat(theta, E * N_PURSUERS, axis=0)                      # one row per (offspring, episode, pursuer)
    ret = np.zeros(n * E, np.float64)
    steps = np.zeros(n * E, np.int32)
    for _ in range(min(int(max_step), MAX_CYCLES)):
        if env.frozen.all():
            break
        running = ~env.frozen
        action = co.policy_forward(OBS, N_ACTIONS, True, False, rows, env.observe().reshape(n * E * N_PURSUERS, OBS))[0]
        r, done = env.step(action.reshape(n * E, N_PURSUERS))
        ret = np.where(running, ret + r, ret)
        steps = steps + running
        env.counts["episodes_ended"] += int((done & running).sum())
        env.frozen = done
    ep = ret.reshape(n, E)
    total = np.zeros(n, np.float64)
    for e in range(E):
        total = total + ep[:, e]
    return (total / float(E)).astype(np.float32), ep, steps.reshape(n, E), env.counts


# ---- the inputs the tests share ------------------------------------------------------------------------------------------------
def entry(x, y):
    """the init entry that names free cell (x, y): the centre of its 1/193 interval"""
    i = int(np.nonzero((FREE[:, 0] == x) & (FREE[:, 1] == y))[0][0])
    return np.float32((i + 0.5) / 193.0)


def craft(pursuers=(), evaders=(), key=(0.123, 0.456)):
    """One init row: the pursuers parked on (15, 8 + i) out of everybody's way except those given as {index: (x, y)}; ONLY the evaders
    given as {index: (x, y)} exist, all others carry a negative entry."""
    row = np.full(INIT_W, -1.0, np.float32)
    for i in range(N_PURSUERS):
        row[i] = entry(15, 8 + i)
    for i, (x, y) in dict(pursuers).items():
        row[i] = entry(x, y)
    for e, (x, y) in dict(evaders).items():
        row[N_PURSUERS + e] = entry(x, y)
    row[38:40] = key
    return row


CRAFTED = {
    # an evader in the corner has two open neighbours: both held / one short
    "corner_caught": craft(pursuers={0: (1, 0), 1: (0, 1)}, evaders={0: (0, 0)}),
    "corner_short": craft(pursuers={0: (1, 0)}, evaders={0: (0, 0)}),
    # beside the block at (4, 8): (5, 8) is in the block, three open neighbours
    "block_caught": craft(pursuers={0: (3, 8), 1: (4, 7), 2: (4, 9)}, evaders={0: (4, 8)}),
    "block_short": craft(pursuers={0: (3, 8), 1: (4, 7)}, evaders={0: (4, 8)}),
    # in the open at (2, 2): four
    "open_caught": craft(pursuers={0: (1, 2), 1: (3, 2), 2: (2, 1), 3: (2, 3)}, evaders={0: (2, 2)}),
    "open_short": craft(pursuers={0: (1, 2), 1: (3, 2), 2: (2, 1)}, evaders={0: (2, 2)}),
    # two boxed evaders, in opposite corners
    "two_corners": craft(pursuers={0: (1, 0), 1: (0, 1), 2: (14, 0), 3: (15, 1)}, evaders={0: (0, 0), 7: (15, 0)}),
    # no evader at all: done after the first cycle, whatever it is
    "no_evaders": craft(pursuers={0: (1, 0), 1: (0, 1)}),
    # everybody in one cell
    "one_cell": np.concatenate([np.full(38, entry(3, 3), np.float32), np.float32([0.5, 0.25])]),
    # actors on every edge and at the block's sides
    "edges": np.concatenate([np.float32([entry(0, 0), entry(0, 15), entry(15, 0), entry(15, 15), entry(4, 8), entry(12, 8), entry(8, 3),
                                         entry(8, 13)]),
                             np.float32([entry(x, y) for x, y in [(0, 7), (15, 7), (7, 0), (7, 15), (4, 4), (12, 12), (5, 3), (11, 13)]]),
                             np.float32([entry(0, y) for y in range(11)]), np.float32([entry(x, 15) for x in range(11)]),
                             np.float32([0.75, 0.0625])]),
}


def crafted_rows():
    return np.stack(list(CRAFTED.values()))


def stay_theta(n=1, seed=0):
    """policies whose b2 makes action 4 (stay) win everywhere: tiny random weights, b2 = (0, 0, 0, 0, 100)"""
    rng = np.random.RandomState(seed)
    th = (rng.randn(n, P) * 1e-3).astype(np.float32)
    th[:, -N_ACTIONS:] = (0.0, 0.0, 0.0, 0.0, 100.0)
    return th


def thetas(n, seed):
    """randn x {0.2, 1, 3} per row"""
    rng = np.random.RandomState(seed)
    return (rng.randn(n, P) * rng.choice([0.2, 1.0, 3.0], size=(n, 1))).astype(np.float32)


STEPWISE_N, STEPWISE_CYCLES = 37, 40


def stepwise_reference():
    """(init[37, 40], actions[T][37, 8], obs[T + 1][37, 8, 147], reward[T][37] float32, done[T][37], counts): the crafted rows and
    random ones, 40 cycles of random actions -- one in eight of them outside 0 .. 4"""
    if "stepwise" not in _cache:
        crafted = crafted_rows()
        init = np.concatenate([crafted, co.init_states_uniform(5, 1, 0, STEPWISE_N - len(crafted), 1, INIT_W, False, 0.0, 1.0)[:, 0]])
        rng = np.random.RandomState(11)
        env = Pursuit(init)
        obs, acts, rews, dones = [env.observe()], [], [], []
        for _ in range(STEPWISE_CYCLES):
            a = rng.randint(0, 5, size=(STEPWISE_N, N_PURSUERS)).astype(np.int32)
            odd = rng.rand(STEPWISE_N, N_PURSUERS) < 0.125
            a[odd] = rng.choice([-1, 5, 7, -2 ** 31, 2 ** 31 - 1], size=int(odd.sum()))
            r, d = env.step(a)
            acts.append(a)
            rews.append(r.astype(np.float32))
            dones.append(d.copy())
            obs.append(env.observe())
        _cache["stepwise"] = (init, acts, obs, rews, dones, dict(env.counts))
    return _cache["stepwise"]


FUSED_E, FUSED_N, FUSED_MAX_STEP = (1, 3, 4, 5, 8), (1, 5, 37), 60


def fused_inputs(E, n):
    theta = thetas(n, 100 * E + n)
    init = co.init_states_uniform(7, E, 3, n, E, INIT_W, False, 0.0, 1.0)
    flat = init.reshape(-1, INIT_W)
    crafted = crafted_rows()
    for i in range(min(len(crafted), (flat.shape[0] + 1) // 2)):            # every second (offspring, episode) slot, while they last
        flat[2 * i] = crafted[(i + E) % len(crafted)]
    return theta, init


_cache = {}


def fused_reference(E, n):
    """(theta, init, fitness, ep_return, ep_steps, counts) of a case, computed once and handed out read-only"""
    if (E, n) not in _cache:
        theta, init = fused_inputs(E, n)
        fit, ep, steps, counts = rollout(theta, init, E, FUSED_MAX_STEP)
        for a in (theta, init, fit, ep, steps):
            a.setflags(write=False)
        _cache[(E, n)] = (theta, init, fit, ep, steps, dict(counts))
    return _cache[(E, n)]


def early_inputs(n=5, E=5):
    """(theta, init): stay-put policies; of every offspring's five episodes, 0 and 3 hold one boxed evader in a corner, 1 holds two in
    opposite corners, and 2 and 4 are the generator's 30 evaders, which run on to max_step"""
    theta = stay_theta(n, 3)
    init = co.init_states_uniform(13, 2, 0, n, E, INIT_W, False, 0.0, 1.0)
    for i in range(n):
        # different key words per slot: different cycles in which the evaders first stay put
        init[i, 0] = craft(pursuers={0: (1, 0), 1: (0, 1)}, evaders={0: (0, 0)}, key=(0.1 + 0.01 * i, 0.7))
        init[i, 1] = craft(pursuers={0: (1, 0), 1: (0, 1), 2: (14, 0), 3: (15, 1)}, evaders={0: (0, 0), 7: (15, 0)}, key=(0.2, 0.3 + 0.01 * i))
        init[i, 3] = craft(pursuers={0: (1, 0), 1: (0, 1)}, evaders={0: (0, 0)}, key=(0.9, 0.05 * (i + 1)))
    return theta, init
