"""pursuit without a GPU: the map, hand-predicted transitions of the numpy restatement (tests/pursuit_np.py, the yardstick of
tests/test_gpu_pursuit.py), the wrapper's and the config's shape, and the coverage of the GPU tests' inputs."""
import os

import numpy as np
import yaml

import pursuit_np as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
STAY = np.full((1, 8), 4, np.int64)


def key_for(move_of, cycles=1, **kw):
    """Key words (as two floats) under which evader e draws move_of[e] in each of the first `cycles` cycles."""
    for k in range(1, 4000):
        key = np.float32([k / 4096.0, 0.5])
        if all(all(pu.evader_moves(key.view(np.uint32), c)[e] == m for e, m in move_of.items()) for c in range(cycles)):
            return tuple(key)
    raise AssertionError("no key found")


def one(name, move_of=None):
    row = pu.CRAFTED[name].copy()
    if move_of:
        row[38:40] = key_for(move_of)
    return pu.Pursuit(row[None])


def test_free_table_has_193_cells_none_in_the_block():
    assert pu.FREE.shape == (193, 2) and len({tuple(c) for c in pu.FREE}) == 193
    assert [tuple(c) for c in pu.FREE] == sorted(tuple(c) for c in pu.FREE)             # ascending (x, y)
    assert not any(5 <= x <= 11 and 4 <= y <= 12 for x, y in pu.FREE)
    assert all(0 <= x < 16 and 0 <= y < 16 for x, y in pu.FREE)
    # rectangle_map's block for xb = 0.3, yb = 0.2 on 16 x 16: 7 x 9 cells
    assert int(pu.BLOCKED.sum()) == 63 and 256 - 63 == 193
    assert tuple(pu.FREE[0]) == (0, 0) and tuple(pu.FREE[192]) == (15, 15) and tuple(pu.FREE[80]) == (5, 0) and tuple(pu.FREE[84]) == (5, 13)


def test_init_entries_name_cells():
    assert pu.cell_index(np.float32([0.0, 0.999999, 1.0, 5.0, -0.5, np.nan, 0.5])).tolist() == [0, 192, 192, 192, 0, 0, 96]
    for i in (0, 1, 80, 84, 192):
        x, y = pu.FREE[i]
        assert pu.cell_index(pu.entry(x, y)) == i


def test_moves_respect_the_grid_and_the_block_from_every_boundary_cell():
    want = {0: (-1, 0), 1: (1, 0), 2: (0, 1), 3: (0, -1), 4: (0, 0)}
    seen_refusals = 0
    for x, y in pu.FREE:
        for m, (dx, dy) in want.items():
            nx, ny, refused = pu._step_cells(np.array([x]), np.array([y]), np.array([m]))
            tx, ty = x + dx, y + dy
            ok = 0 <= tx < 16 and 0 <= ty < 16 and not (5 <= tx <= 11 and 4 <= ty <= 12)
            assert (int(nx[0]), int(ny[0])) == ((tx, ty) if ok else (x, y)) and bool(refused[0]) == (not ok)
            seen_refusals += not ok
    # 64 moves off the grid (16 cells a side) and 32 into the block (7 + 7 + 9 + 9 cells beside it)
    assert seen_refusals == 64 + 32
    env = one("corner_short")
    env.step(np.array([[3, 9, -3, 5, 2 ** 31 - 1, -2 ** 31, 4, 4]]))                    # pursuer 0: off the grid; the rest: no move
    assert (env.px[0].tolist(), env.py[0].tolist()) == ([1] + [15] * 7, [0] + list(range(9, 16)))
    assert env.counts["out_of_range_actions"] == 5


def test_catch_rule_on_hand_placed_positions():
    for name, opens in (("corner", 2), ("block", 3), ("open", 4)):
        env = one(name + "_caught", {0: 4})
        assert env.alive[0].sum() == 1
        r, done = env.step(STAY)
        assert env.counts["catches"] == 1 and not env.alive.any() and done[0], name
        # `opens` pursuers are adjacent to the caught evader: each 0.01 + 5.0 - 0.1, the others -0.1
        own = [(0.01 * 1.0 + 5.0 * 1.0) + -0.1] * opens + [(0.01 * 0.0 + 5.0 * 0.0) + -0.1] * (8 - opens)
        total = own[0]
        for v in own[1:]:
            total = total + v
        mean = total / 8.0
        team = mean
        for _ in range(7):
            team = team + mean
        assert r[0] == team and abs(r[0] - (5.01 * opens - 0.8)) < 1e-12, name
        env = one(name + "_short", {0: 4})
        r, done = env.step(STAY)
        assert env.counts["catches"] == 0 and env.alive[0].sum() == 1 and not done[0], name
        assert abs(r[0] - (0.01 * (opens - 1) - 0.8)) < 1e-12, name


def test_an_evader_that_moves_away_is_not_caught_until_it_stays():
    env = one("corner_caught", {0: 1})                                                   # (0, 0) -> (1, 0), onto pursuer 0
    r, done = env.step(STAY)
    assert (env.ex[0, 0], env.ey[0, 0]) == (1, 0) and env.alive[0, 0] and not done[0]
    # it now shares pursuer 0's cell (tagged by it) and sits beside nobody else: (0, 1) is at distance 2
    assert abs(r[0] - (0.01 - 0.8)) < 1e-12


def test_a_pursuer_in_the_evaders_own_cell_tags_it_but_does_not_hold_a_neighbour():
    env = pu.Pursuit(pu.craft(pursuers={0: (0, 0), 1: (0, 1)}, evaders={0: (0, 0)}, key=key_for({0: 4}))[None])
    r, done = env.step(STAY)
    assert env.counts["catches"] == 0 and abs(r[0] - (0.02 - 0.8)) < 1e-12               # (1, 0) is open and empty


def test_observation_layout():
    env = one("edges")
    obs = env.observe().reshape(8, 7, 7, 3)
    # pursuer 0 at (0, 0): window x, y = -3 .. 3; off the grid is wall
    assert (obs[0, :3, :, 0] == 1).all() and (obs[0, :, :3, 0] == 1).all() and (obs[0, 3:, 3:, 0] == 0).all()
    assert obs[0, 3, 3, 1] == 1 and obs[0, 3, 3, 2] == 1                                  # itself; the evader on (0, 0)
    assert obs[0, 3, 4, 2] == 1 and obs[0, 3, 6, 2] == 1                                  # evaders (0, 1), (0, 3)
    # pursuer 3 at (15, 15): the far edges
    assert (obs[3, 4:, :, 0] == 1).all() and (obs[3, :, 4:, 0] == 1).all() and (obs[3, :4, :4, 0] == 0).all()
    # pursuer 1 at (0, 15) and pursuer 2 at (15, 0): the other two corners
    assert (obs[1, :3, :, 0] == 1).all() and (obs[1, :, 4:, 0] == 1).all() and (obs[1, 3:, :4, 0] == 0).all()
    assert (obs[2, 4:, :, 0] == 1).all() and (obs[2, :, :3, 0] == 1).all() and (obs[2, :4, 3:, 0] == 0).all()
    # pursuer 4 at (4, 8): the block is x >= 5, i.e. dx >= 4, for y = 5 .. 11, all seven dy
    assert (obs[4, 4:, :, 0] == 1).all() and (obs[4, :4, :, 0] == 0).all()
    # pursuer 6 at (8, 3): the block's top rows are y >= 4, i.e. dy >= 4, for x = 5 .. 11
    assert (obs[6, :, 4:, 0] == 1).all() and (obs[6, :, :4, 0] == 0).all()
    assert obs[6, 0, 3, 2] == 1                                                           # evader (5, 3)
    # channels 1 and 2 are 0 wherever channel 0 is 1
    assert not obs[..., 1][obs[..., 0] == 1].any() and not obs[..., 2][obs[..., 0] == 1].any()
    env = one("one_cell")
    obs = env.observe().reshape(8, 7, 7, 3)
    assert (obs[:, 3, 3, 1] == 8).all() and (obs[:, 3, 3, 2] == 30).all()
    assert obs[..., 1].sum() == 64 and obs[..., 2].sum() == 240
    # flattening: component ((dx * 7) + dy) * 3 + channel
    flat = env.observe()
    assert flat[0, 0, (3 * 7 + 3) * 3 + 1] == 8 and flat[0, 0, (3 * 7 + 3) * 3 + 2] == 30


def test_an_evader_with_a_negative_entry_does_not_exist():
    env = one("corner_short")
    assert env.alive[0].tolist() == [True] + [False] * 29
    # the absent evaders were given cell 0 = (0, 0), where pursuer-adjacent cells would tag and observe them if they existed
    obs = env.observe().reshape(8, 7, 7, 3)
    assert obs[..., 2].sum() == 1 * 1                                                     # only pursuer 0 at (1, 0) sees evader 0
    row = pu.craft(pursuers={0: (1, 0), 1: (0, 1)})                                       # no evader at all
    env = pu.Pursuit(row[None])
    assert not env.observe()[..., 2::3].any()
    r, done = env.step(STAY)
    assert done[0] and abs(r[0] - -0.8) < 1e-12 and env.counts["catches"] == 0


def test_evader_stream_depends_on_key_cycle_and_index_only():
    key = np.float32([0.123, 0.456]).view(np.uint32)
    a = pu.evader_moves(key, 7)
    assert a.shape == (30,) and ((a >= 0) & (a <= 4)).all()
    assert (a == pu.evader_moves(key.copy(), 7)).all()
    assert (a != pu.evader_moves(key, 8)).any() and (a != pu.evader_moves(key[::-1].copy(), 7)).any()
    # removing evaders changes nobody else's move: two envs, one of them without evaders 0 .. 9
    rows = np.stack([pu.CRAFTED["edges"], pu.CRAFTED["edges"]])
    rows[1, 8:18] = -1.0
    env = pu.Pursuit(rows)
    for _ in range(5):
        env.step(np.full((2, 8), 4))
        assert (env.ex[0, 10:] == env.ex[1, 10:]).all() and (env.ey[0, 10:] == env.ey[1, 10:]).all()
    # all five moves occur, in roughly equal shares
    many = np.concatenate([pu.evader_moves(key, c) for c in range(200)])
    assert (np.bincount(many, minlength=5) > 0.15 * many.size).all()


def test_parameter_count():
    from oracle import c_oracle as co
    assert pu.P == 4901 == co.param_count(147, 5, False)


def test_wrapper_constructs_without_a_gpu():
    from envs.pettingzoo_wrapper import PettingzooWrapper
    env = PettingzooWrapper("pursuit", 500)
    assert env.get_agent_ids() == [f"pursuer_{i}" for i in range(8)] and env.n_agents == 8 and env.horizon == 500
    assert PettingzooWrapper("pursuit", 2000).horizon == 500 and PettingzooWrapper("pursuit", 40).horizon == 40
    assert env.variant == "pettingzoo-restated"
    try:
        PettingzooWrapper("pursuit", 500, n_agents=5)
    except NotImplementedError as e:
        assert "eight" in str(e)
    else:
        raise AssertionError("n_agents=5 accepted")


def test_config_builds_the_147_input_network():
    import builder
    from ses import device
    cfg = yaml.load(open(os.path.join(SRC, "conf", "pursuit.yaml")), Loader=yaml.FullLoader)
    assert cfg["env"] == {"name": "pursuit", "max_step": 500}
    assert cfg["strategy"]["name"] == "openai_es" and cfg["strategy"]["offspring_num"] == 256
    assert cfg["network"]["discrete_action"] is True and cfg["network"]["gru"] is False
    net = builder.build_network(cfg["network"])
    assert net.param_count() == 4901
    env = builder.build_env(cfg["env"])
    assert env.n_agents == 8 and env.horizon == 500
    assert device.ENV_IDS["pursuit"] == 12


def test_gpu_test_inputs_reach_every_event():
    """Over inputs of tests/test_gpu_pursuit.py -- the step-wise run, two fused cases and the early-termination case -- each event
    happens, and the early case ends episodes at different cycles beside episodes that run to max_step."""
    total = dict.fromkeys(pu.EVENTS, 0)
    theta, init = pu.early_inputs()
    _, _, steps, early = pu.rollout(theta, init, 5, pu.FUSED_MAX_STEP)
    for counts in (pu.stepwise_reference()[5], pu.fused_reference(5, 5)[5], pu.fused_reference(3, 1)[5], early):
        assert set(counts) == set(pu.EVENTS)
        for k, v in counts.items():
            total[k] += v
    assert all(v >= 1 for v in total.values()), total
    assert (steps[:, [2, 4]] == pu.FUSED_MAX_STEP).all() and (steps[:, [0, 1, 3]] < pu.FUSED_MAX_STEP).sum() >= 8
    assert len(set(steps[:, [0, 1, 3]].ravel().tolist())) >= 4
