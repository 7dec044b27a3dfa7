"""waterworld without a GPU: the sensor table, hand-predicted transitions of the numpy restatement (tests/waterworld_np.py, the
yardstick of tests/test_gpu_waterworld.py), the wrapper's and the config's shape, and the coverage of the GPU tests' inputs."""
import os
import re

import numpy as np
import yaml

import waterworld_np as ww

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
IDLE = np.zeros((1, 5, 2), np.float32)


def ulps(a, b):
    return np.abs(np.asarray(a, np.float64).view(np.int64) - np.asarray(b, np.float64).view(np.int64))


def test_sensor_literals_equal_the_headers():
    text = open(os.path.join(SRC, "csrc", "ses_waterworld.h")).read()
    table = text[text.index("WW_SENSOR_TABLE_BEGIN"):text.index("WW_SENSOR_TABLE_END")]
    lits = re.findall(r"-?0x[0-9a-f]+\.[0-9a-f]+p[+-][0-9]+", table)
    assert len(lits) == 60
    assert lits == [x for pair in ww.SENSOR_HEX for x in pair]


def test_sensor_literals_are_cos_and_sin():
    ang = np.arange(30, dtype=np.float64) * (6.283185307179586 / 30.0)
    # a value and its neighbour differ by 1 in the int64 view except across zero, which only sin(0) = 0 touches (it is exact)
    assert ww.SENSORS[0, 0] == 1.0 and ww.SENSORS[0, 1] == 0.0
    assert ulps(ww.SENSORS[1:, 0], np.cos(ang[1:])).max() <= 1
    assert ulps(ww.SENSORS[1:, 1], np.sin(ang[1:])).max() <= 1


def one(name):
    return ww.Waterworld(ww.CRAFTED[name][None])


def test_two_idle_pursuers_on_one_evader_catch_it():
    env = one("catch")
    r = env.step(IDLE)
    assert r[0] == (10.0 + 0.01) + (10.0 + 0.01) and abs(r[0] - 2 * 10.01) < 1e-12
    assert env.ctr[0] == 1 and env.counts["catches"] == 1 and env.counts["lone_touches"] == 0
    assert (env.px[0, 5], env.py[0, 5]) != (np.float64(np.float32(0.30)), np.float64(np.float32(0.10)) + 0.01)
    obs = env.observe()
    assert obs[0, :, 240].tolist() == [1, 1, 0, 0, 0] and not obs[0, :, 241].any()


def test_one_pursuer_on_an_evader_only_meets_it():
    env = one("lone_touch")
    assert env.step(IDLE)[0] == 0.01
    assert env.ctr[0] == 0 and env.counts["catches"] == 0 and env.counts["lone_touches"] == 1


def test_a_pursuer_on_a_poison_pays_and_the_poison_respawns():
    env = one("poison")
    assert env.step(IDLE)[0] == -1.0
    assert env.ctr[0] == 1 and env.counts["poison_touches"] == 1
    assert env.observe()[0, :, 241].tolist() == [1, 0, 0, 0, 0]


def test_an_evader_aimed_at_a_wall_bounces():
    env = one("wall_bounce")
    assert env.vx[0, 5] == 0.01 and env.vy[0, 5] == 0.0
    env.step(IDLE)
    assert env.px[0, 5] == 1.0 and env.vx[0, 5] == -0.01 and env.counts["wall_bounces"] == 1
    env.step(IDLE)
    assert env.px[0, 5] == 1.0 - 0.01


def test_a_poison_aimed_at_the_obstacle_rebounds_and_ends_outside():
    env = one("obstacle")
    lim = ww.R_PO + ww.R_OB
    env.step(IDLE)
    assert env.counts["obstacle_rebounds"] == 1
    assert env.vx[0, 10] == -0.01 and abs(env.vy[0, 10]) == 0.0          # head on: the velocity is mirrored
    for _ in range(3):
        env.step(IDLE)
    assert abs(env.px[0, 10] - 0.5) > lim and env.vx[0, 10] < 0.0


def test_a_pursuer_pushed_past_a_wall_loses_that_velocity_component():
    env = one("wall_clip")
    act = IDLE.copy()
    act[0, 0] = (-0.05, 0.003)                                            # longer than pursuer_max_accel: rescaled to length 0.01
    r = env.step(act)
    assert env.px[0, 0] == 0.0 and env.vx[0, 0] == 0.0 and env.vy[0, 0] > 0.0 and env.counts["wall_clips"] == 1
    assert abs(r[0] - (-0.5 * 0.01)) < 1e-15


def test_objects_drawn_inside_the_obstacle_are_moved_at_reset():
    env = one("in_obstacle")
    assert env.counts["reset_respawns"] == 3 and env.ctr[0] == 3
    d2 = (env.px[0] - 0.5) ** 2 + (env.py[0] - 0.5) ** 2
    assert (d2 > (ww.R_OB + ww.RADIUS) ** 2).all()
    assert env.vx[0, 2] == 0.0 and env.vy[0, 2] == 0.0                   # a respawned pursuer keeps velocity 0


def test_wrapper_constructs_without_a_gpu():
    from envs.pettingzoo_wrapper import PettingzooWrapper
    env = PettingzooWrapper("waterworld", 500)
    assert env.get_agent_ids() == [f"pursuer_{i}" for i in range(5)] and env.n_agents == 5 and env.horizon == 500
    assert PettingzooWrapper("waterworld", 2000).horizon == 500 and PettingzooWrapper("waterworld", 40).horizon == 40
    assert env.variant == "waterworld-restated"


def test_config_builds_the_242_input_network():
    import builder
    cfg = yaml.load(open(os.path.join(SRC, "conf", "waterworld.yaml")), Loader=yaml.FullLoader)
    assert cfg["env"] == {"name": "waterworld", "max_step": 500}
    assert cfg["strategy"]["name"] == "openai_es" and cfg["strategy"]["offspring_num"] == 256
    net = builder.build_network(cfg["network"])
    assert net.param_count() == 7842 == ww.P
    env = builder.build_env(cfg["env"])
    assert env.n_agents == 5 and env.horizon == 500


def test_gpu_test_inputs_reach_every_event():
    """Over the exact inputs of tests/test_gpu_waterworld.py -- the step-wise run and every fused case -- each event happens."""
    total = dict.fromkeys(ww.EVENTS, 0)
    for counts in [ww.stepwise_reference()[5]] + [ww.fused_reference(case)[4] for case in ww.FUSED_CASES]:
        assert set(counts) == set(ww.EVENTS)
        for k, v in counts.items():
            total[k] += v
    assert all(v >= 1 for v in total.values()), total
    assert {c[0] for c in ww.FUSED_CASES} >= {1, 5, 6, 7, 13} and {c[1] for c in ww.FUSED_CASES} >= {1, 3, 70}
    assert {c[2] for c in ww.FUSED_CASES} >= {1, 12, 40}
