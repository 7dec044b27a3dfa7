"""Pendulum-v1 and MountainCarContinuous-v0 on the host side (no GPU needed): the wrapper, the configs, the C ABI's validation
of the new env ids, and hand cases of the numpy checker (tests/classic_control_cont_np.py) that follow from the equations
alone."""
import ctypes
import os

import numpy as np
import pytest
import yaml

import classic_control_cont_np as ccc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
SPECS = {"Pendulum-v1": (3, 1, 200, "pendulum"), "MountainCarContinuous-v0": (2, 1, 999, "mountaincar_continuous")}


@pytest.mark.parametrize("name", sorted(SPECS))
def test_gym_wrapper_accepts_the_continuous_classic_envs(name):
    import builder
    from envs.gym_wrapper import GymWrapper
    S, A, limit, _ = SPECS[name]
    env = builder.build_env({"name": name, "max_step": "None", "pomdp": False})
    assert isinstance(env, GymWrapper)
    assert env.spec == dict(num_state=S, num_action=A, discrete=False, time_limit=limit)
    assert env.horizon == limit and env.variant == "classic-control-restated"
    assert GymWrapper(name, 150).horizon == 150 and GymWrapper(name, 10 ** 6).horizon == limit
    with pytest.raises(AssertionError):
        GymWrapper(name, None, pomdp=True)


@pytest.mark.parametrize("name", sorted(SPECS))
def test_the_continuous_classic_configs_load_through_the_builder(name):
    import builder
    S, A, limit, conf = SPECS[name]
    cfg = yaml.load(open(os.path.join(SRC, "conf", conf + ".yaml")), Loader=yaml.FullLoader)
    env = builder.build_env(cfg["env"])
    net = builder.build_network(cfg["network"])
    strat = builder.build_strategy(cfg["strategy"])
    assert env.name == name and env.horizon == limit and cfg["env"]["max_step"] == limit
    assert (net.num_state, net.num_action, net.discrete_action, net.use_gru) == (S, A, False, False)
    assert cfg["strategy"]["name"] in ("openai_es", "simple_evolution") and strat is not None
    if name == "Pendulum-v1":
        assert cfg["strategy"]["name"] == "openai_es"


def _create(env_id, S, A, discrete=0, gru=0, pomdp=0, physics64=0, lanes=0):
    from ses import _lib
    lib = _lib.load()
    cfg = _lib.SesConfig(env_id, S, A, discrete, gru, pomdp, 100, 5, 0, lanes, 1, physics64)
    h = ctypes.c_void_p()
    rc = lib.ses_create(ctypes.byref(cfg), None, ctypes.byref(h))
    if rc == _lib.SES_OK:
        lib.ses_destroy(h)
    return rc


@pytest.mark.parametrize("env", ["pendulum", "mountaincar_continuous"])
def test_ses_create_validates_the_continuous_classic_envs(env):
    from ses import _lib
    from ses.device import ENV_IDS
    assert (_lib.ENV_PENDULUM, _lib.ENV_MOUNTAINCAR_CONT) == (6, 7)
    assert ENV_IDS["Pendulum-v1"] == 6 and ENV_IDS["MountainCarContinuous-v0"] == 7
    eid, S = (_lib.ENV_PENDULUM, 3) if env == "pendulum" else (_lib.ENV_MOUNTAINCAR_CONT, 2)
    ok = (_lib.SES_OK, -4)                                              # SES_ERR_NO_DEVICE on a machine without a GPU
    assert _create(eid, S, 1) in ok
    assert _create(eid, S, 1, gru=1) in ok
    assert _create(eid, S, 1, lanes=32) in ok
    for bad in (dict(S=S + 1), dict(A=2), dict(discrete=1), dict(pomdp=1), dict(physics64=1), dict(gru=2)):
        kw = dict(S=S, A=1)
        kw.update(bad)
        assert _create(eid, **kw) == -1, bad                            # SES_ERR_INVALID_ARG


def f32(*v):
    return np.array(v, np.float32)


def test_checker_pendulum_hand_cases():
    """Transitions whose outcome follows from the equations alone (no rounding question)."""
    # at rest upright with no torque nothing moves and nothing is charged
    s, obs, r, d = ccc.pendulum_step(np.zeros((2, 1)), f32(0.0))
    assert s[0, 0] == 0.0 and s[1, 0] == 0.0 and r[0] == 0.0 and not d[0]
    assert obs.dtype == np.float32 and obs.shape == (1, 3) and tuple(obs[0]) == (1.0, 0.0, 0.0)
    assert r.dtype == np.float64
    # th = -pi: (th + pi) mod 2 pi = 0, the normalised angle is -pi and the cost pi^2
    _, _, r, _ = ccc.pendulum_step(np.array([[-np.pi], [0.0]]), f32(0.0))
    assert r[0] == -(np.pi * np.pi)
    # th = pi: th + pi = 2 pi, mod 0 again; a whole turn more or less changes nothing about the angle's cost
    _, _, r2, _ = ccc.pendulum_step(np.array([[np.pi], [0.0]]), f32(0.0))
    assert r2[0] == r[0]
    # the speed clip at +-8, and th' uses the clipped speed
    for sign in (1.0, -1.0):
        s, _, _, _ = ccc.pendulum_step(np.array([[sign * 0.5 * np.pi], [sign * 7.9]]), f32(sign * 1.0))
        assert s[1, 0] == sign * 8.0 and s[0, 0] == sign * 0.5 * np.pi + (sign * 8.0) * 0.05
    # the torque is clipped at +-2: a = 5 and a = 2 give the same transition and the same reward
    sa, _, ra, _ = ccc.pendulum_step(np.array([[0.3], [0.1]]), f32(5.0))
    sb, _, rb, _ = ccc.pendulum_step(np.array([[0.3], [0.1]]), f32(2.0))
    assert np.array_equal(sa, sb) and ra[0] == rb[0]
    sa, _, ra, _ = ccc.pendulum_step(np.array([[0.3], [0.1]]), f32(-7.0))
    sb, _, rb, _ = ccc.pendulum_step(np.array([[0.3], [0.1]]), f32(-2.0))
    assert np.array_equal(sa, sb) and ra[0] == rb[0]
    # every reward is <= 0 and the env never terminates
    rng = np.random.default_rng(0)
    s0 = np.stack([rng.uniform(-80, 80, 1000), rng.uniform(-9, 9, 1000)])
    _, _, r, d = ccc.pendulum_step(s0, rng.uniform(-3, 3, 1000).astype(np.float32))
    assert (r <= 0).all() and not d.any()
    # reset: th = u0 * pi, w = u1
    s = ccc.pendulum_reset(f32(0.5, -0.25)[None, :])
    assert s[0, 0] == 0.5 * np.pi and s[1, 0] == -0.25


def test_checker_mountaincar_continuous_hand_cases():
    # the left wall stops the car
    s, _, r, d = ccc.mountaincar_cont_step(np.array([[-1.2], [-0.05]]), f32(-1.0))
    assert s[0, 0] == float(np.float32(-1.2)) and s[1, 0] == 0.0 and not d[0]
    # the force is clipped at +-1 but the reward charges the unclipped a * a
    sa, _, ra, _ = ccc.mountaincar_cont_step(np.array([[-0.5], [0.0]]), f32(3.0))
    sb, _, rb, _ = ccc.mountaincar_cont_step(np.array([[-0.5], [0.0]]), f32(1.0))
    assert np.array_equal(sa, sb) and ra[0] == -(3.0 * 3.0) * 0.1 and rb[0] == -(1.0 * 1.0) * 0.1
    # the goal needs p >= 0.45 and v >= 0, and pays 100 - 0.1 a^2
    s, _, r, d = ccc.mountaincar_cont_step(np.array([[0.44], [0.05]]), f32(0.5))
    assert d[0] and s[0, 0] >= 0.45 and r[0] == 100.0 - (0.5 * 0.5) * 0.1
    s, _, r, d = ccc.mountaincar_cont_step(np.array([[0.5], [-0.03]]), f32(-1.0))
    assert s[0, 0] >= 0.45 and s[1, 0] < 0 and not d[0] and r[0] == -0.1
    s, _, r, d = ccc.mountaincar_cont_step(np.array([[0.40], [0.01]]), f32(0.0))
    assert s[0, 0] < 0.45 and not d[0] and r[0] == 0.0
    # the speed clip and the right end of the track
    s, _, _, _ = ccc.mountaincar_cont_step(np.array([[-0.5], [0.0699]]), f32(1.0))    # + 0.0015 - 0.0025 cos(-1.5) > 0.07
    assert s[1, 0] == float(np.float32(0.07))
    s, _, _, _ = ccc.mountaincar_cont_step(np.array([[-0.5], [-0.0699]]), f32(-1.0))
    assert s[1, 0] == float(np.float32(-0.07))
    s, _, _, d = ccc.mountaincar_cont_step(np.array([[0.59], [0.07]]), f32(1.0))
    assert s[0, 0] == float(np.float32(0.6)) and d[0]
    # the state after a step is float32-representable
    rng = np.random.default_rng(1)
    s0 = np.stack([rng.uniform(-1.25, 0.65, 1000), rng.uniform(-0.08, 0.08, 1000)])
    s, obs, _, d = ccc.mountaincar_cont_step(s0, rng.uniform(-1.5, 1.5, 1000).astype(np.float32))
    assert np.array_equal(s, s.astype(np.float32).astype(np.float64))
    assert np.array_equal(obs.astype(np.float64), s.T) and d.any() and not d.all()
    # reset: the widened float32 position, velocity 0
    s = ccc.mountaincar_cont_reset(f32(-0.5)[None, :])
    assert s[0, 0] == -0.5 and s[1, 0] == 0.0
