"""Acrobot-v1 and MountainCar-v0 on the host side (no GPU needed): the wrapper, the configs, the C ABI's validation of the
new env ids, and the accuracy of the numpy checker's sin / cos (tests/classic_control_np.py, the port of the device's)."""
import ctypes
import math
import os

import numpy as np
import pytest
import yaml

import classic_control_np as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
SPECS = {"Acrobot-v1": (6, 3, 500, "acrobot"), "MountainCar-v0": (2, 3, 200, "mountaincar")}


@pytest.mark.parametrize("name", sorted(SPECS))
def test_gym_wrapper_accepts_the_classic_envs(name):
    import builder
    from envs.gym_wrapper import GymWrapper
    S, A, limit, _ = SPECS[name]
    env = builder.build_env({"name": name, "max_step": "None", "pomdp": False})
    assert isinstance(env, GymWrapper)
    assert env.spec == dict(num_state=S, num_action=A, discrete=True, time_limit=limit)
    assert env.horizon == limit and env.variant == "classic-control-restated"
    assert GymWrapper(name, 150).horizon == 150 and GymWrapper(name, 10 ** 6).horizon == limit
    with pytest.raises(AssertionError):
        GymWrapper(name, None, pomdp=True)


@pytest.mark.parametrize("name", sorted(SPECS))
def test_the_classic_configs_load_through_the_builder(name):
    import builder
    S, A, limit, conf = SPECS[name]
    cfg = yaml.load(open(os.path.join(SRC, "conf", conf + ".yaml")), Loader=yaml.FullLoader)
    env = builder.build_env(cfg["env"])
    net = builder.build_network(cfg["network"])
    strat = builder.build_strategy(cfg["strategy"])
    assert env.name == name and env.horizon == limit
    assert (net.num_state, net.num_action, net.discrete_action, net.use_gru) == (S, A, True, False)
    assert cfg["strategy"]["name"] in ("openai_es", "simple_evolution") and strat is not None


def _create(env_id, S, A, discrete=1, gru=0, pomdp=0, physics64=0, lanes=0):
    from ses import _lib
    lib = _lib.load()
    cfg = _lib.SesConfig(env_id, S, A, discrete, gru, pomdp, 100, 5, 0, lanes, 1, physics64)
    h = ctypes.c_void_p()
    rc = lib.ses_create(ctypes.byref(cfg), None, ctypes.byref(h))
    if rc == _lib.SES_OK:
        lib.ses_destroy(h)
    return rc


@pytest.mark.parametrize("env", ["acrobot", "mountaincar"])
def test_ses_create_validates_the_classic_envs(env):
    from ses import _lib
    eid, S = (_lib.ENV_ACROBOT, 6) if env == "acrobot" else (_lib.ENV_MOUNTAINCAR, 2)
    assert (_lib.ENV_ACROBOT, _lib.ENV_MOUNTAINCAR) == (4, 5)
    ok = (_lib.SES_OK, -4)                                              # SES_ERR_NO_DEVICE on a machine without a GPU
    assert _create(eid, S, 3) in ok
    assert _create(eid, S, 3, gru=1) in ok
    assert _create(eid, S, 3, lanes=32) in ok
    for bad in (dict(S=S + 1), dict(A=2), dict(discrete=0), dict(pomdp=1), dict(physics64=1), dict(gru=2)):
        kw = dict(S=S, A=3)
        kw.update(bad)
        assert _create(eid, **kw) == -1, bad                            # SES_ERR_INVALID_ARG


def test_checker_sincos_is_within_two_ulp():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-1e3, 1e3, 200000), rng.uniform(-20.0, 20.0, 100000),
                        np.arange(-1000, 1001) * (np.pi / 4), np.nextafter(np.arange(-600, 601) * (np.pi / 2), np.inf),
                        [0.0, -0.0, 1e-300, -1e-300, 1e3, -1e3]])
    s, c = cc.sincos(x)
    want_s = np.array([math.sin(v) for v in x])
    want_c = np.array([math.cos(v) for v in x])
    tiny = np.spacing(0.0)
    for got, want in ((s, want_s), (c, want_c)):
        ulps = np.abs(got - want) / np.maximum(np.spacing(np.abs(want)), tiny)
        assert ulps.max() <= 2.0, (ulps.max(), x[np.argmax(ulps)])


def test_checker_follows_gym_on_hand_cases():
    """A few transitions whose outcome follows from the equations alone (no rounding question)."""
    # MountainCar: the left wall stops the car; the goal needs position >= 0.5 and velocity >= 0; the speed is clipped
    s, _, r, d = cc.mountaincar_step(np.array([[-1.2], [-0.05]]), np.array([0]))
    assert s[0, 0] == -1.2 and s[1, 0] == 0.0 and not d[0] and r[0] == -1.0
    s, _, _, d = cc.mountaincar_step(np.array([[0.49], [0.07]]), np.array([2]))
    assert s[1, 0] == 0.07 and s[0, 0] >= 0.5 and d[0]
    # Acrobot: at rest hanging down with no torque nothing moves; straight up is terminal
    s, obs, r, d = cc.acrobot_step(np.zeros((4, 1)), np.array([1]))
    assert np.all(np.abs(s) < 1e-12) and not d[0] and r[0] == -1.0
    assert obs.dtype == np.float32 and obs.shape == (1, 6)
    assert cc.acrobot_terminal(np.array([[np.pi], [0.0], [0.0], [0.0]]))[0]
    # wrap: into [-pi, pi] by whole turns
    assert cc.wrap(np.array([np.pi + 0.5]))[0] == (np.pi + 0.5) - 2 * np.pi
