"""ReacherBulletEnv-v0 on the host side (no GPU needed).  tests/reacher_np.py restates DESIGN.md 7 and the device code is held
to it bit for bit, so a derivation error would be copied faithfully: these tests are what checks the equations themselves --
energy conservation of the undamped arm in the limit dt -> 0, dissipation under zero action, the elbow limit, the action clip,
the idle return -- plus the wrapper, the two configs and the constants of the Python layer."""
import ctypes
import os

import numpy as np
import pytest
import yaml

import reacher_np as rn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
NAME = "ReacherBulletEnv-v0"


def f32(*v):
    return np.array(v, np.float32).reshape(-1, 2)


def col(th, w1, g, w2, tx=0.0, ty=0.0):
    s = np.array([th, w1, g, w2, tx, ty, 0.0], np.float64).reshape(-1, 1)
    s[6] = rn.potential(s, rn.trig(s))
    return s


# ---- the equations ---------------------------------------------------------------------------------------------------------------
ENERGY_STARTS = {"elbow-swinging": (0.3, 3.0, 0.5, -2.0), "folding": (-2.0, 1.5, -0.4, 3.0), "slow": (1.0, -0.7, 1.2, 0.9)}


@pytest.mark.parametrize("case", sorted(ENERGY_STARTS))
def test_energy_is_conserved_in_the_limit(case):
    """With D = 0, no torque and the elbow clear of its limit the arm is conservative (the plane is horizontal: the energy is
    the kinetic energy of the two rods and the two rotors, written in reacher_np.kinetic_energy from the rods' velocities, not
    from the mass matrix), and semi-implicit Euler is first order: over 1 s the worst relative drift shrinks 4 x when dt does.
    The issue's window is 3 ... 5 x per refinement (dt, dt / 4, dt / 16).  A wrong mass-matrix or Coriolis term leaves an
    error that does not shrink."""
    drift = []
    for k in (1, 4, 16):
        s = col(*ENERGY_STARTS[case])
        e0 = rn.kinetic_energy(s)[0]
        worst, reach = 0.0, 0.0
        for _ in range(int(round(1.0 / (rn.DT / k)))):
            s = rn.step(s, f32(0.0, 0.0), dt=rn.DT / k, damping=0.0)[0]
            worst = max(worst, abs(rn.kinetic_energy(s)[0] - e0) / e0)
            reach = max(reach, abs(s[2, 0]))
        assert reach < 2.9, (case, reach)                         # never at the elbow limit
        drift.append(worst)
    ratios = [drift[0] / drift[1], drift[1] / drift[2]]
    print(case, "relative drift", drift, "ratios", ratios)
    assert drift[0] > 1e-5                                        # (there is something to shrink)
    for r in ratios:
        assert 3.0 <= r <= 5.0, (case, ratios)


def test_zero_action_never_raises_the_kinetic_energy():
    """Viscous damping only takes energy out, and the elbow limit only zeroes a rate.  Semi-implicit Euler's own energy error
    is second order per step (1e-3 relative over a whole second, above) and the damping term first order (dt D / M ~ 0.08 per
    step), so the decrease holds step by step."""
    rng = np.random.default_rng(2)
    n = 400
    s = rn.reset(rng.uniform(-1, 1, (n, 4)).astype(np.float32))
    s[1], s[3] = rng.uniform(-6, 6, n), rng.uniform(-6, 6, n)
    ke = rn.kinetic_energy(s)
    hit = 0
    for _ in range(150):
        s = rn.step(s, np.zeros((n, 2), np.float32))[0]
        new = rn.kinetic_energy(s)
        assert (new <= ke).all(), (new - ke).max()
        ke = new
        hit += int((np.abs(s[2]) == 3.0).sum())
    assert hit > 0                                                # some elbows ran into the limit on the way
    assert (ke < 1e-3 * rn.kinetic_energy(col(0.0, 6.0, 0.0, 6.0))[0]).all()


def test_the_limit_clips_the_angle_and_zeroes_outward_rates_only():
    for side in (1.0, -1.0):
        # driven into the limit: g exactly +-3, w2 exactly 0, w1 untouched by the limit
        for g0, w20 in ((side * 2.99, side * 5.0), (side * 3.0, side * 0.5), (side * 3.2, side * 0.1)):
            s = rn.step(col(0.2, 0.3, g0, w20), f32(0.0, 0.0))[0]
            assert s[2, 0] == side * 3.0 and s[3, 0] == 0.0 and s[1, 0] != 0.0, (g0, w20, s[:4, 0])
        # moving away from it: the plain integration result
        s = rn.step(col(0.2, 0.3, side * 3.0, -side * 2.0), f32(0.0, 0.0))[0]
        assert abs(s[2, 0]) < 3.0 and s[3, 0] * side < -1.0
        # clipped from outside with an inward rate: the angle is clipped, the rate kept
        s = rn.step(col(0.2, 0.0, side * 3.5, -side * 2.0), f32(0.0, 0.0))[0]
        assert s[2, 0] == side * 3.0 and s[3, 0] * side < -1.0


def test_actions_are_clipped_to_one():
    s0 = col(0.4, 0.5, -0.7, 1.0, 0.1, -0.05)
    up = np.nextafter(np.float32(1.0), np.float32(2.0))
    for slot in (0, 1):
        for big, one in ((4.0, 1.0), (-4.0, -1.0), (up, 1.0), (-up, -1.0)):
            a, b = [0.3, 0.3], [0.3, 0.3]
            a[slot], b[slot] = big, one
            x, y = rn.step(s0, f32(*a)), rn.step(s0, f32(*b))
            assert np.array_equal(x[0].view(np.uint64), y[0].view(np.uint64)) and x[2][0] == y[2][0]     # state and reward
            assert np.array_equal(x[1], y[1])
        a, b = [0.3, 0.3], [0.3, 0.3]
        a[slot] = 0.5
        assert not np.array_equal(rn.step(s0, f32(*a))[0], rn.step(s0, f32(*b))[0])


def test_the_idle_return_is_exactly_zero():
    """Rates 0 and actions 0: no acceleration, the state is a fixed point, the potential difference and both costs are 0.  The
    stuck-joint term is the one exception the definition makes: a reset with | |g| - 1 | < 0.01 (probability 0.0067) pays 0.1
    per step also when idle, so those resets return -15 (150 steps of -0.1 added up in float64) and all others 0."""
    rng = np.random.default_rng(1)
    init = rng.uniform(-1, 1, (300, 4)).astype(np.float32)
    init[:3, 3] = (1.0 / 3.0, -0.3345, 0.3301)                    # g = 3 u inside the band
    s0 = rn.reset(init)
    stuck = np.abs(np.abs(s0[2]) - 1.0) < 0.01
    assert stuck[:3].all() and stuck.sum() < 10
    s, ret = s0, np.zeros(300)
    for _ in range(150):
        s, _, r, d = rn.step(s, np.zeros((300, 2), np.float32))
        ret = ret + r
        assert not d.any()
    assert np.array_equal(s.view(np.uint64), s0.view(np.uint64))
    assert (ret[~stuck] == 0.0).all()
    want = 0.0
    for _ in range(150):
        want = want - 0.1
    assert (ret[stuck] == want).all()


def test_reset_observation_and_reward_terms():
    init = np.array([[0.5, -0.25, 0.5, 0.0], [0.0, 0.0, 0.0, 1.0]], np.float32)
    s = rn.reset(init)
    assert s.shape == (7, 2) and np.array_equal(s[4:6, 0], [0.135, -0.0675]) and s[0, 0] == rn.PI * 0.5 and s[2, 1] == 3.0
    obs = rn.obs_of(s)
    assert obs.dtype == np.float32 and obs.shape == (2, 9)
    # th = pi / 2, g = 0: the arm points along +y, fingertip (0, 0.21)
    assert abs(obs[0, 2] - (0.0 - 0.135)) < 1e-7 and abs(obs[0, 3] - (0.21 + 0.0675)) < 1e-7
    assert abs(s[6, 0] + 100.0 * np.hypot(0.135, 0.21 + 0.0675)) < 1e-12
    # fingertip exactly on the target: distance 0, potential -0
    on = col(0.0, 0.0, 0.0, 0.0, 0.1 + 0.11, 0.0)
    assert on[6, 0] == 0.0
    # moving towards the target is rewarded by 100 x the distance gained, minus the costs
    s0 = col(0.0, 2.0, 0.5, 0.0, 0.0, 0.15)
    ns, _, r, _ = rn.step(s0, f32(0.5, -0.25))
    gain = ns[6, 0] - s0[6, 0]
    assert gain > 0 and r.dtype == np.float64
    assert r[0] == ((gain - 0.10 * (abs(0.5 * ns[1, 0]) + abs(-0.25 * ns[3, 0]))) - 0.01 * (0.5 + 0.25))
    # the stuck-joint band: | |g| - 1 | < 0.01 of the NEW angle
    for g, want in ((1.0, True), (-1.0, True), (0.9901, True), (0.99, False), (1.0099, True), (1.0101, False), (0.0, False)):
        base = rn.step(col(0.3, 0.0, g, 0.0), f32(0.0, 0.0))
        assert base[0][2, 0] == g and (base[2][0] == -0.1) == want, g


# ---- wrappers, configs, constants ------------------------------------------------------------------------------------------------
def test_python_layer_agrees_with_the_restatement():
    import builder
    from envs.gym_wrapper import SUPPORTED, GymWrapper
    from ses import _lib
    from ses.device import ENV_IDS
    assert _lib.ENV_REACHER == 13 and ENV_IDS[NAME] == 13
    assert SUPPORTED[NAME] == dict(num_state=rn.S, num_action=rn.A, discrete=False, time_limit=rn.TIME_LIMIT) and rn.TIME_LIMIT == 150
    env = builder.build_env({"name": NAME, "max_step": "None", "pomdp": False})
    assert isinstance(env, GymWrapper) and env.horizon == 150 and env.variant == "pybullet-restated"
    assert GymWrapper(NAME, 40).horizon == 40 and GymWrapper(NAME, 10 ** 6).horizon == 150
    with pytest.raises(AssertionError):
        GymWrapper(NAME, None, pomdp=True)
    with pytest.raises(NotImplementedError):
        GymWrapper("HalfCheetahBulletEnv-v0", None)
    text = open(os.path.join(ROOT, "include", "ses.h")).read()
    assert "#define SES_ENV_REACHER 13 " in text


def test_init_rows_agree_with_the_restatement(monkeypatch):
    """HipES's init_dim / init_range without a device: the constructor is run up to the point where it needs one."""
    import torch
    from ses import device as dv

    class Stop(Exception):
        pass

    def fake_config(*args):
        raise Stop

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(dv, "SesConfig", fake_config)
    es = dv.HipES.__new__(dv.HipES)
    with pytest.raises(Stop):
        es.__init__(NAME, rn.S, rn.A, False, False, max_step=10, eval_ep_num=1)
    assert (es.init_dim, es.init_range) == (rn.INIT_DIM, rn.INIT_RANGE)


@pytest.mark.parametrize("conf,strategy", [("reacher", "openai_es"), ("reacher_sep_cma", "sep_cma_es")])
def test_the_configs_build_a_strategy_and_a_network(conf, strategy):
    import builder
    cfg = yaml.load(open(os.path.join(SRC, "conf", conf + ".yaml")), Loader=yaml.FullLoader)
    env = builder.build_env(cfg["env"])
    net = builder.build_network(cfg["network"])
    strat = builder.build_strategy(cfg["strategy"])
    assert env.name == NAME and env.horizon == 150 and cfg["env"]["max_step"] == 150
    assert (net.num_state, net.num_action, net.discrete_action, net.use_gru) == (9, 2, False, False)
    assert net.param_count() == 386
    assert strat is not None and cfg["strategy"]["name"] == strategy and cfg["strategy"]["offspring_num"] == 256
    base = yaml.load(open(os.path.join(SRC, "conf", "reacher.yaml")), Loader=yaml.FullLoader)
    assert cfg["env"] == base["env"] and cfg["network"] == base["network"]


def _create(S, A, discrete=0, gru=0, pomdp=0, physics64=0, lanes=0):
    from ses import _lib
    lib = _lib.load()
    cfg = _lib.SesConfig(13, S, A, discrete, gru, pomdp, 100, 5, 0, lanes, 1, physics64)
    h = ctypes.c_void_p()
    rc = lib.ses_create(ctypes.byref(cfg), None, ctypes.byref(h))
    msg = lib.ses_last_error().decode() if rc != _lib.SES_OK else ""
    if rc == _lib.SES_OK:
        lib.ses_destroy(h)
    return rc, msg


def test_ses_create_validates_the_env_by_name():
    from ses import _lib
    ok = (_lib.SES_OK, -4)                                              # SES_ERR_NO_DEVICE on a machine without a GPU
    assert _create(9, 2)[0] in ok
    assert _create(9, 2, gru=1)[0] in ok
    assert _create(9, 2, lanes=32)[0] in ok
    assert _lib.load().ses_param_count(9, 2, 0) == 386 and _lib.load().ses_param_count(9, 2, 1) == 6722
    for bad, word in ((dict(S=10), "num_state"), (dict(S=5), "num_state"), (dict(A=1), "num_action"), (dict(discrete=1), "discrete_action"),
                      (dict(pomdp=1), "pomdp"), (dict(physics64=1), "physics64"), (dict(gru=2), "gru")):
        kw = dict(S=9, A=2)
        kw.update(bad)
        rc, msg = _create(**kw)
        assert rc == -1, bad                                            # SES_ERR_INVALID_ARG
        assert "ReacherBulletEnv-v0" in msg and word in msg, (bad, msg)
