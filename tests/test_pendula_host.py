"""The inverted-pendulum family modelled on pybullet_envs on the host side (no GPU needed).  tests/pendula_np.py restates
DESIGN.md 7 and the device code is held to it bit for bit, so a derivation error would be copied faithfully: these tests are
what checks the equations themselves -- energy conservation in the limit dt -> 0, the upright fixed point, the rail, the
termination thresholds and rewards -- plus the wrapper, the seven configs and the constants of the Python layer."""
import ctypes
import os

import numpy as np
import pytest
import yaml

import pendula_np as pn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
BALANCE, SWINGUP, DOUBLE = "InvertedPendulumBulletEnv-v0", "InvertedPendulumSwingupBulletEnv-v0", "InvertedDoublePendulumBulletEnv-v0"
NAMES = (BALANCE, SWINGUP, DOUBLE)
CONFIGS = {"inverted_pendulum": BALANCE, "double_pendulum": DOUBLE, "pendulum_swingup": SWINGUP, "pendulum_swingup_pgpe": SWINGUP,
           "pendulum_swingup_sep_cma": SWINGUP, "pendulum_swingup_lm_ma": SWINGUP, "pendulum_swingup_ma_es": SWINGUP}


def f32(*v):
    return np.array(v, np.float32)


def col(*v):
    return np.array(v, np.float64).reshape(-1, 1)


# ---- energy: kinetic plus potential energy of the cart and the rods, from first principles ------------------------------------
# A uniform rod of mass m and length 2 l has the moment of inertia m (2 l)^2 / 12 about its centre; its kinetic energy is that of
# its centre of mass plus the rotation about it.  Angles are measured from the upward vertical, positive towards +x.
def rod_energy(m, half, cx, cy, vx, vy, rate):
    inertia = m * (2.0 * half) ** 2 / 12.0
    return 0.5 * m * (vx * vx + vy * vy) + 0.5 * inertia * rate * rate + m * pn.G * cy


def energy_single(s):
    x, v, th, w = s
    half = 0.3
    e_cart = 0.5 * 10.472 * v * v
    return e_cart + rod_energy(5.0186, half, x + half * np.sin(th), half * np.cos(th), v + half * w * np.cos(th), -half * w * np.sin(th), w)


def energy_double(s):
    x, v, t1, w1, t2, w2 = s
    half, length, m = 0.3, 0.6, 4.1987
    b, wb = t1 + t2, w1 + w2                                  # the second rod's absolute angle and rate
    e_cart = 0.5 * 10.472 * v * v
    hx, hy = x + length * np.sin(t1), length * np.cos(t1)    # the second hinge
    hvx, hvy = v + length * w1 * np.cos(t1), -length * w1 * np.sin(t1)
    return (e_cart + rod_energy(m, half, x + half * np.sin(t1), half * np.cos(t1), v + half * w1 * np.cos(t1), -half * w1 * np.sin(t1), w1) +
            rod_energy(m, half, hx + half * np.sin(b), hy + half * np.cos(b), hvx + half * wb * np.cos(b), hvy - half * wb * np.sin(b), wb))


def energy_drift(step, energy, start, seconds, dt):
    s = col(*start)
    e0 = energy(s)[0]
    worst, reach = 0.0, 0.0
    for _ in range(int(round(seconds / dt))):
        s = step(s, f32(0.0), dt=dt, force=0.0)[0]
        worst = max(worst, abs(energy(s)[0] - e0))
        reach = max(reach, abs(s[0, 0]))
    return worst, reach


ENERGY_CASES = {"single-falling": (pn.balance_step, energy_single, (0.0, 0.0, 0.5, 0.0)),
                "single-swinging": (pn.balance_step, energy_single, (0.1, 0.0, 3.0, -2.0)),
                "double-falling": (pn.double_step, energy_double, (0.0, 0.0, 0.3, 0.0, 0.2, 0.0)),
                "double-hanging": (pn.double_step, energy_double, (0.0, 0.0, 2.5, 0.0, 0.5, 0.0))}


@pytest.mark.parametrize("case", sorted(ENERGY_CASES))
def test_energy_is_conserved_in_the_limit(case):
    """With the motor off and the cart clear of the rail the system is conservative, and the integrator is first order: over a
    fixed 0.495 s (30 steps at dt) the worst |E(t) - E(0)| halves with every halving of dt.  A wrong mass-matrix or right-hand
    side term leaves an error that does not shrink: a ratio near 1.
    Observed here (dt -> dt/2, dt/2 -> dt/4): single-falling 0.526 0.514; single-swinging 0.513 0.506; double-falling 0.502
    0.501; double-hanging 0.523 0.511 -- all within 0.03 of 0.5, so the window is 0.5 +- 0.05.  The drift itself at dt is
    0.08 ... 1.3 J of |E| between 15 and 50 J, and at dt / 64 it is 1 / 64 of that."""
    step, energy, start = ENERGY_CASES[case]
    drift = []
    for k in (1, 2, 4):
        worst, reach = energy_drift(step, energy, start, 0.495, pn.DT / k)
        assert reach < 0.9, (case, reach)                     # the cart stays off the rail
        drift.append(worst)
    ratios = [drift[1] / drift[0], drift[2] / drift[1]]
    print(case, "drift", drift, "ratios", ratios)
    assert drift[0] > 1e-3                                    # (there is something to halve)
    for r in ratios:
        assert 0.45 <= r <= 0.55, (case, ratios)


# ---- fixed point, rail, termination, rewards --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_upright_at_rest_is_a_fixed_point(name):
    e = pn.ENVS[name]
    s0 = np.zeros((e["state_dim"], 1))
    s = s0
    for _ in range(5):
        s, obs, r, d = e["step"](s, f32(0.0))
        assert np.array_equal(s.view(np.uint64), s0.view(np.uint64)) and not d[0]
    if name == DOUBLE:
        assert tuple(obs[0]) == (0, 0, 0, 1, 0, 0, 1, 0, 0) and r[0] == 10.0 - (0.9 + 0.3 - 2.0) * (0.9 + 0.3 - 2.0)
    else:
        assert tuple(obs[0]) == (0, 0, 1, 0, 0) and r[0] == 1.0
    assert obs.dtype == np.float32 and r.dtype == np.float64


@pytest.mark.parametrize("name", NAMES)
def test_the_rail_stops_the_cart(name):
    e = pn.ENVS[name]
    rest = [0.0] * (e["state_dim"] - 2)
    if name == SWINGUP:
        rest[0] = 3.1415
    for side in (1.0, -1.0):
        # driven into the rail: x exactly +-1, v exactly 0
        for x0, v0, a in ((side * 0.99, side * 2.0, side), (side * 1.0, side * 0.5, 0.0), (side * 1.0, 0.0, side), (side * 1.3, side * 0.1, 0.0)):
            s = e["step"](col(x0, v0, *rest), f32(a))[0]
            assert s[0, 0] == side and s[1, 0] == 0.0, (name, x0, v0, a, s[:2, 0])
        # moving away from it: untouched by the rail (the plain integration result)
        s = e["step"](col(side * 1.0, -side * 0.5, *rest), f32(-side))[0]
        assert abs(s[0, 0]) < 1.0 and s[1, 0] * side < -0.5
        # clipped from outside with an inward velocity: the position is clipped, the velocity kept
        s = e["step"](col(side * 1.5, -side * 0.5, *rest), f32(0.0))[0]
        assert s[0, 0] == side and s[1, 0] * side < 0.0


def test_balance_terminates_beyond_0_2():
    up, dn = np.nextafter(0.2, 1.0), np.nextafter(0.2, 0.0)
    for th, want in ((0.2, False), (up, True), (dn, False), (-0.2, False), (-up, True), (-dn, False), (0.0, False), (3.0, True)):
        s, _, r, d = pn.balance_step(col(0.0, 0.0, th, 0.0), f32(0.0), dt=0.0)       # dt = 0: the new state is the old one
        assert s[2, 0] == th and bool(d[0]) == want and r[0] == 1.0, th


def test_swingup_rewards_the_cosine_of_the_new_angle_and_never_ends():
    rng = np.random.default_rng(0)
    s0 = np.stack([rng.uniform(-1, 1, 500), rng.uniform(-2, 2, 500), rng.uniform(-80, 80, 500), rng.uniform(-10, 10, 500)])
    s, obs, r, d = pn.swingup_step(s0, rng.uniform(-1.2, 1.2, 500).astype(np.float32))
    assert not d.any() and r.dtype == np.float64
    assert np.array_equal(r.astype(np.float32), obs[:, 2])          # the same cos theta' the next observation shows
    assert np.abs(r - np.cos(s[2])).max() < 1e-15
    assert pn.swingup_reset(f32(0.05)[None, :])[2, 0] == 3.1415 + float(np.float32(0.05))
    assert pn.swingup_step(pn.swingup_reset(f32(0.0)[None, :]), f32(0.0))[2][0] < -0.999     # hanging: reward ~ -1


def test_double_terminates_when_the_tip_is_down_to_1():
    def probe(th1, th2=0.0):
        s, _, r, d = pn.double_step(col(0.0, 0.0, th1, 0.0, th2, 0.0), f32(0.0), dt=0.0)
        x2, y2 = pn.double_tip(s, pn.double_trig(s))
        return bool(d[0]), y2[0] + 0.3, r[0], x2[0]

    # straight rods (theta2 = 0): y2 + 0.3 = 0.9 cos theta1 + 0.3 falls through 1 at cos theta1 = 7 / 9
    lo, hi = 0.5, 0.9
    assert probe(lo)[0] is False and probe(hi)[0] is True
    while np.nextafter(lo, hi) < hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if not probe(mid)[0] else (lo, mid)
    assert abs(np.cos(lo) - 7.0 / 9.0) < 1e-15
    for th1, want in ((lo, False), (hi, True), (-lo, False), (-hi, True)):        # the adjacent doubles on both sides
        done, h, r, x2 = probe(th1)
        assert done == want and (h <= 1.0) == want, (th1, h)
        assert r == (10.0 - 0.01 * (x2 * x2)) - (h - 2.0) * (h - 2.0)
    # folded back on itself the centre of the second rod sits at 0.3 cos theta1: always down
    assert probe(0.0, np.pi)[0] is True and probe(0.0, 0.1)[0] is False


@pytest.mark.parametrize("name", NAMES)
def test_actions_are_clipped_to_one(name):
    e = pn.ENVS[name]
    s0 = np.zeros((e["state_dim"], 1))
    s0[2, 0] = 0.05
    for big, one in ((4.0, 1.0), (-4.0, -1.0), (np.nextafter(np.float32(1.0), np.float32(2.0)), 1.0)):
        a, b = e["step"](s0, f32(big)), e["step"](s0, f32(one))
        assert np.array_equal(a[0], b[0]) and a[2][0] == b[2][0]
    assert not np.array_equal(e["step"](s0, f32(0.5))[0], e["step"](s0, f32(1.0))[0])


# ---- wrappers, configs, constants ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_python_layer_agrees_with_the_restatement(name):
    import builder
    from envs.gym_wrapper import SUPPORTED, GymWrapper
    from ses import _lib
    from ses.device import ENV_IDS
    e = pn.ENVS[name]
    assert (_lib.ENV_INVERTED_PENDULUM, _lib.ENV_PENDULUM_SWINGUP, _lib.ENV_DOUBLE_PENDULUM) == (9, 10, 11)
    assert ENV_IDS[name] == 9 + NAMES.index(name)
    assert SUPPORTED[name] == dict(num_state=e["S"], num_action=1, discrete=False, time_limit=1000) and e["time_limit"] == 1000
    env = builder.build_env({"name": name, "max_step": "None", "pomdp": False})
    assert isinstance(env, GymWrapper) and env.horizon == 1000 and env.variant == "pybullet-restated"
    assert GymWrapper(name, 150).horizon == 150 and GymWrapper(name, 10 ** 6).horizon == 1000
    with pytest.raises(AssertionError):
        GymWrapper(name, None, pomdp=True)
    with pytest.raises(NotImplementedError):
        GymWrapper("HalfCheetahBulletEnv-v0", None)


@pytest.mark.parametrize("name", NAMES)
def test_init_rows_agree_with_the_restatement(name, monkeypatch):
    """HipES's init_dim / init_range without a device: the constructor is run up to the point where it needs one."""
    import torch
    from ses import device as dv
    e = pn.ENVS[name]
    seen = {}

    class Stop(Exception):
        pass

    def fake_config(*args):
        raise Stop

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(dv, "SesConfig", fake_config)
    es = dv.HipES.__new__(dv.HipES)
    with pytest.raises(Stop):
        es.__init__(name, e["S"], 1, False, False, max_step=10, eval_ep_num=1)
    seen = (es.init_dim, es.init_range)
    assert seen == (e["init_dim"], e["init_range"])


@pytest.mark.parametrize("conf", sorted(CONFIGS))
def test_the_configs_build_a_strategy_and_a_network(conf):
    import builder
    name = CONFIGS[conf]
    e = pn.ENVS[name]
    cfg = yaml.load(open(os.path.join(SRC, "conf", conf + ".yaml")), Loader=yaml.FullLoader)
    env = builder.build_env(cfg["env"])
    net = builder.build_network(cfg["network"])
    strat = builder.build_strategy(cfg["strategy"])
    assert env.name == name and env.horizon == 1000 and cfg["env"]["max_step"] == 1000
    assert (net.num_state, net.num_action, net.discrete_action, net.use_gru) == (e["S"], 1, False, False)
    assert strat is not None
    if conf.startswith("pendulum_swingup"):
        want = {"": "openai_es", "_pgpe": "pgpe", "_sep_cma": "sep_cma_es", "_lm_ma": "lm_ma_es", "_ma_es": "ma_es"}[conf[len("pendulum_swingup"):]]
        assert cfg["strategy"]["name"] == want
        base = yaml.load(open(os.path.join(SRC, "conf", "pendulum_swingup.yaml")), Loader=yaml.FullLoader)
        assert cfg["env"] == base["env"] and cfg["network"] == base["network"]      # the copies differ in the strategy block only
        assert net.param_count() == 225
        if want == "ma_es":
            strat.check_parameters(net.param_count())                               # the full matrix accepts 225 parameters


def _create(env_id, S, A, discrete=0, gru=0, pomdp=0, physics64=0, lanes=0):
    from ses import _lib
    lib = _lib.load()
    cfg = _lib.SesConfig(env_id, S, A, discrete, gru, pomdp, 100, 5, 0, lanes, 1, physics64)
    h = ctypes.c_void_p()
    rc = lib.ses_create(ctypes.byref(cfg), None, ctypes.byref(h))
    if rc == _lib.SES_OK:
        lib.ses_destroy(h)
    return rc


@pytest.mark.parametrize("name", NAMES)
def test_ses_create_validates_the_family(name):
    from ses import _lib
    from ses.device import ENV_IDS
    eid, S = ENV_IDS[name], pn.ENVS[name]["S"]
    ok = (_lib.SES_OK, -4)                                              # SES_ERR_NO_DEVICE on a machine without a GPU
    assert _create(eid, S, 1) in ok
    assert _create(eid, S, 1, gru=1) in ok
    assert _create(eid, S, 1, lanes=32) in ok
    for bad in (dict(S=S + 1), dict(S=14 - S), dict(A=2), dict(discrete=1), dict(pomdp=1), dict(physics64=1), dict(gru=2)):
        kw = dict(S=S, A=1)
        kw.update(bad)
        assert _create(eid, **kw) == -1, bad                            # SES_ERR_INVALID_ARG
