"""HopperBulletEnv-v0 on the host (tests/hopper_host.py: csrc/ses_hopper_env.h compiled for the CPU): the physics against things
that are not the code under test -- the centre of mass in free flight against the discrete parabola, the joints' integrity and the
ground under random actions, the reward's bookkeeping against numpy float32, the observation's constants and clip, termination --
and the Python layer without a device.

The "measured" bounds were measured with this host build (the figure stands beside each assertion and in DESIGN.md 7) and are
asserted at four times the measurement: the margin covers float32 accumulation order between compilers, not a wrong equation.

Episodes.  Nothing open-loop keeps this hopper up: the zero policy stands for 77 steps from the zero init row and 32 - 43 from
rows of the full range, a first-generation policy falls within 3 - 40.  So no run here reaches the TimeLimit of 1000, and "the cap"
an episode can reach in this file is CAP = 60 steps, the horizon of the device tests (tests/test_gpu_hopper.py): the reference
runs are eight at full action amplitude from rows of the full init range (they end early) and, as extras, four at amplitude
0.0001 from the zero row (they are alive at CAP); each is stepped on to 1000 steps, through and past its fall.  The bounds are
taken twice: over the steps up to an episode's first done -- the hopper as a policy meets it -- and over all 1000."""
import os

import numpy as np
import pytest
import yaml

import hopper_host as hh
from oracle import c_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
NAME = hh.NAME
F32 = np.float32
DT = float(F32(0.0165) / F32(4.0))                  # one world step, as the env forms it
G = float(F32(-9.8))
ANGULAR_SLOP = 2.0 / 180.0 * np.pi
CAP = 60
STEPS = 1000


def reference_runs():
    """the twelve runs (eight loud, four quiet): per step the diagnostics that the bounds are taken over; (first done step or None, rows)"""
    rng = np.random.default_rng(20261021)
    out = []
    for k in range(12):
        loud = k < 8
        sim = hh.HopperSim()
        sim.reset(rng.uniform(-0.1, 0.1, 3).astype(F32) if loud else np.zeros(3, F32))
        first_done, rows = None, []
        for t in range(STEPS):
            a = (rng.uniform(-1.0, 1.0, 3) * (1.0 if loud else 0.0001)).astype(F32)
            obs, r, done = sim.step(a)
            d = sim.debug()
            if done and first_done is None:
                first_done = t + 1
            over = max(float(np.max(d["limits"][:, 0] - d["angles"])), float(np.max(d["angles"] - d["limits"][:, 1])))
            rows.append((float(d["sep"].max()), over, d["lowest_solved"], obs, float(r), sim.terms.copy()))
        out.append((first_done, rows))
    return out


@pytest.fixture(scope="module")
def runs():
    return reference_runs()


# ---- a. free flight -----------------------------------------------------------------------------------------------------------
def test_centre_of_mass_follows_the_discrete_parabola_in_free_flight():
    """The chain lifted 2 m, every body given the same linear velocity and a random spin (joint speeds of at most 0.4 rad/s: from
    thigh and leg angles of -0.09 no limit is reached in 40 world steps), zero action.  After every world step the centre of
    mass of the four bodies is where semi-implicit Euler puts a point mass: v += dt g, then c += dt v.  Joint impulses and
    position corrections are internal and must not move it.  Measured here: 4.3e-7 m over the 40 steps."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for trial in range(6):
        sim = hh.HopperSim()
        sim.reset(np.array([-0.09, -0.09, 0.0], F32))
        d = sim.debug()
        bodies, m = d["bodies"].copy(), d["masses"].astype(np.float64)
        v0 = rng.uniform(-1.0, 1.0, 2)
        bodies[:, 1] += F32(2.0)
        bodies[:, 3], bodies[:, 4] = F32(v0[0]), F32(v0[1])
        bodies[:, 5] = rng.uniform(-0.2, 0.2, 4).astype(F32)
        sim.set_bodies(bodies)
        b = sim.debug()["bodies"].astype(np.float64)
        c = (m[:, None] * b[:, 0:2]).sum(0) / m.sum()
        v = (m[:, None] * b[:, 3:5]).sum(0) / m.sum()
        for n in range(40):
            sim.world_step()
            d = sim.debug()
            v = v + DT * np.array([0.0, G])
            c = c + DT * v
            b = d["bodies"].astype(np.float64)
            got = (m[:, None] * b[:, 0:2]).sum(0) / m.sum()
            worst = max(worst, float(np.abs(got - c).max()))
            assert d["contact_points"] == 0 and not d["foot_contact"] and d["limit_states"] == [0, 0, 0], (trial, n)
        assert d["lowest"] > 1.0                                        # still in the air
    print("free flight: worst centre-of-mass deviation", worst)
    assert worst <= 4 * 4.3e-7, worst


# ---- b, c. joints and ground under random actions -----------------------------------------------------------------------------
# measured with this host build (module docstring): (up to the first done, over all 1000 steps)
MEASURED_SEP = (1.7e-3, 7.0e-3)                   # m
MEASURED_OVER = (1.82, 8.0)                  # ANGULAR_SLOP
MEASURED_DEPTH = 0.0158                             # m below the ground line (inside the 0.02 m contact skin's reach)


def worst(runs, col, pre, lowest=False):
    vals = [r[col] for first, rows in runs for r in (rows[:first] if pre else rows)]
    return min(vals) if lowest else max(vals)


def test_joints_hold_together_and_stay_inside_their_limits(runs):
    """Largest distance between the two bodies' images of a joint's anchor, and the farthest a joint angle gets outside its limits
    (in units of ANGULAR_SLOP, the slack Box2D's position solver leaves).  Up to the first done of each episode: 1.7e-3 m and
    1.82 slops.  Over all 12 x 1000 steps -- most of them after the fall, the torso (whose contacts are not solved) through
    the ground and 150 N m held against a limit: 7.0e-3 m and 8.0 slops (16 degrees); that excess is a finding about 150 N m against 8
    velocity iterations, and the loose bound is kept for the thrashing only."""
    for pre in (True, False):
        sep, over = worst(runs, 0, pre), worst(runs, 1, pre) / ANGULAR_SLOP
        print("joint integrity", "up to the first done:" if pre else "all steps:", "anchor separation", sep, "limit excess in slops", over)
        assert sep <= 4 * MEASURED_SEP[0 if pre else 1], (pre, sep)
        assert over <= 4 * MEASURED_OVER[0 if pre else 1], (pre, over)


def test_no_solved_body_sinks_into_the_ground(runs):
    """The lowest vertex of thigh, leg and foot over the same runs.  Measured here: at the lowest 0.0158 m below the ground
    line, in the thrashing after a fall (the position solver's correction is capped per step).  The derived bound is what "no
    tunnelling without continuous collision" means: never deeper than the thinnest body is thick (0.08 m)."""
    low = worst(runs, 2, False, lowest=True)
    print("ground: lowest vertex of a solved body", low)
    assert low > -0.08
    assert low >= -4 * MEASURED_DEPTH, low


def test_body_tables_are_the_capsules_masses_on_uniform_boxes():
    """The generated tables against the specification, not against themselves: mass 1000 (pi r^2 L + 4/3 pi r^3) of the capsule, the
    box (L + 2r) x 2r, inertia m (w^2 + h^2) / 12 of the uniform box.  float32 tables built by Box2D's polygon sums: 1e-5 relative."""
    caps = [(0.40, 0.05, False), (0.45, 0.05, False), (0.50, 0.04, False), (0.39, 0.06, True)]
    props = hh.body_props().astype(np.float64)
    for (L, r, horizontal), (m, inertia, hx, hy) in zip(caps, props):
        want_m = 1000.0 * (np.pi * r * r * L + 4.0 / 3.0 * np.pi * r ** 3)
        w, h = (L + 2 * r, 2 * r) if horizontal else (2 * r, L + 2 * r)
        assert abs(2 * hx - w) <= 1e-6 and abs(2 * hy - h) <= 1e-6
        assert abs(m - want_m) <= 1e-5 * want_m, (m, want_m)
        assert abs(inertia - want_m * (w * w + h * h) / 12.0) <= 1e-5 * inertia, (inertia, want_m * (w * w + h * h) / 12.0)
    assert np.allclose(hh.HopperSim().debug()["masses"], props[:, 0])


# ---- d. reward bookkeeping -------------------------------------------------------------------------------------------------------
def test_reward_terms_are_the_numpy_float32_ones_and_progress_telescopes():
    """Every step of four episodes under random actions: the alive, progress, electricity and joints-at-limit terms recomputed in
    numpy float32 from the diagnostics (torso before and after, the observation after, the clipped action) equal the env's, and
    their sum in the env's order equals the returned reward, bit for bit.  The progress terms of an episode sum to
    (x_T - x_0) / 0.0165: each term is fl(fl(x1 - x0) / dt), two roundings of at most 2^-24 relative each, and the sum is taken in
    float64 here as the rollouts take it, so the error is below 2.5 * 2^-24 * sum |term| (the float64 additions are orders below)."""
    rng = np.random.default_rng(4)
    dt = F32(0.0165)
    for ep in range(4):
        sim = hh.HopperSim()
        sim.reset(rng.uniform(-0.1, 0.1, 3).astype(F32))
        x_start = x0 = sim.debug()["bodies"][0, 0]
        total, total_abs = 0.0, 0.0
        for t in range(60):
            raw = (rng.uniform(-1.5, 1.5, 3) * (1.0 if ep < 2 else 0.05)).astype(F32)
            obs, r, done = sim.step(raw)
            d = sim.debug()
            a = np.clip(raw, F32(-1.0), F32(1.0))
            x1, y1 = d["bodies"][0, 0], d["bodies"][0, 1]
            alive = F32(1.0) if (y1 > F32(0.8) and abs(obs[7]) < F32(1.0)) else F32(-1.0)
            progress = F32(x1 - x0) / dt
            work, sq, at_limit = F32(0.0), F32(0.0), F32(0.0)
            for j in range(3):
                work = work + abs(F32(a[j] * obs[9 + 2 * j]))
                sq = sq + F32(a[j] * a[j])
                at_limit = at_limit + (F32(1.0) if abs(obs[8 + 2 * j]) > F32(0.99) else F32(0.0))
            electricity = F32(F32(-2.0) * F32(work / F32(3.0))) - F32(F32(0.1) * F32(sq / F32(3.0)))
            limit = F32(-0.1) * at_limit
            want = np.array([alive, progress, electricity, limit], F32)
            assert np.array_equal(want.view(np.uint32), sim.terms.view(np.uint32)), (ep, t, want, sim.terms)
            assert F32(F32(F32(alive + progress) + electricity) + limit).view(np.uint32) == F32(r).view(np.uint32), (ep, t)
            assert done == (alive < 0 or d["game_over"])
            total += float(progress)
            total_abs += abs(float(progress))
            x0 = x1
            if done:
                break
        exact = (float(x0) - float(x_start)) / float(dt)
        assert abs(total - exact) <= 2.5 * 2.0 ** -24 * total_abs + 1e-300, (ep, total, exact)
        assert total_abs > 0.0


# ---- e. observation ---------------------------------------------------------------------------------------------------------------
def test_observation_constants_clip_and_contact_flag(runs):
    for _, rows in runs:
        for r in rows:
            obs = r[3]
            assert obs[1] == 0.0 and obs[2] == 1.0 and obs[4] == 0.0 and obs[6] == 0.0
            assert (obs >= -5.0).all() and (obs <= 5.0).all() and obs[14] in (0.0, 1.0)
    assert any((np.abs(r[3]) == 5.0).any() for _, rows in runs for r in rows)    # the clip is reached (joint speeds in the thrashing)
    # the hopper starts with its foot 0.04 m above the ground, drops onto it within a few steps and stands: the flag is 1
    sim = hh.HopperSim()
    obs = sim.reset(np.zeros(3, F32))
    assert obs[14] == 0.0 and obs[0] == 0.0
    seen = [sim.step(np.zeros(3, F32))[0][14] for _ in range(10)]
    assert seen[0] == 0.0 and seen[-1] == 1.0 and sim.debug()["contact_points"] >= 1
    # ... and lifted into free flight it is 0 again from the next step on
    b = sim.debug()["bodies"].copy()
    b[:, 1] += F32(2.0)
    sim.set_bodies(b)
    assert sim.step(np.zeros(3, F32))[0][14] == 0.0 and sim.debug()["contact_points"] == 0


# ---- f. termination ---------------------------------------------------------------------------------------------------------------
def test_the_zero_policy_falls_and_the_runs_hold_both_kinds_of_episode(runs):
    sim = hh.HopperSim()
    sim.reset(np.zeros(3, F32))
    for t in range(STEPS):
        obs, r, done = sim.step(np.zeros(3, F32))
        if done:
            break
        assert sim.terms[0] == 1.0
    assert done and 60 < t + 1 < 200 and sim.terms[0] == -1.0            # 77 steps with this build
    d = sim.debug()
    assert d["bodies"][0, 1] <= 0.8 or abs(d["bodies"][0, 2]) >= 1.0
    ends = [first for first, _ in runs]
    assert all(e is not None for e in ends)                              # nothing open-loop stands for 1000 steps (module docstring)
    assert all(e < CAP for e in ends[:8]) and sum(e < 20 for e in ends) >= 4 and sum(e > CAP for e in ends[8:]) >= 2, ends
    for first, rows in runs:                                             # the alive term turns -1 exactly at the first done
        assert all(r[5][0] == 1.0 for r in rows[:first - 1]) and rows[first - 1][5][0] == -1.0


# ---- g. host interface --------------------------------------------------------------------------------------------------------------
def test_python_layer_without_a_device():
    import builder
    from envs.gym_wrapper import PYBULLET_RESTATED, SUPPORTED, GymWrapper
    from ses import _lib
    from ses.device import ENV_IDS
    from ses.envs import REGISTRY
    assert _lib.ENV_HOPPER == 14 and ENV_IDS[NAME] == 14
    assert SUPPORTED[NAME] == dict(num_state=15, num_action=3, discrete=False, time_limit=1000) and NAME in PYBULLET_RESTATED
    assert REGISTRY[NAME].family == "pybullet-hopper" and not REGISTRY[NAME].obs_normalizer and not REGISTRY[NAME].pomdp
    env = builder.build_env({"name": NAME, "max_step": "None", "pomdp": False})
    assert isinstance(env, GymWrapper) and env.horizon == 1000 and env.variant == "pybullet-restated"
    assert GymWrapper(NAME, 40).horizon == 40 and GymWrapper(NAME, 10 ** 6).horizon == 1000
    with pytest.raises(AssertionError):
        GymWrapper(NAME, None, pomdp=True)
    assert "#define SES_ENV_HOPPER 14 " in open(os.path.join(ROOT, "include", "ses.h")).read()
    info = _lib.env_info(env_id=14, num_state=15, num_action=3, discrete_action=0, gru=0, pomdp=0, eval_ep_num=1, n_agents=1, physics64=0)
    assert (info.init_width, info.init_lo, info.init_hi, info.obs_width, info.num_action) == (3, -0.1, 0.1, 15, 3)
    assert info.state_bytes == hh.lib().hop_state_size() and info.action_layout == _lib.ACTION_F32_N_A


@pytest.mark.parametrize("conf,strategy,offspring", [("hopper", "openai_es", 96), ("hopper_ars", "ars", 256), ("hopper_sep_cma", "sep_cma_es", 256)])
def test_configs_build_the_15_32_3_network(conf, strategy, offspring):
    import builder
    cfg = yaml.load(open(os.path.join(SRC, "conf", conf + ".yaml")), Loader=yaml.FullLoader)
    env = builder.build_env(cfg["env"])
    net = builder.build_network(cfg["network"])
    assert builder.build_strategy(cfg["strategy"]) is not None
    assert env.name == NAME and env.horizon == 1000 and cfg["env"]["max_step"] == "None"
    assert (net.num_state, net.num_action, net.discrete_action, net.use_gru) == (15, 3, False, False)
    assert net.param_count() == co.param_count(15, 3, False) == 611 and co.param_count(15, 3, True) == 6947
    assert cfg["strategy"]["name"] == strategy and cfg["strategy"]["offspring_num"] == offspring
    base = yaml.load(open(os.path.join(SRC, "conf", "hopper.yaml")), Loader=yaml.FullLoader)
    assert cfg["env"] == base["env"] and cfg["network"] == base["network"]
