"""Walker2DBulletEnv-v0 on the host (tests/walker2d_host.py: csrc/ses_walker2d_env.h compiled for the CPU): the physics against
things that are not the code under test -- the seven-body centre of mass in free flight against the discrete parabola (with the
hopper's host build through the same protocol as the yardstick), the joints' integrity and the ground under random actions (the
hopper test's own asserted bounds as the yardsticks), the generated tables against the capsule formula, the reward's bookkeeping
against numpy float32, the observation's constants, clip, both foot flags and the two legs' symmetry, termination -- and the
Python layer without a device.

Episodes.  Nothing open-loop keeps this walker up: the zero policy stands for 67 steps from the zero init row, then tips backwards
(pitch reaches +1.0), and falls after 34 - 44 steps from rows of the full range; uniform random actions fell it within 7 - 20.  So no
run here reaches the TimeLimit of 1000, and "the cap" an episode can reach in this file is CAP = 60 steps, the horizon of the
device tests (tests/test_gpu_walker2d.py).  The reference runs are eight at full action amplitude from rows of the full init
range (they end early) and four near-idle ones at amplitude 1e-5 from the zero row (standing with both legs in one place is a knife edge:
torques of 4e-4 N m move the fall between steps 53 and 67, so some of the four are alive at CAP and some are not); each is stepped on to 1000 steps, through and
past its fall.  The bounds are taken twice: over the steps up to an episode's first done and over all 1000."""
import os

import numpy as np
import pytest
import yaml

import hopper_host as hh
import walker2d_host as wh
from oracle import c_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
NAME = wh.NAME
F32 = np.float32
DT = float(F32(0.0165) / F32(4.0))                  # one world step, as the env forms it
G = float(F32(-9.8))
ANGULAR_SLOP = 2.0 / 180.0 * np.pi
CAP = 60
STEPS = 1000
# (L, r, horizontal) of torso, thigh, leg, foot: the specification, not the generator's table
CAPSULES = [(0.40, 0.05, False), (0.45, 0.05, False), (0.50, 0.04, False), (0.20, 0.06, True)]


def reference_runs():
    """the twelve runs (eight loud, four near-idle): per step the diagnostics that the bounds are taken over; (first done step, rows)"""
    rng = np.random.default_rng(20261021)
    out = []
    for k in range(12):
        loud = k < 8
        sim = wh.Walker2dSim()
        sim.reset(rng.uniform(-0.1, 0.1, 6).astype(F32) if loud else np.zeros(6, F32))
        first_done, rows = None, []
        for t in range(STEPS):
            a = (rng.uniform(-1.0, 1.0, 6) * (1.0 if loud else 1e-5)).astype(F32)
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


# ---- free flight ---------------------------------------------------------------------------------------------------------------
def free_flight_deviation(make_sim, row, nb):
    """The chain lifted 2 m, every body given the same linear velocity and a random spin (joint speeds of at most 0.4 rad/s: from
    thigh and leg angles of -0.09 no limit is reached in 40 world steps), zero action.  After every world step the centre of mass
    of the nb bodies is where semi-implicit Euler puts a point mass: v += dt g, then c += dt v.  Returns the worst deviation."""
    rng = np.random.default_rng(1)
    worst = 0.0
    for trial in range(6):
        sim = make_sim()
        sim.reset(np.array(row, F32))
        d = sim.debug()
        bodies, m = d["bodies"].copy(), d["masses"].astype(np.float64)
        v0 = rng.uniform(-1.0, 1.0, 2)
        bodies[:, 1] += F32(2.0)
        bodies[:, 3], bodies[:, 4] = F32(v0[0]), F32(v0[1])
        bodies[:, 5] = rng.uniform(-0.2, 0.2, nb).astype(F32)
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
            assert d["contact_points"] == 0 and not d["foot_contact"] and not any(d["limit_states"]), (trial, n)
        assert d["lowest"] > 1.0                                        # still in the air
    return worst


def test_centre_of_mass_follows_the_discrete_parabola_in_free_flight():
    """Joint impulses and position corrections are internal and must not move the centre of mass -- with two chains meeting in
    body 0 as with one.  The yardstick is the hopper's host build through the same protocol in this same test: Walker2D may
    deviate by 4 x the hopper's worst (the margin covers float32 summation order between compilers and three more bodies in the
    sum).  Measured with these host builds: hopper 4.3e-7 m, Walker2D 3.0e-7 m over the 40 steps."""
    hopper = free_flight_deviation(hh.HopperSim, [-0.09, -0.09, 0.0], 4)
    walker2d = free_flight_deviation(wh.Walker2dSim, [-0.09, -0.09, 0.0, -0.09, -0.09, 0.0], 7)
    print("free flight: worst centre-of-mass deviation, hopper", hopper, "walker2d", walker2d)
    assert hopper > 0.0
    assert walker2d <= 4 * hopper, (walker2d, hopper)
    assert wh.Walker2dSim().debug()["masses"].sum() == pytest.approx(23.68, abs=0.005)


# ---- joints and ground under random actions ---------------------------------------------------------------------------------------
# the hopper test's own asserted bounds (tests/test_hopper_host.py): (up to the first done, over all 1000 steps)
HOPPER_SEP = (1.7e-3, 7.0e-3)                       # m
HOPPER_OVER = (1.82, 8.0)                           # ANGULAR_SLOP


def worst(runs, col, pre, lowest=False):
    vals = [r[col] for first, rows in runs for r in (rows[:first] if pre else rows)]
    return min(vals) if lowest else max(vals)


def test_joints_hold_together_and_stay_inside_their_limits(runs):
    """Largest distance between the two bodies' images of a joint's anchor, and the farthest a joint angle gets outside its limits
    (in units of ANGULAR_SLOP), against 4 x the hopper's measured figures.  Walker2D has about a quarter of the torque on the
    same links and stays inside the hopper's own figures, not only inside four times them.  Measured with this host build: up to
    the first done 1.1e-3 m and 1.49 slops, over all 12 x 1000 steps 2.6e-3 m and 5.65 slops."""
    for pre in (True, False):
        sep, over = worst(runs, 0, pre), worst(runs, 1, pre) / ANGULAR_SLOP
        print("joint integrity", "up to the first done:" if pre else "all steps:", "anchor separation", sep, "limit excess in slops", over)
        assert sep <= 4 * HOPPER_SEP[0 if pre else 1], (pre, sep)
        assert over <= 4 * HOPPER_OVER[0 if pre else 1], (pre, over)


def test_no_solved_body_tunnels_through_the_ground(runs):
    """The lowest vertex of the six solved bodies over the same runs.  The derived bound is what "no tunnelling without continuous
    collision" means: never deeper than the thinnest box is thick (0.08 m, the leg)."""
    low = worst(runs, 2, False, lowest=True)
    print("ground: lowest vertex of a solved body", low)
    assert low > -0.08


def test_body_tables_are_the_capsules_masses_on_uniform_boxes_and_both_legs_equal():
    """The generated tables against the specification, not against themselves: mass 1000 (pi r^2 L + 4/3 pi r^3) of the capsule, the
    box (L + 2r) x 2r, inertia m (w^2 + h^2) / 12 of the uniform box, 1e-5 relative.  The left leg's rows are the right leg's, bit
    for bit."""
    props = wh.body_props()
    assert props.shape == (7, 4)
    assert np.array_equal(props[1:4].view(np.uint32), props[4:7].view(np.uint32))
    for (L, r, horizontal), (m, inertia, hx, hy) in zip(CAPSULES + CAPSULES[1:], props.astype(np.float64)):
        want_m = 1000.0 * (np.pi * r * r * L + 4.0 / 3.0 * np.pi * r ** 3)
        w, h = (L + 2 * r, 2 * r) if horizontal else (2 * r, L + 2 * r)
        assert abs(2 * hx - w) <= 1e-6 and abs(2 * hy - h) <= 1e-6
        assert abs(m - want_m) <= 1e-5 * want_m, (m, want_m)
        assert abs(inertia - want_m * (w * w + h * h) / 12.0) <= 1e-5 * inertia, (inertia, want_m * (w * w + h * h) / 12.0)
    assert np.allclose(wh.Walker2dSim().debug()["masses"], props[:, 0])
    # the chain at the zero row: both legs in the same place, the feet from the ankle (0, 0.10) forward to (0.20, 0.10), lifted by
    # the foot's radius less its height over the ground (0.10 - 0.06 = 0.04 m above it, so no lift)
    sim = wh.Walker2dSim()
    sim.reset(np.zeros(6, F32))
    b = sim.debug()["bodies"]
    assert np.array_equal(b[1:4].view(np.uint32), b[4:7].view(np.uint32))
    assert np.allclose(b[:4, 0:2], [[0.0, 1.25], [0.0, 0.825], [0.0, 0.35], [0.10, 0.10]], atol=1e-6)


# ---- reward bookkeeping -----------------------------------------------------------------------------------------------------------
def test_reward_terms_are_the_numpy_float32_ones_and_progress_telescopes():
    """Every step of four episodes under random actions: the alive, progress, electricity and joints-at-limit terms recomputed in
    numpy float32 from the diagnostics (torso before and after, the observation after, the clipped action) equal the env's, and
    their sum in the env's order equals the returned reward, bit for bit; the means run over six joints.  The progress terms of an
    episode sum to (x_T - x_0) / 0.0165: each term is fl(fl(x1 - x0) / dt), two roundings of at most 2^-24 relative each, and the
    sum is taken in float64 here as the rollouts take it, so the error is below 2.5 * 2^-24 * sum |term|."""
    rng = np.random.default_rng(4)
    dt = F32(0.0165)
    for ep in range(4):
        sim = wh.Walker2dSim()
        sim.reset(rng.uniform(-0.1, 0.1, 6).astype(F32))
        x_start = x0 = sim.debug()["bodies"][0, 0]
        total, total_abs = 0.0, 0.0
        for t in range(60):
            raw = (rng.uniform(-1.5, 1.5, 6) * (1.0 if ep < 2 else 0.05)).astype(F32)
            obs, r, done = sim.step(raw)
            d = sim.debug()
            a = np.clip(raw, F32(-1.0), F32(1.0))
            x1, y1 = d["bodies"][0, 0], d["bodies"][0, 1]
            alive = F32(1.0) if (y1 > F32(0.8) and abs(obs[7]) < F32(1.0)) else F32(-1.0)
            progress = F32(x1 - x0) / dt
            work, sq, at_limit = F32(0.0), F32(0.0), F32(0.0)
            for j in range(6):
                work = work + abs(F32(a[j] * obs[9 + 2 * j]))
                sq = sq + F32(a[j] * a[j])
                at_limit = at_limit + (F32(1.0) if abs(obs[8 + 2 * j]) > F32(0.99) else F32(0.0))
            electricity = F32(F32(-2.0) * F32(work / F32(6.0))) - F32(F32(0.1) * F32(sq / F32(6.0)))
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


# ---- observation -------------------------------------------------------------------------------------------------------------------
def test_observation_constants_clip_and_both_contact_flags(runs):
    for _, rows in runs:
        for r in rows:
            obs = r[3]
            assert obs.shape == (22,)
            assert obs[1] == 0.0 and obs[2] == 1.0 and obs[4] == 0.0 and obs[6] == 0.0
            assert (obs >= -5.0).all() and (obs <= 5.0).all() and obs[20] in (0.0, 1.0) and obs[21] in (0.0, 1.0)
    # the two flags are two bodies' contacts, not one flag twice: in every loud run they differ at some step
    for first, rows in runs[:8]:
        assert any(r[3][20] != r[3][21] for r in rows), first
    assert any(r[3][20] != r[3][21] for first, rows in runs[:8] for r in rows[:first])      # ... also before a first done
    # the clip: a spin of 100 rad/s on the left foot alone makes 0.1 x its joint speed 10, shown as 5
    sim = wh.Walker2dSim()
    obs = sim.reset(np.zeros(6, F32))
    assert obs[20] == 0.0 and obs[21] == 0.0 and obs[0] == 0.0
    b = sim.debug()["bodies"].copy()
    b[6, 5] = F32(100.0)
    sim.set_bodies(b)
    obs = sim.obs()
    assert obs[19] == 5.0 and (np.delete(obs, 19) == np.delete(sim.reset(np.zeros(6, F32)), 19)).all()
    # both feet start 0.04 m above the ground, drop onto it within a few steps and stand: both flags are 1
    seen = [sim.step(np.zeros(6, F32))[0][20:22] for _ in range(10)]
    assert (seen[0] == 0.0).all() and (seen[-1] == 1.0).all() and sim.debug()["contact_points"] >= 2
    # ... and lifted into free flight they are 0 again from the next step on
    b = sim.debug()["bodies"].copy()
    b[:, 1] += F32(2.0)
    sim.set_bodies(b)
    assert (sim.step(np.zeros(6, F32))[0][20:22] == 0.0).all() and sim.debug()["contact_points"] == 0
    # a right leg bent alone lifts the right foot only: [20] is the right foot (body 3), [21] the left (body 6)
    sim.reset(np.zeros(6, F32))
    for _ in range(10):
        sim.step(np.zeros(6, F32))
    lifted = [sim.step(np.array([0.0, -1.0, 0.0, 0.0, 0.0, 0.0], F32))[0][20:22] for _ in range(12)]
    assert any(f[0] == 0.0 and f[1] == 1.0 for f in lifted), lifted
    assert not any(f[0] == 1.0 and f[1] == 0.0 for f in lifted), lifted


# the two legs under equal rows and equal actions: measured with this host build over the runs below
MEASURED_LEG_ASYMMETRY = 0.041                      # of a scaled angle or 0.1 x a joint speed; the flags differed in 4 steps


def leg_asymmetry():
    """Four runs of 60 steps with the same three init values and the same three actions on both legs: the largest difference
    between the legs' observation entries ([8 .. 13] against [14 .. 19], [20] against [21] excluded: a flag flips whole)."""
    rng = np.random.default_rng(7)
    worst_diff, flags_differ = 0.0, 0
    for k in range(4):
        sim = wh.Walker2dSim()
        u = rng.uniform(-0.1, 0.1, 3).astype(F32)
        sim.reset(np.concatenate([u, u]))
        for t in range(60):
            a = (rng.uniform(-1.0, 1.0, 3) * (1.0, 0.3, 0.1, 0.02)[k]).astype(F32)
            obs, r, done = sim.step(np.concatenate([a, a]))
            worst_diff = max(worst_diff, float(np.abs(obs[8:14] - obs[14:20]).max()))
            flags_differ += int(obs[20] != obs[21])
            if done:
                break
    return worst_diff, flags_differ


def test_equal_legs_under_equal_actions_stay_together():
    """The joints are solved in sequence (right leg first), so the legs are not bit-equal; they stay together to 4 x the measured
    difference (0.041, reached in the thrashing of the loudest run just before its done; a leg that took the other's actions or
    rows would differ by the actions' own size, 0.1 - 1)."""
    diff, flags_differ = leg_asymmetry()
    print("leg symmetry: worst difference between the legs' observation entries", diff, "steps with differing flags", flags_differ)
    assert diff <= 4 * MEASURED_LEG_ASYMMETRY, diff


# ---- termination -------------------------------------------------------------------------------------------------------------------
def test_the_zero_policy_falls_and_the_runs_hold_both_kinds_of_episode(runs):
    sim = wh.Walker2dSim()
    sim.reset(np.zeros(6, F32))
    for t in range(STEPS):
        obs, r, done = sim.step(np.zeros(6, F32))
        if done:
            break
        assert sim.terms[0] == 1.0
    assert done and CAP < t + 1 < 200 and sim.terms[0] == -1.0           # 67 steps with this build
    d = sim.debug()
    assert d["bodies"][0, 1] <= 0.8 or abs(d["bodies"][0, 2]) >= 1.0
    ends = [first for first, _ in runs]
    assert all(e is not None for e in ends)                              # nothing open-loop stands for 1000 steps (module docstring)
    assert all(e < CAP for e in ends[:8]) and sum(e < 20 for e in ends) >= 4 and any(e > CAP for e in ends[8:]), ends
    for first, rows in runs:                                             # the alive term turns -1 exactly at the first done
        assert all(r[5][0] == 1.0 for r in rows[:first - 1]) and rows[first - 1][5][0] == -1.0


# ---- host interface ------------------------------------------------------------------------------------------------------------------
def test_python_layer_without_a_device():
    import builder
    from envs.gym_wrapper import PYBULLET_RESTATED, SUPPORTED, GymWrapper
    from ses import _lib
    from ses.device import ENV_IDS
    from ses.envs import REGISTRY
    assert _lib.ENV_WALKER2D == 15 and ENV_IDS[NAME] == 15
    assert SUPPORTED[NAME] == dict(num_state=22, num_action=6, discrete=False, time_limit=1000) and NAME in PYBULLET_RESTATED
    assert REGISTRY[NAME].family == "pybullet-walker2d" and not REGISTRY[NAME].obs_normalizer and not REGISTRY[NAME].pomdp
    env = builder.build_env({"name": NAME, "max_step": "None", "pomdp": False})
    assert isinstance(env, GymWrapper) and env.horizon == 1000 and env.variant == "pybullet-restated"
    assert GymWrapper(NAME, 40).horizon == 40 and GymWrapper(NAME, 10 ** 6).horizon == 1000
    with pytest.raises(AssertionError):
        GymWrapper(NAME, None, pomdp=True)
    with pytest.raises(NotImplementedError):                             # the rest of the family stays refused
        GymWrapper("HalfCheetahBulletEnv-v0", None)
    assert "#define SES_ENV_WALKER2D 15 " in open(os.path.join(ROOT, "include", "ses.h")).read()
    info = _lib.env_info(env_id=15, num_state=22, num_action=6, discrete_action=0, gru=0, pomdp=0, eval_ep_num=1, n_agents=1, physics64=0)
    assert (info.init_width, info.init_lo, info.init_hi, info.obs_width, info.num_action) == (6, -0.1, 0.1, 22, 6)
    assert info.state_bytes == wh.lib().w2d_state_size() and info.action_layout == _lib.ACTION_F32_N_A


@pytest.mark.parametrize("conf,strategy,offspring", [("walker2d", "openai_es", 96), ("walker2d_ars", "ars", 256),
                                                     ("walker2d_sep_cma", "sep_cma_es", 256)])
def test_configs_build_the_22_32_6_network(conf, strategy, offspring):
    import builder
    cfg = yaml.load(open(os.path.join(SRC, "conf", conf + ".yaml")), Loader=yaml.FullLoader)
    env = builder.build_env(cfg["env"])
    net = builder.build_network(cfg["network"])
    assert builder.build_strategy(cfg["strategy"]) is not None
    assert env.name == NAME and env.horizon == 1000 and cfg["env"]["max_step"] == "None"
    assert (net.num_state, net.num_action, net.discrete_action, net.use_gru) == (22, 6, False, False)
    assert net.param_count() == co.param_count(22, 6, False) == 934 and co.param_count(22, 6, True) == 7270
    assert cfg["strategy"]["name"] == strategy and cfg["strategy"]["offspring_num"] == offspring
    base = yaml.load(open(os.path.join(SRC, "conf", "walker2d.yaml")), Loader=yaml.FullLoader)
    assert cfg["env"] == base["env"] and cfg["network"] == base["network"]
    hopper = yaml.load(open(os.path.join(SRC, "conf", conf.replace("walker2d", "hopper") + ".yaml")), Loader=yaml.FullLoader)
    assert cfg["strategy"] == hopper["strategy"]                         # the hopper's config with the env name and shape
