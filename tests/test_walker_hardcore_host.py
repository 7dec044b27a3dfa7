"""BipedalWalkerHardcore-v3 on the CPU: the host build of csrc/ses_walker_hardcore_env.h (tests/walker_hardcore_host.py).

The terrain generator and the terrain type over 2000 keys, the lidar against a closed form, and the physics on obstacle edges with
BipedalWalker-v3's own host build on grass (oracle/c_oracle.WalkerSim) as the yardstick; then the Python layer.

Penetration.  The world keeps polygons apart by their skins: POLY_RADIUS = 0.01 m on the polygon and on the edge, so two shapes
at rest have their cores about 0.02 - LINEAR_SLOP apart.  "Penetration" of a leg vertex is how far the two skins overlap:
2 * POLY_RADIUS minus the vertex's clearance over its supporting edge.  Figures of the drop from 0.3 m under zero action (float32
host build, the deepest of every leg vertex over the 80 steps that follow):
    BipedalWalker-v3, grass (start pad)      0.01306 m
    hardcore, flat span (start pad)          0.01320 m
    hardcore, stump top                      0.01320 m
    hardcore, stair tread (after the first)  0.01320 m
    hardcore, pit floor                      0.01181 m
The bound on every hardcore figure is 2 x the BipedalWalker-v3 figure (the margin allows for the different slot order), computed
by the test, not written down.  Driven against a stump's riser no leg vertex gets inside the stump at all (the deepest is 0.008 m
OUTSIDE its faces, i.e. a penetration of 0.012 by the same measure)."""
import os
import re

import numpy as np
import pytest

import walker_hardcore_host as hh
from oracle import c_oracle as co

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = hh.NAME
H, STEP = float(hh.TERRAIN_HEIGHT), float(hh.STEP)
SKIN = 2 * 0.01                                     # 2 * POLY_RADIUS (csrc/ses_b2.h)
N_KEYS = 2000


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def terrains():
    return [(key,) + hh.row_generate(key, key >> 3) for key in range(N_KEYS)]


def test_the_host_philox_is_the_oracles():
    """BipedalWalker-v3's terrain by this host build's Philox equals the oracle's, bit for bit"""
    for key in (0, 1, 0xDEADBEEF):
        sim = co.WalkerSim()
        sim.reset(hh.init_row(key))
        ty, _ = hh.walker_terrain(key, 0)
        dbg = sim.debug()
        want = dbg["terrain"] if isinstance(dbg, dict) else dbg[1]
        assert np.array_equal(bits(ty), bits(want))
        assert len(np.unique(ty[21:])) > 100


def test_terrains_of_2000_keys(terrains):
    kinds_seen = np.zeros(4, int)
    obstacle_starts = {hh.KIND_STUMP: 0, hh.KIND_PIT_FLOOR: 0, hh.KIND_TREAD: 0}
    tol = 4 * np.spacing(np.float32(8.0))           # heights stay below 8 m: y + k STEP and its difference round twice each
    for key, row, kind in terrains:
        yl, yr = row[:hh.COLS], row[hh.COLS:2 * hh.COLS]
        ty, _ = hh.walker_terrain(key, key >> 3)
        # columns 0 .. 19: the flat start pad, BipedalWalker-v3's heights bit for bit
        assert np.array_equal(bits(yl[:20]), bits(ty[:20])) and np.array_equal(bits(yr[:20]), bits(ty[1:21]))
        assert (yl[:20] == hh.TERRAIN_HEIGHT).all() and (kind[:20] == 0).all()
        # the first obstacle starts at column 20: a stump (riser at x_20), a pit (lip, then a riser at x_21) or stairs (first
        # tread level with the pad, a riser at x_24)
        if kind[20] == hh.KIND_STUMP:
            first = hh.KIND_STUMP
            assert yl[20] > yr[19]
        elif kind[21] == hh.KIND_PIT_FLOOR:
            first = hh.KIND_PIT_FLOOR
            assert yl[20] == yr[20] == yr[19] and yl[21] < yr[20]
        else:
            first = hh.KIND_TREAD
            assert (yl[20:24] == yr[19]).all() and (yr[20:24] == yr[19]).all() and kind[24] == hh.KIND_TREAD and yl[24] != yr[23]
        obstacle_starts[first] += 1
        kinds_seen += np.bincount(kind, minlength=4)
        # risers: whole multiples of STEP -- 1 or 2 at a stump, 4 at a pit, 1 at stairs
        for c in np.flatnonzero(yr[:-1] != yl[1:]) + 1:
            m = (float(yl[c]) - float(yr[c - 1])) / STEP
            assert abs(m - round(m)) * STEP <= tol, (key, c, m)
            k = int(round(m))
            around = {int(kind[c - 1]), int(kind[c])}
            if hh.KIND_STUMP in around:
                assert abs(k) in (1, 2), (key, c, k)
            elif hh.KIND_PIT_FLOOR in around:
                assert abs(k) == 4, (key, c, k)
            else:
                assert around <= {hh.KIND_GROUND, hh.KIND_TREAD} and abs(k) == 1, (key, c, k, around)
        # obstacle columns are flat
        assert (yl[kind != 0] == yr[kind != 0]).all()
        # the edge list: contiguous, x-monotone, no zero-length edge, spans one column long, risers vertical
        e = hh.row_edges(row)
        n_risers = int((yr[:-1] != yl[1:]).sum())
        assert len(e) == hh.COLS + n_risers
        assert np.array_equal(bits(e[1:, :2]), bits(e[:-1, 2:]))
        assert (e[:, 2] >= e[:, 0]).all()
        assert not ((e[:, 0] == e[:, 2]) & (e[:, 1] == e[:, 3])).any()
        riser = e[:, 0] == e[:, 2]
        assert riser.sum() == n_risers and (np.abs(e[riser, 3] - e[riser, 1]) > 0.9 * STEP).all()
        assert e[0, 0] == 0.0 and e[-1, 2] == np.float32(199) * hh.STEP
        # index_of: -1 left of column 0, n_edges right of the last column, the column's SPAN in between, monotone
        assert hh.row_index_of(row, -0.01) == -1 and hh.row_index_of(row, -1e6) == -1
        assert hh.row_index_of(row, 199 * STEP + 0.01) == len(e) and hh.row_index_of(row, 1e6) == len(e)
        if key % 50 == 0:
            xs = np.arange(-1.0, 199 * STEP + 1.0, 0.0371, dtype=np.float32)
            idx = np.array([hh.row_index_of(row, x) for x in xs])
            assert (np.diff(idx) >= 0).all()
            inside = (idx >= 0) & (idx < len(e))
            assert not riser[idx[inside]].any()
            assert (e[idx[inside], 0] <= xs[inside]).all() and (xs[inside] <= e[idx[inside], 2]).all()
    assert all(v > N_KEYS // 6 for v in obstacle_starts.values()), obstacle_starts       # all three kinds, about a third each
    assert (kinds_seen[1:] > 0).all()


def test_an_obstacle_free_row_is_walker_terrain_bit_for_bit():
    for key in (1, 2, 3):
        ty, want = hh.walker_terrain(key)
        row = hh.row_from_spans(ty[:-1], ty[1:])
        got = hh.row_edges(row)
        assert got.shape == want.shape == (199, 4) and np.array_equal(bits(got), bits(want))
        for x in np.arange(0.0, 199 * STEP, 0.0731, dtype=np.float32):
            assert hh.row_index_of(row, x) == hh.walker_index_of(ty, x)
        # outside, the callers clamp: -1 and n_edges clamp to what WalkerTerrain's unclamped column numbers clamp to
        for x in (-0.3, -5.0, 199 * STEP + 0.2, 120.0):
            assert min(max(hh.row_index_of(row, x), 0), 198) == min(max(hh.walker_index_of(ty, x), 0), 198)


def test_lidar_hits_a_riser_at_the_closed_form_fraction():
    """Ground at y = 1, a stump two columns wide and 1 m high on columns 30, 31: risers at x_30 (up) and x_32 (down).  A ray that
    meets a vertical edge at x_r: fraction = (x_r - p1x) / (p2x - p1x), the edge's unit normal being (+-1, 0) exactly.  In float32
    that is two subtractions and one division, each within half an ulp, (1 + 2^-24)^3: the bound is 4 * 2^-24 relative."""
    yl = np.ones(hh.COLS, np.float32)
    yl[30:32] = 2.0
    row = hh.row_from_spans(yl, yl)
    e = hh.row_edges(row)
    assert len(e) == 201
    x30, x32 = np.float32(30) * hh.STEP, np.float32(32) * hh.STEP
    rays = [((x30 - np.float32(1.5), 1.5), (x30 + np.float32(2.5), 1.5), x30),            # level, from the left
            ((x30 - np.float32(1.0), 2.2), (x30 + np.float32(1.0), 1.2), x30),            # descending, meets the riser at y = 1.7
            ((x32 + np.float32(1.0), 1.5), (x32 - np.float32(1.0), 1.5), x32),            # from the right: the edge is two-sided
            ((x30 - np.float32(0.7), 1.9), (x30 + np.float32(0.35), 1.1), x30)]
    for p1, p2, xr in rays:
        p1 = np.array(p1, np.float32)
        p2 = np.array(p2, np.float32)
        want = (float(xr) - float(p1[0])) / (float(p2[0]) - float(p1[0]))
        got = float(hh.row_raycast(row, p1, p2))
        assert 0.0 < want < 1.0 and abs(got - want) <= 4 * 2.0 ** -24 * want, (p1, p2, got, want)
    # a ray over the stump misses, one onto its top hits the top
    assert hh.row_raycast(row, (x30 - 1.0, 2.5), (x32 + 1.0, 2.5)) == 1.0
    got = float(hh.row_raycast(row, (float(x30) + 0.4, 3.0), (float(x30) + 0.4, 1.0)))
    assert abs(got - 0.5) <= 4 * 2.0 ** -24


# ---- physics ------------------------------------------------------------------------------------------------------------------------
def _penetration(verts, height):
    return SKIN - (float(verts[:, 1].min()) - height)


@pytest.fixture(scope="module")
def grass_figure():
    """the yardstick: BipedalWalker-v3 dropped from 0.3 m above its start pad, zero action, 80 steps"""
    sim = co.WalkerSim()
    sim.reset(hh.init_row(1))
    hh.shift_walker_sim(sim, 0.0, 0.3)
    worst, landed = -1.0, False
    for _ in range(80):
        _, _, done = sim.step(np.zeros(4, np.float32))
        dbg = sim.debug()
        bodies, ints = (dbg["bodies"], None) if isinstance(dbg, dict) else (dbg[0], dbg[2])
        worst = max(worst, _penetration(np.concatenate(hh.vertices(bodies)[1:]), H))
        if done:
            break
    assert 0.005 < worst < SKIN, worst                  # it landed (skins overlap) and no vertex went below the surface
    return worst


def _find_run(kind_wanted, min_cols):
    for key in range(1, 500):
        row, kind = hh.row_generate(key)
        idx = np.flatnonzero(kind == kind_wanted)
        if len(idx):
            c0 = c1 = int(idx[0])
            while c1 + 1 < hh.COLS and kind[c1 + 1] == kind_wanted and row[c1 + 1] == row[c0]:
                c1 += 1
            if c1 - c0 + 1 >= min_cols:
                return key, c0, c1, float(row[c0])
    raise AssertionError("no such obstacle in 500 keys")


DROPS = {"flat span": lambda: (1, 9, 10, H), "stump top": lambda: _find_run(hh.KIND_STUMP, 1), "stair tread": lambda: _find_run(hh.KIND_TREAD, 4),
         "pit floor": lambda: _find_run(hh.KIND_PIT_FLOOR, 2)}


@pytest.mark.parametrize("surface", list(DROPS))
def test_a_drop_onto_each_surface_penetrates_no_more_than_on_grass(grass_figure, surface):
    key, c0, c1, height = DROPS[surface]()
    sim = hh.HardcoreSim()
    sim.reset(hh.init_row(key))
    sim.shift(0.5 * (c0 + c1 + 1) * STEP - float(sim.debug()["bodies"][0, 0]), height - H + 0.3)
    worst, touched_wanted = -1.0, False
    for _ in range(80):
        _, _, done = sim.step(np.zeros(4, np.float32))
        v = sim.leg_vertices()
        over = v[(v[:, 0] >= c0 * STEP) & (v[:, 0] <= (c1 + 1) * STEP)]
        if len(over):
            worst = max(worst, _penetration(over, height))
        flags, _ = sim.manifolds()
        touched_wanted |= bool((flags == (0 if surface == "flat span" else 1)).any())
        if done:
            break
    print(f"{surface}: penetration {worst:.5f} m, BipedalWalker-v3 on grass {grass_figure:.5f} m, bound {2 * grass_figure:.5f} m")
    assert touched_wanted                               # the legs did land on that kind of edge
    assert 0.005 < worst <= 2 * grass_figure, (surface, worst, grass_figure)


STUMP_KEYS = (3, 4)                                     # the first obstacle of these keys is a stump one / two columns wide
DRIVES = ([1, 1, 1, 1], [1, 0, 1, 0], [1, -1, -1, 1], [-1, 1, 1, -1], [0.5, 1, 0.5, 1], [1, 1, 0, 0])


def _before_the_first_stump(key, gap):
    sim = hh.HardcoreSim()
    sim.reset(hh.init_row(key))
    row, kind = sim.terrain()
    width = int((kind[20:22] == hh.KIND_STUMP).sum())
    assert kind[20] == hh.KIND_STUMP and width == {3: 1, 4: 2}[key]
    sim.shift(20 * STEP - gap - float(sim.debug()["bodies"][0, 0]), 0.0)
    riser = hh.row_index_of(row, 20 * STEP + 0.01) - 1
    assert np.allclose(hh.row_edges(row)[riser], [20 * STEP, H, 20 * STEP, H + width * STEP])
    return sim, width, riser


def _hull_touching(sim):
    e = np.zeros(16, np.int32)
    return e[:hh.lib().bwh_hull_touching(sim._buf, hh._p(e))].tolist()


def test_a_leg_driven_against_a_stumps_riser_does_not_pass_it(grass_figure):
    worst, on_riser = -1.0, 0
    for key in STUMP_KEYS:
        for act in DRIVES:
            for gap in (0.35, 0.6):
                sim, width, riser = _before_the_first_stump(key, gap)
                x0, x1, top = 20 * STEP, (20 + width) * STEP, H + width * STEP
                for _ in range(120):
                    _, _, done = sim.step(np.array(act, np.float32))
                    v = sim.leg_vertices()
                    inside = np.minimum(np.minimum(v[:, 0] - x0, x1 - v[:, 0]), top - v[:, 1]).max()      # > 0: inside the stump
                    worst = max(worst, SKIN + float(inside))
                    flags, edges = sim.manifolds()
                    on_riser += int(((edges == riser) & (flags == 1)).any())
                    if done:
                        break
    print(f"deepest leg vertex against a stump: penetration {worst:.5f} m, bound {2 * grass_figure:.5f} m, {on_riser} steps with a leg on the riser")
    assert on_riser > 50
    assert worst <= 2 * grass_figure


def test_a_hull_that_touches_a_riser_ends_the_episode():
    """the walker falls against the stump: whenever the hull's polygon touches a terrain edge before a step, that step returns -100 and
    done; in the scenarios below the touched edges include the stump's riser"""
    hits = 0
    for key, act, gap in ((4, [1, 1, 0, 0], 0.35), (4, [-1, 1, 1, -1], 0.9), (3, [0.5, 1, 0.5, 1], 0.9), (4, [1, 1, 1, 1], 0.6)):
        sim, width, riser = _before_the_first_stump(key, gap)
        for t in range(150):
            touching = _hull_touching(sim)
            _, r, done = sim.step(np.array(act, np.float32))
            if touching:
                assert done and r == np.float32(-100.0) and sim.debug()["game_over"], (key, act, gap, t)
                assert riser in touching, (touching, riser)
                hits += 1
            if done:
                break
        assert done and t > 10
    assert hits == 4


def test_the_golden_walker_policies_reach_the_obstacles():
    """the inputs of the GPU rollout test: at least 30 of the 60 (policy, episode) pairs put a leg on an obstacle edge in 250 steps"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "g10_box2d_mlp.npz"))
    touched = np.zeros((20, 3), bool)
    hh.rollout(g["walker_theta"][12:32], g["walker_init"], 3, 250, touched=touched)
    print("pairs with a leg manifold on an obstacle edge:", int(touched.sum()), "of 60")
    assert touched.sum() >= 30


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def test_registry_wrapper_and_header():
    from envs.gym_wrapper import SUPPORTED, GymWrapper
    from ses import _lib
    from ses.envs import ENV_IDS, REGISTRY
    rec = REGISTRY[NAME]
    assert rec.env_id == _lib.ENV_BIPEDALWALKER_HARDCORE == ENV_IDS[NAME] == 16
    assert (rec.num_state, rec.num_action, rec.discrete, rec.time_limit) == (24, 4, False, 2000)
    assert rec.variant == "box2d-restated" and not rec.pomdp and not rec.obs_normalizer and rec.wrapper == "gym"
    assert NAME in SUPPORTED
    assert GymWrapper(NAME, None).horizon == 2000 and GymWrapper(NAME, "None").horizon == 2000 and GymWrapper(NAME, 300).horizon == 300
    assert GymWrapper(NAME, 5000).horizon == 2000 and GymWrapper(NAME, None).variant == "box2d-restated"
    with pytest.raises(AssertionError):
        GymWrapper(NAME, None, pomdp=True)
    text = open(os.path.join(ROOT, "include", "ses.h")).read()
    assert re.search(r"^#define SES_ENV_BIPEDALWALKER_HARDCORE 16\b", text, re.M)


def test_env_info_row():
    from ses import _lib
    walker = _lib.env_info(_lib.ENV_BIPEDALWALKER, 24, 4, False)
    for gru in (False, True):                           # (BipedalWalker-v3 refuses gru = 1)
        info = _lib.env_info(_lib.ENV_BIPEDALWALKER_HARDCORE, 24, 4, False, gru=gru)
        assert (info.init_width, info.obs_width, info.agents, info.num_action, info.has_ep_steps, info.is_f64) == (4, 24, 1, 4, 1, 0)
        assert (info.init_lo, info.init_hi, info.action_layout) == (0.0, 1.0, _lib.ACTION_F32_N_A)
        for field, _ in _lib.SesEnvInfo._fields_:
            if field != "state_bytes":
                assert getattr(info, field) == getattr(walker, field), field
        # the blob: the env struct with eight manifold slots per leg, then the terrain row
        assert info.state_bytes == hh.lib().bwh_blob_size() > walker.state_bytes + 4 * (hh.lib().bwh_row_floats() - 200)
    with pytest.raises(Exception, match="BipedalWalkerHardcore-v3"):
        _lib.env_info(_lib.ENV_BIPEDALWALKER_HARDCORE, 24, 4, False, pomdp=True)


def test_configs_build():
    import yaml
    import builder
    want = {"bipedalwalker_hardcore.yaml": "simple_genetic", "bipedalwalker_hardcore_sep_cma.yaml": "sep_cma_es", "bipedalwalker_hardcore_pgpe.yaml": "pgpe"}
    ref = yaml.safe_load(open(os.path.join(ROOT, "simple-es_amd", "conf", "bipedalwalker.yaml")))
    for name, strategy in want.items():
        cfg = yaml.safe_load(open(os.path.join(ROOT, "simple-es_amd", "conf", name)))
        assert cfg["env"]["name"] == NAME and cfg["strategy"]["name"] == strategy
        assert cfg["network"] == ref["network"] and {k: v for k, v in cfg["env"].items() if k != "name"} == {k: v for k, v in ref["env"].items() if k != "name"}
        assert builder.build_env(cfg["env"]).horizon == 300
        builder.build_strategy(cfg["strategy"])
    assert yaml.safe_load(open(os.path.join(ROOT, "simple-es_amd", "conf", "bipedalwalker_hardcore.yaml")))["strategy"] == ref["strategy"]
