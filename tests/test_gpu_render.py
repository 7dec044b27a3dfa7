"""The device renderer (csrc/ses_render.hip) against tests/render_np.py.

The rasteriser: device bytes equal rasterise() bytes, for crafted lists that sit on every rule of the primitive contract, at the
extreme sizes, and for seeded random lists.  The scenes: the device list has the restatement's count, the same kind and colour in
every slot and every coordinate within +-1 unit.  That bound is derived, not measured: coordinates stay below 2^14 units, the
float32 chain of a coordinate (a handful of operations on values below 2^14, each rounded once) is off by a few ulp of 2^14, i.e.
far below 1/256 of a unit, so float32 and float64 can only land on different integers where the value sits on a rounding
boundary, and then they differ by one.  Then the device frames must equal rasterise(device list) byte for byte.  On top: the
wrappers' render(), the refusals, and test.py --save-gif."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

import render_np as rn
from oracle import c_oracle as co
from render_np import CAPSULE, DISC, FILL, TRI

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def plain():
    """an env-less handle: the rasteriser knows no env"""
    from ses import HipES
    es = HipES(None, 4, 2, True, False)
    yield es
    es.close()


def device_frames(es, prims, counts, W, H):
    got = es.render_frames(dev(np.asarray(prims, np.int32)), dev(np.asarray(counts, np.int32)), W, H)
    return got.cpu().numpy()


# ---- the rasteriser -----------------------------------------------------------------------------------------------------------
def crafted_pool():
    """primitives that sit on the rules of the contract, for a 61 x 47 frame (976 x 752 units; samples at 16 p + 8)"""
    P = []
    P.append([TRI, 1, 40, 40, 600, 90, 300, 700])                     # one orientation ..
    P.append([TRI, 2, 40, 40, 300, 700, 600, 90])                     # .. and the other
    P.append([TRI, 3, 8, 8, 24, 24, 56, 56])                          # zero area, through pixel centres
    P.append([TRI, 4, 8, 8, 8 + 16 * 20, 8, 8, 8 + 16 * 20])           # legs and hypotenuse exactly on pixel centres
    P.append([TRI, 5, 968, 744, 968 - 160, 744, 968, 744 - 160])       # the same in the far corner (last column, last row)
    P.append([DISC, 6, 8 + 16 * 30, 8 + 16 * 20, 16 * 5, 0, 0, 0])     # rim exactly on pixel centres
    P.append([DISC, 7, 500, 300, -1, 0, 0, 0])                         # negative radius: never
    P.append([DISC, 8, 8 + 16 * 10, 8 + 16 * 40, 0, 0, 0, 0])          # radius 0 on a pixel centre: that pixel
    P.append([DISC, 9, 9 + 16 * 12, 8 + 16 * 40, 0, 0, 0, 0])          # radius 0 off centre: none
    P.append([CAPSULE, 10, 100, 600, 800, 200, 24, 0])
    P.append([CAPSULE, 11, 200, 100, 200, 100, 40, 0])                 # a == b: a disc
    P.append([CAPSULE, 12, 8, 8 + 16 * 25, 8 + 16 * 50, 8 + 16 * 25, 16, 0])   # axis and rim on pixel centres
    P.append([CAPSULE, 13, 300, 300, 500, 500, -5, 0])                 # negative radius: never
    P.append([7, 14, 0, 0, 900, 0, 0, 700])                            # kind 7: skipped
    P.append([-1, 14, 0, 0, 900, 0, 0, 700])
    P.append([TRI, 0x1F, 700, 500, 900, 520, 760, 700])                # colour 0x1F is used as 15
    P.append([FILL, 0x13, 1, 2, 3, 4, 5, 6])                           # a FILL in the middle of a list (colour 3)
    P.append([DISC, 1, -40, 300, 100, 0, 0, 0])                        # partly outside: left, right, top, bottom
    P.append([DISC, 2, 1000, 300, 100, 0, 0, 0])
    P.append([CAPSULE, 3, 400, -60, 600, -20, 70, 0])
    P.append([TRI, 4, 300, 700, 500, 900, 100, 900])
    P.append([DISC, 5, -400, 300, 100, 0, 0, 0])                       # wholly outside: left, right, top, bottom
    P.append([DISC, 6, 1400, 300, 100, 0, 0, 0])
    P.append([CAPSULE, 7, 100, -300, 800, -300, 50, 0])
    P.append([TRI, 8, 100, 800, 800, 800, 400, 1200])
    P.append([TRI, 9, -16384, -16384, 16383, -16384, 0, 16383])        # the ends of the coordinate range
    P.append([TRI, 10, -16384, 16383, 16383, 16383, 600, -16384])
    P.append([CAPSULE, 11, -16384, -16384, 16383, 16383, 40, 0])
    P.append([CAPSULE, 12, 16383, -16384, -16384, 16383, 16383, 0])
    P.append([DISC, 13, -16000, 300, 16383, 0, 0, 0])
    P.append([DISC, 14, 16383, 16383, 16383, 0, 0, 0])
    P.append([DISC, 2, 488, 376, 60, 0, 0, 0])
    return np.array(P, dtype=np.int32)


def crafted_lists(n=37, cap=256):
    pool = crafted_pool()
    m = len(pool)
    rng = np.random.RandomState(7)
    prims = np.zeros((n, cap, 8), np.int32)
    counts = np.zeros(n, np.int32)
    for f in range(n):
        order = np.arange(cap) % m if f % 3 == 0 else rng.randint(0, m, size=cap)
        prims[f] = pool[np.roll(order, f)]
        counts[f] = rng.randint(0, cap + 1)
    counts[0], counts[1], counts[2] = 0, 1, cap
    for f in range(3, 3 + m):                                         # every pool entry is the LAST (visible) one of some list
        prims[f, 5] = pool[f - 3]
        counts[f] = 6
    counts[n - 1] = cap + 44                                          # above cap: read as cap
    return prims, counts


def test_crafted_lists_at_an_odd_size(plain):
    prims, counts = crafted_lists()
    assert len(crafted_pool()) + 3 <= 37 and {0, 1, 256} <= set(counts.tolist())
    want = rn.rasterise(prims, counts, 61, 47)
    got = device_frames(plain, prims, counts, 61, 47)
    assert got.shape == (37, 47, 61) and got.dtype == np.uint8
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    # every colour is on some pixel but 7 and 14: the negative radii, the unknown kinds and what lies wholly outside carry those
    assert set(np.unique(want).tolist()) == set(range(16)) - {7, 14}


def test_extreme_sizes(plain):
    few = np.array([[FILL, 9, 0, 0, 0, 0, 0, 0], [TRI, 1, 100, 100, 16000, 300, 400, 16383], [TRI, 2, 9000, 9000, 9000, 9000, 9100, 9100],
                    [DISC, 3, 8200, 8200, 5000, 0, 0, 0], [CAPSULE, 4, -16384, 16383, 16383, -16384, 333, 0], [5, 5, 0, 0, 9999, 0, 0, 9999],
                    [DISC, 6, 16376, 16376, 0, 0, 0, 0], [CAPSULE, 7, 8, 8, 8, 16376, 0, 0]], np.int32)[None]
    want = rn.rasterise(few, [8], 1024, 1024)
    got = device_frames(plain, few, [8], 1024, 1024)
    assert np.array_equal(got, want)
    assert got[0, 1023, 1023] == 6 and (got[0, :, 0] == 7).all() and {9, 1, 3, 4} <= set(np.unique(got).tolist())
    # one pixel: its sample is (8, 8)
    for prim, colour in (([DISC, 5, 8, 8, 0, 0, 0, 0], 5), ([DISC, 5, 9, 8, 0, 0, 0, 0], 0), ([TRI, 6, 8, 8, 100, 8, 8, 100], 6),
                         ([FILL, 7, 0, 0, 0, 0, 0, 0], 7)):
        one = np.array([[prim]], np.int32)
        got = device_frames(plain, one, [1], 1, 1)
        assert got.shape == (1, 1, 1) and got[0, 0, 0] == colour == rn.rasterise(one, [1], 1, 1)[0, 0, 0]
    # cap = 1, several frames, a width that ends in a partial store
    ones = np.array([[[DISC, 3, 100, 100, 90, 0, 0, 0]], [[FILL, 4, 0, 0, 0, 0, 0, 0]], [[CAPSULE, 5, 0, 0, 300, 200, 20, 0]]], np.int32)
    counts = [1, 5, 0]
    assert np.array_equal(device_frames(plain, ones, counts, 19, 13), rn.rasterise(ones, counts, 19, 13))


def test_random_lists(plain):
    rng = np.random.RandomState(2024)
    n, cap, W, H = 16, 256, 64, 48
    prims = rng.randint(-300, 1400, size=(n, cap, 8)).astype(np.int32)
    prims[..., 0] = rng.choice([TRI, TRI, DISC, CAPSULE, CAPSULE, FILL, 4], size=(n, cap), p=[0.3, 0.2, 0.2, 0.15, 0.1, 0.02, 0.03])
    prims[..., 1] = rng.randint(0, 32, size=(n, cap))
    disc, caps = prims[..., 0] == DISC, prims[..., 0] == CAPSULE
    prims[..., 4][disc] = rng.randint(-10, 160, size=int(disc.sum()))
    prims[..., 6][caps] = rng.randint(-10, 90, size=int(caps.sum()))
    counts = rng.randint(0, cap + 1, size=n).astype(np.int32)
    want = rn.rasterise(prims, counts, W, H)
    got = device_frames(plain, prims, counts, W, H)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:5])


def test_bad_arguments_are_refused_with_a_message(plain):
    from ses import _lib
    lib = _lib.load()
    prims = torch.zeros(1, 256, 8, dtype=torch.int32, device="cuda")
    counts = torch.zeros(1, dtype=torch.int32, device="cuda")
    frames = torch.zeros(1, 1024, 1024, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())                       # noqa: E731
    for cap, W, H, word in ((256, 0, 16, "width"), (256, 16, 1025, "height"), (257, 16, 16, "cap")):
        rc = lib.ses_render_frames(plain._h, p(prims), p(counts), 1, cap, W, H, p(frames))
        assert rc < 0 and word in lib.ses_last_error().decode(), (cap, W, H, rc, lib.ses_last_error())
    assert lib.ses_render_frames(plain._h, None, p(counts), 1, 256, 16, 16, p(frames)) < 0 and b"null" in lib.ses_last_error()
    assert lib.ses_render_frames(plain._h, p(prims), p(counts), 1, 256, 16, 16, p(frames)) == 0
    from ses import SesError
    with pytest.raises(SesError, match="1024"):
        plain.render_frames(prims, counts, 16, 1025)


# ---- the scenes ---------------------------------------------------------------------------------------------------------------
def check_scene(es, state, want, W, H):
    """device lists of the state blobs against the restatements `want` = [(prims, count), ...]; -> the device frames"""
    assert es.render_size() == (W, H)
    prims, counts = es.render_scene(state)
    frames = es.render_frames(prims, counts, W, H)
    prims, counts, frames = prims.cpu().numpy(), counts.cpu().numpy(), frames.cpu().numpy()
    for i, (wp, wn) in enumerate(want):
        assert counts[i] == wn, (i, counts[i], wn)
        assert np.array_equal(prims[i, :wn, :2], wp[:wn, :2]), (i, prims[i, :wn, :2].tolist(), wp[:wn, :2].tolist())
        diff = np.abs(prims[i, :wn, 2:].astype(np.int64) - wp[:wn, 2:])
        assert diff.max() <= 1, (i, np.argwhere(diff > 1)[:4], prims[i, :wn][diff.max(1) > 1][:2], wp[:wn][diff.max(1) > 1][:2])
    assert np.array_equal(frames, rn.rasterise(prims, counts, W, H))
    assert np.array_equal(es.render(state).cpu().numpy(), frames)      # the two launches behind one call
    return frames


def test_cartpole_scene():
    from ses import HipES
    es = HipES("CartPole-v1", 4, 2, True, False)
    cases = [(0.0, 0.0), (2.4, 0.2095), (2.4, -0.2095), (-2.4, 0.2095), (-2.4, -0.2095), (1.0, 0.75), (5.0, 0.0), (1.0, -0.75)]
    blobs = np.array([[x, 0.3, th, -0.2] for x, th in cases], np.float32)
    state = dev(blobs.view(np.uint8).reshape(len(cases), 16))
    assert es.env_state_bytes() == 16
    want = [rn.scene_cartpole(b) for b in blobs]
    frames = check_scene(es, state, want, 600, 400)
    assert want[6][1] == 2 and want[0][1] == 6                        # a cart off the canvas leaves the FILL and the track
    # semantics, independent of both implementations: the pivot is 107.5 px above the bottom edge, at x_px = 300 + 125 x
    assert frames[0][400 - 158, 300] == rn.POLE                       # 50 px above the pivot, upright
    assert frames[0][400 - 100, 300] == rn.BLACK and frames[0][400 - 100, 5] == rn.BLACK and frames[0][10, 10] == rn.WHITE
    for k, side in ((5, 1), (7, -1)):                                 # theta = +0.75 leans right of the cart centre, -0.75 left
        cols = np.nonzero(frames[k] == rn.POLE)[1]
        assert len(cols) > 500 and side * (cols.mean() - (300 + 125 * 1.0)) > 20, (k, cols.mean())
    es.close()


@pytest.mark.parametrize("na", [2, 3])
def test_spread_scene(na):
    from ses import HipES
    es = HipES("simple_spread", 6 * na, 5, True, False, max_step=25, eval_ep_num=1, n_agents=na)
    lm = np.array([[-1.0, 0.5], [0.7, -1.2], [1.5, 1.9]], np.float32)[:na]

    def blob(agents):
        a = np.asarray(agents, np.float32)
        st = np.concatenate([a[:, 0], a[:, 1], np.full(2 * na, 0.25, np.float32), lm[:, 0], lm[:, 1]]).astype(np.float32)
        return np.concatenate([st.view(np.uint8), np.array([3], np.int32).view(np.uint8)])

    cases = [lm.copy(),                                               # agents on landmarks
             np.concatenate([[[2.5, 0.0]], lm[1:]]),                  # one agent outside the square on the right: dropped
             np.concatenate([[[-2.5, 0.0]], lm[1:]]),                 # .. on the left
             np.tile([[0.1, 0.1]], (na, 1)) + np.arange(na)[:, None] * 0.05,   # overlapping agents
             np.concatenate([[[2.1, -2.1]], lm[1:]])]                 # partly outside: kept
    state = dev(np.stack([blob(c) for c in cases]))
    assert state.shape[1] == es.env_state_bytes() == 4 * (6 * na + 1)
    want = [rn.scene_spread(np.frombuffer(bytes(s), np.float32, count=6 * na), na) for s in state.cpu().numpy()]
    frames = check_scene(es, state, want, 400, 400)
    assert [w[1] for w in want] == [1 + 2 * na, 2 * na, 2 * na, 1 + 2 * na, 1 + 2 * na]
    assert frames[0][200 - 50, 200 - 100] == rn.AGENT and frames[0][0, 0] == rn.WHITE      # the agent on the landmark at (-1, 0.5) hides it
    assert frames[1][200 + 120, 200 + 70] == rn.AGENT and (frames[1][:, 395:] != rn.AGENT).all()
    es.close()


LANDER_ACTION_TABLE = np.array([[0.0, 0.0], [0.0, -1.0], [1.0, 0.0], [0.0, 1.0]], np.float32)   # gym's discrete lander


@pytest.mark.parametrize("name", ["LunarLanderContinuous-v2", "LunarLander-v2"])
def test_lander_scene(name):
    from ses import HipES
    discrete = name == "LunarLander-v2"
    n = 4
    es = HipES(name, 8, 4, discrete, False, max_step=300, eval_ep_num=1)
    init = es.init_states_uniform(21, 3, 0, n)[:, 0].contiguous()
    state, _ = es.env_reset(init)
    sims = [co.LanderSim() for _ in range(n)]
    for s, u in zip(sims, init.cpu().numpy()):
        s.reset(u)
    rng = np.random.RandomState(5)
    snapshots, states, t = [], [], 0
    for until in (0, 1, 5, 40):
        while t < until:
            if discrete:
                a = rng.randint(0, 4, size=n).astype(np.int32)
                pairs = LANDER_ACTION_TABLE[a]
                es.env_step_generic(state, dev(a))
            else:
                act = np.tanh(rng.randn(n, 4)).astype(np.float32)
                pairs = act[:, :2]
                es.env_step_generic(state, dev(act))
            for s, (a0, a1) in zip(sims, pairs):
                s.step(float(a0), float(a1))
            t += 1
        states.append(state.clone())
        for s in sims:
            bodies, _ = s.debug()
            terrain = np.frombuffer(s._buf, np.float32)[-11:]          # LanderSim keeps the episode's heights behind the env
            snapshots.append(rn.scene_lander(bodies.astype(np.float64), terrain.astype(np.float64)))
    frames = check_scene(es, torch.cat(states), snapshots, 600, 400)
    # FILL, 20 terrain and 4 flag primitives always; up to 4 + 4 of the lander, which starts at the canvas's upper edge (what
    # pokes out above it is dropped)
    assert all(1 + 20 + 4 < w[1] <= 1 + 20 + 4 + 4 + 4 for w in snapshots), [w[1] for w in snapshots]
    assert (frames[:, 399, :] == rn.WHITE).all() and (frames[:, 0, 0] == rn.BLACK).all()     # the moon below, the sky above
    assert all((f == rn.YELLOW).sum() > 20 for f in frames)                                  # the two helipad flags
    # after reset the lander hangs at the canvas's upper edge, the lower half of the hull and the legs in view (later the engines
    # may have lifted it out of the picture)
    assert all((f == rn.HULL).sum() > 200 and (f == rn.LANDER_LEG).sum() > 50 for f in frames[:n])
    es.close()


def test_walker_scene():
    from ses import HipES
    n = 4
    es = HipES("BipedalWalker-v3", 24, 4, False, False, max_step=300, eval_ep_num=1)
    init = es.init_states_uniform(8, 1, 0, n)[:, 0].contiguous()
    state, _ = es.env_reset(init)
    sims = [co.WalkerSim() for _ in range(n)]
    obs = [s.reset(u) for s, u in zip(sims, init.cpu().numpy())]
    centres = co.walker_body_props()[:, 2:4].astype(np.float64)
    rng = np.random.RandomState(9)
    snapshots, scrolls, hulls, states, t = [], [], [], [], 0
    for until in (0, 1, 10, 60):
        while t < until:
            act = np.tanh(rng.randn(n, 4)).astype(np.float32)
            es.env_step_generic(state, dev(act))
            obs = [s.step(a)[0] for s, a in zip(sims, act)]
            t += 1
        states.append(state.clone())
        for s, o in zip(sims, obs):
            bodies, terrain, _ = s.debug()
            scene, scroll = rn.scene_walker(bodies.astype(np.float64), terrain.astype(np.float64), o[14:24].astype(np.float64), centres)
            snapshots.append(scene)
            scrolls.append(scroll)
            hulls.append(rn._origin(bodies[0].astype(np.float64), centres[0])[:2])
    frames = check_scene(es, torch.cat(states), snapshots, 600, 400)
    assert all(90 <= w[1] <= 140 for w in snapshots), [w[1] for w in snapshots]
    scrolls = np.array(scrolls).reshape(4, n)
    assert (np.abs(scrolls[3] - scrolls[0]) > 0.05).all()             # the view scrolls with the hull ..
    assert (scrolls[:3] > 0.5).all()                                  # (after reset, 1 and 10 steps the terrain's start is left of it)
    for f, (hx, hy), scroll in zip(frames, hulls, scrolls.reshape(-1)):
        assert abs(30.0 * (hx - scroll) - 120.0) < 1e-9               # .. which stays a fifth of the canvas from the left edge
        assert f[int(400 - 30.0 * hy), 120] == rn.HULL                # the hull's centre pixel
        # Column 0 at the bottom row has the terrain colour -- while the terrain is under it: the terrain starts at world x = 0 and
        # the view at x = scroll = hull x - 4, so a walker that has stumbled BACK past x = 4 (one of the four does within 60 random
        # steps: tests/ replay on the host oracle, hull x = 3.89) has sky there, as gym's own view would.  Column 0 is sampled at
        # 8 units, the first edge starts at -480 scroll units; two units of margin for the roundings.
        first_edge = -480.0 * scroll
        assert abs(first_edge - 8.0) > 2.0
        assert f[399, 0] == (rn.GRASS if first_edge < 8.0 else rn.SKY) and f[0, 0] == rn.SKY
        assert f[399, 300] == rn.GRASS
        assert (f == rn.RED).sum() > 100 and (f == rn.LEG_NEAR).sum() + (f == rn.LEG_FAR).sum() > 300 and (f == rn.LEG_FAR).sum() > 100
    es.close()


# ---- the host layers ----------------------------------------------------------------------------------------------------------
def test_palette_constant_equals_the_librarys():
    from ses import _lib
    from ses.render import palette
    buf = (ctypes.c_uint8 * 48)()
    assert _lib.load().ses_render_palette(buf) == 0
    assert np.array_equal(np.frombuffer(buf, np.uint8).reshape(16, 3), palette())


@pytest.mark.parametrize("family", ["CartPole-v1", "LunarLanderContinuous-v2", "BipedalWalker-v3", "simple_spread"])
def test_wrapper_render_is_the_device_frame_in_rgb(family):
    from envs.gym_wrapper import GymWrapper
    from envs.pettingzoo_wrapper import PettingzooWrapper
    from ses.render import palette
    env = PettingzooWrapper("simple_spread") if family == "simple_spread" else GymWrapper(family)
    with pytest.raises(RuntimeError) as e:
        env.render()
    assert not isinstance(e.value, NotImplementedError) and "reset" in str(e.value)
    with pytest.raises(RuntimeError):
        env.state_blob()
    env.reset()
    rgb = env.render()
    W, H = env._device().render_size()
    assert rgb.shape == (H, W, 3) and rgb.dtype == np.uint8
    blob = env.state_blob()
    assert blob.data_ptr() != env._state.data_ptr() and torch.equal(blob, env._state)
    assert np.array_equal(rgb, palette()[env._device().render(blob)[0].cpu().numpy()])
    assert len(np.unique(rgb.reshape(-1, 3), axis=0)) >= 3


def test_envs_without_a_scene_say_which_have_one():
    from envs.gym_wrapper import GymWrapper
    from envs.pettingzoo_wrapper import PettingzooWrapper
    from ses import _lib
    for env in (GymWrapper("Pendulum-v1"), PettingzooWrapper("pursuit")):
        with pytest.raises(NotImplementedError) as e:
            env.render()
        for word in ("CartPole", "LunarLander", "BipedalWalker", "simple_spread"):
            assert word in str(e.value), str(e.value)
    pend = GymWrapper("Pendulum-v1")
    pend.reset()
    es = pend._device()
    lib = _lib.load()
    prims = torch.zeros(1, 256, 8, dtype=torch.int32, device="cuda")
    counts = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = lib.ses_render_scene(es._h, ctypes.c_void_p(pend._state.data_ptr()), 1, ctypes.c_void_p(prims.data_ptr()),
                              ctypes.c_void_p(counts.data_ptr()))
    assert rc == _lib.SES_ERR_UNSUPPORTED == -2 and b"BipedalWalker" in lib.ses_last_error()
    w, h = ctypes.c_int32(), ctypes.c_int32()
    assert lib.ses_render_size(es._h, ctypes.byref(w), ctypes.byref(h)) == -2
    with pytest.raises(NotImplementedError):
        es.render(pend._state)


def _playback_cli():
    spec = importlib.util.spec_from_file_location("ses_playback_cli", os.path.join(SRC, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_save_gif_writes_one_file_per_episode(tmp_path, monkeypatch, capsys):
    Image = pytest.importorskip("PIL.Image")
    import yaml
    import builder
    from ses import HipES
    cfg_path = os.path.join(SRC, "conf", "cartpole.yaml")
    with open(cfg_path) as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    network = builder.build_network(config["network"])
    network.zero_init()
    monkeypatch.chdir(tmp_path)
    os.makedirs("logs/run7/saved_models")
    torch.save(network.state_dict(), "logs/run7/saved_models/ep_0.pt")
    cli = _playback_cli()
    argv = ["test.py", "--cfg-path", cfg_path, "--ckpt-path", "logs/run7/saved_models/ep_0.pt", "--episodes", "2"]

    monkeypatch.setattr(sys, "argv", argv + ["--save-gif"])
    cli.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("reward:")]
    assert len(lines) == 2
    assert sorted(os.listdir("test_gif/run7")) == ["ep_0.gif", "ep_1.gif"]
    for i, ln in enumerate(lines):
        ep_step = int(ln.split("ep_step:")[1])
        assert 5 <= ep_step <= 20 and float(ln.split()[1]) == ep_step          # the zero policy pushes one way until the pole falls
        with Image.open(f"test_gif/run7/ep_{i}.gif") as im:
            assert im.n_frames == ep_step and im.size == (600, 400)
            im.seek(ep_step - 1)
            last = np.asarray(im.convert("RGB"))
        assert (last == (204, 153, 102)).all(-1).sum() > 500                     # a pole is in the picture

    # without the flag: what it has always printed -- the episodes as ONE launch of the fused rollout
    monkeypatch.setattr(sys, "argv", argv)
    cli.main()
    out = capsys.readouterr().out.splitlines()
    es = HipES("CartPole-v1", 4, 2, True, False, pomdp=False, max_step=500, eval_ep_num=2)
    theta = torch.from_numpy(network.flat()[None, :]).to(es.device)
    fit, ep_ret, ep_steps = es.rollout(theta, es.init_states_uniform(0, 0, 0, 1), want_episodes=True)
    want = [f"reward:  {r} ep_step:  {s}" for r, s in zip(ep_ret[0].cpu().tolist(), ep_steps[0].cpu().tolist())]
    want.append(f"mean reward over 2 episodes: {float(fit[0]):.3f}")
    assert out == want
    assert sorted(os.listdir("test_gif/run7")) == ["ep_0.gif", "ep_1.gif"]
    es.close()
