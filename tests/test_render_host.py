"""CPU side of the renderer: the numpy restatement of the primitive contract (tests/render_np.py) against hand-written tiny
frames, and ses.render (palette, write_gif), which needs no device.  The device rasteriser and the scenes are held to
render_np in tests/test_gpu_render.py."""
import numpy as np
import pytest

import render_np as rn
from render_np import CAPSULE, DISC, FILL, TRI


def one(prims, W, H, **kw):
    """a single frame from a python list of 8-int primitives"""
    arr = np.array(prims, dtype=np.int64).reshape(1, -1, 8)
    return rn.rasterise(arr, [arr.shape[1]], W, H, **kw)[0]


def test_triangle_edges_through_pixel_centres_are_inclusive():
    # samples are at 8, 24, 40, 56; the hypotenuse x + y = 64 passes through (8, 56), (24, 40), (40, 24), (56, 8)
    for tri in ([TRI, 5, 8, 8, 56, 8, 8, 56], [TRI, 5, 8, 8, 8, 56, 56, 8]):      # both orientations draw the same
        got = one([tri], 4, 4)
        want = np.array([[5, 5, 5, 5],
                         [5, 5, 5, 0],
                         [5, 5, 0, 0],
                         [5, 0, 0, 0]], dtype=np.uint8)
        assert np.array_equal(got, want), got
    # moved by one unit the diagonal samples fall outside
    got = one([[TRI, 5, 8, 8, 55, 8, 8, 55]], 4, 4)
    assert np.array_equal(got, np.array([[5, 5, 5, 0], [5, 5, 0, 0], [5, 0, 0, 0], [0, 0, 0, 0]], dtype=np.uint8)), got


def test_disc_of_radius_zero_covers_its_own_sample_only():
    got = one([[DISC, 3, 24, 40, 0, 0, 0, 0]], 4, 4)
    want = np.zeros((4, 4), np.uint8)
    want[2, 1] = 3
    assert np.array_equal(got, want)
    assert not one([[DISC, 3, 25, 40, 0, 0, 0, 0]], 4, 4).any()                    # off-centre: none
    assert not one([[DISC, 3, 24, 40, -1, 0, 0, 0]], 4, 4).any()                   # a negative radius never draws
    # radius 16 reaches the four neighbours exactly (rim on pixel centres), not the diagonals
    got = one([[DISC, 3, 24, 24, 16, 0, 0, 0]], 4, 4)
    assert got.sum() == 5 * 3 and got[1, 1] == got[0, 1] == got[2, 1] == got[1, 0] == got[1, 2] == 3


def test_capsule_with_equal_ends_is_a_disc():
    for r in (0, 16, 23, 40):
        a = one([[CAPSULE, 2, 24, 40, 24, 40, r, 0]], 5, 5)
        b = one([[DISC, 2, 24, 40, r, 0, 0, 0]], 5, 5)
        assert np.array_equal(a, b)
    # and a proper capsule: the segment (8, 24) - (56, 24) with radius 0 covers exactly the row it runs through
    got = one([[CAPSULE, 2, 8, 24, 56, 24, 0, 0]], 5, 5)
    want = np.zeros((5, 5), np.uint8)
    want[1, 0:4] = 2
    assert np.array_equal(got, want), got


def test_zero_area_triangle_draws_nothing():
    assert not one([[TRI, 7, 8, 8, 24, 24, 56, 56]], 4, 4).any()                    # collinear, through four pixel centres
    assert not one([[TRI, 7, 24, 24, 24, 24, 24, 24]], 4, 4).any()                  # a point


def test_painters_order_and_fill_and_unknown_kinds():
    prims = [[DISC, 1, 24, 24, 16, 0, 0, 0], [FILL, 0x1F, 0, 0, 0, 0, 0, 0], [DISC, 2, 24, 24, 0, 0, 0, 0], [7, 9, 0, 0, 999, 999, 999, 0]]
    got = one(prims, 3, 3)
    want = np.full((3, 3), 15, np.uint8)                                            # colour 0x1F is used as 15; kind 7 is skipped
    want[1, 1] = 2
    assert np.array_equal(got, want)
    arr = np.array(prims, dtype=np.int64).reshape(1, -1, 8)
    assert np.array_equal(rn.rasterise(arr, [1], 3, 3)[0], one(prims[:1], 3, 3))    # the count cuts the list
    assert np.array_equal(rn.rasterise(arr, [99], 3, 3)[0], want)                   # above cap: read as cap


def test_windowed_evaluation_equals_the_full_one():
    rng = np.random.RandomState(0)
    prims = rng.randint(-200, 1200, size=(6, 40, 8))
    prims[..., 0] = rng.randint(0, 5, size=(6, 40))
    prims[..., 1] = rng.randint(0, 32, size=(6, 40))
    prims[:, ::7, 4] = rng.randint(-5, 300, size=prims[:, ::7, 4].shape)            # some small radii, some negative
    prims[:, ::5, 6] = rng.randint(-5, 200, size=prims[:, ::5, 6].shape)
    counts = [40, 0, 13, 40, 27, 1]
    assert np.array_equal(rn.rasterise(prims, counts, 61, 47), rn.rasterise(prims, counts, 61, 47, windowed=False))


def test_palette_has_sixteen_distinct_colours():
    from ses.render import palette, to_rgb
    pal = palette()
    assert pal.shape == (16, 3) and pal.dtype == np.uint8
    assert len({tuple(row) for row in pal.tolist()}) == 16
    idx = np.arange(16, dtype=np.uint8).reshape(4, 4)
    assert np.array_equal(to_rgb(idx), pal[idx]) and to_rgb(idx).shape == (4, 4, 3)


def test_write_gif_round_trip(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from ses.render import palette, write_gif
    rng = np.random.RandomState(1)
    frames = rng.randint(0, 16, size=(3, 6, 8)).astype(np.uint8)
    frames[1] = frames[0]                                                          # a frame equal to its predecessor stays a frame
    path = tmp_path / "a.gif"
    write_gif(str(path), frames, fps=30)
    with Image.open(str(path)) as im:
        assert im.n_frames == 3 and im.size == (8, 6)
        for k in range(3):
            im.seek(k)
            assert np.array_equal(np.asarray(im.convert("RGB")), palette()[frames[k]]), k


def test_scene_restatements_follow_the_drop_and_clamp_rule():
    prims, n = rn.scene_cartpole(np.array([5.0, 0, 0, 0], np.float32))              # cart off the canvas: FILL and the track remain
    assert n == 2 and prims[0, 0] == FILL and prims[1, 0] == CAPSULE
    prims, n = rn.scene_cartpole(np.array([0.0, 0, 0, 0], np.float32))
    assert n == 6 and [int(k) for k in prims[:6, 0]] == [FILL, CAPSULE, TRI, TRI, CAPSULE, DISC]
    assert tuple(prims[4, 2:7]) == (4800, 6400 - 1720, 4800, 6400 - 1720 - 1920, 80)   # the pole stands upright on the pivot
    blob = np.zeros(12, np.float32)
    blob[0] = 2.5                                                                  # one agent outside the square
    prims, n = rn.scene_spread(blob, 2)
    assert n == 1 + 2 + 1
