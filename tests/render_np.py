"""The renderer restated in numpy (TEST INFRASTRUCTURE; imports no product code).

rasterise(): the primitive contract of include/ses.h / DESIGN.md section 19 in int64 -- what the device rasteriser must equal
byte for byte.  scene_*(): the four scenes in float64, from sources of the state that do not pass through the device scene
builders: the documented float32 blobs (CartPole: x, x', theta, theta'; simple_spread: agent x[NA], y[NA], velocities, landmark
x[NA], y[NA]) and, for the Box2D envs, what the host oracle's LanderSim / WalkerSim report (body poses, terrain, lidar fractions)
with the polygon vertices written out from gym's definitions.  The device works in float32 with one rounding per operation and
rounds to the nearest unit, so a coordinate may differ from these by one unit where a value sits on a rounding boundary.
"""
import numpy as np

TRI, DISC, CAPSULE, FILL = 0, 1, 2, 3
MAX_PRIMS = 256
COORD_MIN, COORD_MAX = -16384, 16383

# palette indices (csrc/ses_render.h)
BLACK, WHITE, SKY, GRASS, RED, YELLOW, HULL, LANDER_LEG, POLE, AXLE, LEG_NEAR, LEG_FAR, LANDMARK, AGENT, GREY, FLAG = range(16)


# ---- the rasteriser ---------------------------------------------------------------------------------------------------------
def _cross(ux, uy, vx, vy):
    return ux * vy - uy * vx


def covered(prim, X, Y):
    """bool array like X, Y (int64 sample coordinates): the samples primitive `prim` (8 ints) covers"""
    kind, _, x0, y0, x1, y1, x2, y2 = (int(v) for v in prim)
    if kind == TRI:
        area = _cross(x1 - x0, y1 - y0, x2 - x0, y2 - y0)
        if area == 0:
            return np.zeros(X.shape, bool)
        s = 1 if area > 0 else -1
        return ((s * _cross(x1 - x0, y1 - y0, X - x0, Y - y0) >= 0) & (s * _cross(x2 - x1, y2 - y1, X - x1, Y - y1) >= 0) &
                (s * _cross(x0 - x2, y0 - y2, X - x2, Y - y2) >= 0))
    if kind == DISC:
        r = x1
        if r < 0:
            return np.zeros(X.shape, bool)
        return (X - x0) ** 2 + (Y - y0) ** 2 <= r * r
    if kind == CAPSULE:
        r = x2
        if r < 0:
            return np.zeros(X.shape, bool)
        dx, dy = x1 - x0, y1 - y0
        l2 = dx * dx + dy * dy
        t = dx * (X - x0) + dy * (Y - y0)
        at_a = (X - x0) ** 2 + (Y - y0) ** 2 <= r * r
        at_b = (X - x1) ** 2 + (Y - y1) ** 2 <= r * r
        between = _cross(dx, dy, X - x0, Y - y0) ** 2 <= r * r * l2
        return np.where(t <= 0, at_a, np.where(t >= l2, at_b, between))
    if kind == FILL:
        return np.ones(X.shape, bool)
    return np.zeros(X.shape, bool)


def _window(prim, W, H):
    """pixel rows / columns outside which `prim` covers nothing (its bounding box; every predicate implies it)"""
    kind, _, x0, y0, x1, y1, x2, y2 = (int(v) for v in prim)
    if kind == TRI:
        lox, hix, loy, hiy = min(x0, x1, x2), max(x0, x1, x2), min(y0, y1, y2), max(y0, y1, y2)
    elif kind == DISC:
        lox, hix, loy, hiy = x0 - x1, x0 + x1, y0 - x1, y0 + x1
    elif kind == CAPSULE:
        lox, hix, loy, hiy = min(x0, x1) - x2, max(x0, x1) + x2, min(y0, y1) - x2, max(y0, y1) + x2
    else:
        return 0, W, 0, H
    # sample 16 p + 8 inside [lo, hi]  <=>  ceil((lo - 8) / 16) <= p <= floor((hi - 8) / 16)
    return (max(0, -((8 - lox) // 16)), min(W, (hix - 8) // 16 + 1), max(0, -((8 - loy) // 16)), min(H, (hiy - 8) // 16 + 1))


def rasterise(prims, counts, W, H, windowed=True):
    """prims int[n, cap, 8], counts int[n] -> uint8[n, H, W]: painter's order over exact integer predicates.  windowed: evaluate a
    primitive over its bounding box only (the same bytes, test_render_host.py holds the two forms equal; False: every pixel)."""
    prims = np.asarray(prims, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    n, cap = prims.shape[:2]
    frames = np.zeros((n, H, W), dtype=np.uint8)
    for f in range(n):
        for i in range(int(min(max(counts[f], 0), cap))):
            prim = prims[f, i]
            c0, c1, r0, r1 = _window(prim, W, H) if windowed else (0, W, 0, H)
            if c0 >= c1 or r0 >= r1:
                continue
            Y, X = np.meshgrid(16 * np.arange(r0, r1, dtype=np.int64) + 8, 16 * np.arange(c0, c1, dtype=np.int64) + 8, indexing="ij")
            view = frames[f, r0:r1, c0:c1]
            view[covered(prim, X, Y)] = int(prim[1]) & 15
    return frames


# ---- the scenes -------------------------------------------------------------------------------------------------------------
class Scene:
    def __init__(self, W, H):
        self.W, self.H, self.prims = W, H, []

    def unit(self, v):
        return int(np.rint(np.clip(v, -1.0e6, 1.0e6)))

    def ux(self, x_px):
        return self.unit(16.0 * x_px)

    def uy(self, y_px):
        return self.unit(16.0 * self.H - 16.0 * y_px)

    def emit(self, kind, colour, x0=0, y0=0, x1=0, y1=0, x2=0, y2=0):
        wu, hu = 16 * self.W, 16 * self.H
        if kind == TRI:
            lox, hix, loy, hiy = min(x0, x1, x2), max(x0, x1, x2), min(y0, y1, y2), max(y0, y1, y2)
        elif kind == DISC:
            lox, hix, loy, hiy = x0 - x1, x0 + x1, y0 - x1, y0 + x1
        elif kind == CAPSULE:
            lox, hix, loy, hiy = min(x0, x1) - x2, max(x0, x1) + x2, min(y0, y1) - x2, max(y0, y1) + x2
        else:
            lox, hix, loy, hiy = 0, wu, 0, hu
        if hix < 0 or lox > wu or hiy < 0 or loy > hu or len(self.prims) >= MAX_PRIMS:
            return
        self.prims.append([kind, colour] + [int(np.clip(v, COORD_MIN, COORD_MAX)) for v in (x0, y0, x1, y1, x2, y2)])

    def result(self):
        out = np.zeros((MAX_PRIMS, 8), dtype=np.int32)
        if self.prims:
            out[:len(self.prims)] = np.array(self.prims, dtype=np.int32)
        return out, len(self.prims)


def scene_cartpole(blob):
    """blob: float32[4] = x, x', theta, theta'"""
    x, th = float(blob[0]), float(blob[2])
    sc = Scene(600, 400)
    x_px = 300.0 + 125.0 * x
    sc.emit(FILL, WHITE)
    sc.emit(CAPSULE, BLACK, sc.ux(0.0), sc.uy(100.0), sc.ux(600.0), sc.uy(100.0), 8)
    L, R, B, T = sc.ux(x_px - 25.0), sc.ux(x_px + 25.0), sc.uy(100.0 - 15.0), sc.uy(100.0 + 15.0)
    sc.emit(TRI, BLACK, L, B, R, B, R, T)
    sc.emit(TRI, BLACK, L, B, R, T, L, T)
    ex, ey = x_px + 120.0 * np.sin(th), 107.5 + 120.0 * np.cos(th)
    sc.emit(CAPSULE, POLE, sc.ux(x_px), sc.uy(107.5), sc.ux(ex), sc.uy(ey), 80)
    sc.emit(DISC, AXLE, sc.ux(x_px), sc.uy(107.5), 80)
    return sc.result()


def scene_spread(blob, na):
    """blob: float32[6 na] = agent x[na], y[na], vx[na], vy[na], landmark x[na], y[na]"""
    b = np.asarray(blob, dtype=np.float64)
    ax, ay, lx, ly = b[0:na], b[na:2 * na], b[4 * na:5 * na], b[5 * na:6 * na]
    sc = Scene(400, 400)
    sc.emit(FILL, WHITE)
    for a in range(na):
        sc.emit(DISC, LANDMARK, sc.ux(200.0 + 100.0 * lx[a]), sc.uy(200.0 + 100.0 * ly[a]), 80)
    for a in range(na):
        sc.emit(DISC, AGENT, sc.ux(200.0 + 100.0 * ax[a]), sc.uy(200.0 + 100.0 * ay[a]), 240)
    return sc.result()


# gym's polygons (lunar_lander.py LANDER_POLY and the leg box, bipedal_walker.py HULL_POLY and the leg boxes), in pixels / 30, listed
# in the order Box2D stores a polygon's vertices (counter-clockwise from the lowest of the rightmost points)
POLY_LANDER_HULL = np.array([(17, -10), (17, 0), (14, 17), (-14, 17), (-17, 0), (-17, -10)], dtype=np.float64) / 30.0
POLY_LANDER_LEG = np.array([(-2, -8), (2, -8), (2, 8), (-2, 8)], dtype=np.float64) / 30.0
POLY_WALKER_HULL = np.array([(34, -8), (34, 1), (6, 9), (-30, 9), (-30, -8)], dtype=np.float64) / 30.0
POLY_WALKER_UPPER = np.array([(-4, -17), (4, -17), (4, 17), (-4, 17)], dtype=np.float64) / 30.0
POLY_WALKER_LOWER = np.array([(-3.2, -17), (3.2, -17), (3.2, 17), (-3.2, 17)], dtype=np.float64) / 30.0


def polygon_centroid(v):
    """area centroid of a simple polygon (what b2PolygonShape::ComputeMass takes as the local centre of a one-fixture body)"""
    x, y = v[:, 0], v[:, 1]
    xn, yn = np.roll(x, -1), np.roll(y, -1)
    w = x * yn - xn * y
    return np.array([((x + xn) * w).sum(), ((y + yn) * w).sum()]) / (3.0 * w.sum())


def _origin(body, local_centre):
    """body = (cx, cy, angle, ...): the centre of mass and the angle; -> the body origin (b2Body position) and (sin, cos)"""
    cx, cy, a = float(body[0]), float(body[1]), float(body[2])
    s, c = np.sin(a), np.cos(a)
    return cx - (c * local_centre[0] - s * local_centre[1]), cy - (s * local_centre[0] + c * local_centre[1]), s, c


def _emit_body(sc, colour, body, local_centre, poly, scroll):
    px, py, s, c = _origin(body, local_centre)
    X = [sc.ux(30.0 * (px + (c * vx - s * vy) - scroll)) for vx, vy in poly]
    Y = [sc.uy(30.0 * (py + (s * vx + c * vy))) for vx, vy in poly]
    for v in range(1, len(poly) - 1):
        sc.emit(TRI, colour, X[0], Y[0], X[v], Y[v], X[v + 1], Y[v + 1])


def _emit_ground(sc, colour, x1, y1, x2, y2, scroll):
    X1, X2 = sc.ux(30.0 * (x1 - scroll)), sc.ux(30.0 * (x2 - scroll))
    Y1, Y2, Y0 = sc.uy(30.0 * y1), sc.uy(30.0 * y2), sc.uy(0.0)
    sc.emit(TRI, colour, X1, Y1, X2, Y2, X2, Y0)
    sc.emit(TRI, colour, X1, Y1, X2, Y0, X1, Y0)


def _emit_flag(sc, pole_colour, pole_r, flag_colour, x, y, scroll):
    top = y + 50.0 / 30.0
    X = sc.ux(30.0 * (x - scroll))
    sc.emit(CAPSULE, pole_colour, X, sc.uy(30.0 * y), X, sc.uy(30.0 * top), pole_r)
    sc.emit(TRI, flag_colour, X, sc.uy(30.0 * top), X, sc.uy(30.0 * (top - 10.0 / 30.0)), sc.ux(30.0 * (x + 25.0 / 30.0 - scroll)),
            sc.uy(30.0 * (top - 5.0 / 30.0)))


def scene_lander(bodies, terrain):
    """bodies[3, >= 3] = (cx, cy, angle, ...) of hull / leg -1 / leg +1 (LanderSim.debug()), terrain[11] heights at x = 0, 2, .., 20"""
    sc = Scene(600, 400)
    sc.emit(FILL, BLACK)
    for k in range(10):
        _emit_ground(sc, WHITE, 2.0 * k, float(terrain[k]), 2.0 * (k + 1), float(terrain[k + 1]), 0.0)
    helipad_y = 400.0 / 30.0 / 4.0
    for x in (8.0, 12.0):
        _emit_flag(sc, WHITE, 8, YELLOW, x, helipad_y, 0.0)
    for k in (1, 2):
        _emit_body(sc, LANDER_LEG, bodies[k], (0.0, 0.0), POLY_LANDER_LEG, 0.0)
    _emit_body(sc, HULL, bodies[0], polygon_centroid(POLY_LANDER_HULL), POLY_LANDER_HULL, 0.0)
    return sc.result()



def scene_walker(bodies, terrain, lidar, local_centres):
    """bodies[5, >= 3] and terrain[200] from WalkerSim.debug(), lidar[10] = the observation's fractions, local_centres[5, 2] from
    walker_body_props()"""
    sc = Scene(600, 400)
    step = 14.0 / 30.0
    hx, hy, _, _ = _origin(bodies[0], local_centres[0])
    scroll = hx - 600.0 / 30.0 / 5.0
    sc.emit(FILL, SKY)
    for k in range(199):
        _emit_ground(sc, GRASS, k * step, float(terrain[k]), (k + 1) * step, float(terrain[k + 1]), scroll)
    _emit_flag(sc, BLACK, 16, FLAG, 3.0 * step, 400.0 / 30.0 / 4.0, scroll)
    HX, HY = sc.ux(30.0 * (hx - scroll)), sc.uy(30.0 * hy)
    for i in range(10):
        ang = 1.5 * i / 10.0
        ex = hx + float(lidar[i]) * (np.sin(ang) * (160.0 / 30.0))
        ey = hy - float(lidar[i]) * (np.cos(ang) * (160.0 / 30.0))
        sc.emit(CAPSULE, RED, HX, HY, sc.ux(30.0 * (ex - scroll)), sc.uy(30.0 * ey), 8)
    for k in (1, 2, 3, 4):
        _emit_body(sc, LEG_NEAR if k <= 2 else LEG_FAR, bodies[k], local_centres[k], POLY_WALKER_UPPER if k in (1, 3) else POLY_WALKER_LOWER,
                   scroll)
    _emit_body(sc, HULL, bodies[0], local_centres[0], POLY_WALKER_HULL, scroll)
    return sc.result(), scroll
