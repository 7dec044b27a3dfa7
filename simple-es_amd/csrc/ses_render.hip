// ses_render.hip -- episodes as pictures, on the device: `env.render()` of the reference's wrappers (envs/gym_wrapper.py:50-51,
// envs/pettingzoo_wrapper.py:63-64) and the frames its test.py --save-gif collects (test.py:59-67), for n state blobs at once.
//
// Two layers (the numbers are in ses_render.h):
//   * scene builders, one per env: one lane turns one state blob of the step-wise envs (ses_env_blobs.h) into a short list of
//     integer primitives -- the build's own depictions, modelled on gym's / pettingzoo's renderers, pixel parity a non-goal;
//   * the rasteriser, env-independent: one launch turns F primitive lists into F palette-indexed frames.  Its result is
//     defined by exact integer predicates alone (include/ses.h), so tests/render_np.py restates it in numpy byte for byte.
// Neither synchronises the device; both run on the handle's stream.
#include "ses_env_blobs.h"
#include "ses_internal.h"
#include "ses_reacher.h"
#include "ses_render.h"

namespace ses {

// ---- scene builders ---------------------------------------------------------------------------------------------------
// float32, one rounding per operation (the unit is also built with -ffp-contract=off; the intrinsics say it where it matters)
__device__ __forceinline__ float rmul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float radd(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float rsub(float a, float b) { return __fsub_rn(a, b); }

struct Scene {
    int32_t *prims;      // this state's [RENDER_MAX_PRIMS][8]
    int n;
    int wu, hu;          // the canvas in units: 16 * width, 16 * height
    float hu_f;
};

__device__ __forceinline__ int to_unit(float v) { return (int)__builtin_rintf(min_(max_(v, -1.0e6f), 1.0e6f)); }
// pixel coordinates (x to the right, y UP from the bottom edge, as the upstream renderers count) -> units, y down
__device__ __forceinline__ int ux(float x_px) { return to_unit(rmul(16.0f, x_px)); }
__device__ __forceinline__ int uy(const Scene &sc, float y_px) { return to_unit(rsub(sc.hu_f, rmul(16.0f, y_px))); }
__device__ __forceinline__ int clamp_coord(int v) { return v < RENDER_COORD_MIN ? RENDER_COORD_MIN : (v > RENDER_COORD_MAX ? RENDER_COORD_MAX : v); }

// the general rule of the scenes: a primitive whose bounding box lies wholly outside the canvas is dropped, the coordinates
// of the others are clamped into the defined range; a list that is full drops what follows
__device__ __forceinline__ void emit(Scene &sc, int kind, int colour, int x0, int y0, int x1, int y1, int x2, int y2)
{
    int lox, hix, loy, hiy;
    if (kind == RENDER_TRI) {
        lox = min(x0, min(x1, x2)); hix = max(x0, max(x1, x2));
        loy = min(y0, min(y1, y2)); hiy = max(y0, max(y1, y2));
    } else if (kind == RENDER_DISC) {
        lox = x0 - x1; hix = x0 + x1; loy = y0 - x1; hiy = y0 + x1;
    } else if (kind == RENDER_CAPSULE) {
        lox = min(x0, x1) - x2; hix = max(x0, x1) + x2;
        loy = min(y0, y1) - x2; hiy = max(y0, y1) + x2;
    } else {
        lox = 0; hix = sc.wu; loy = 0; hiy = sc.hu;
    }
    if (hix < 0 || lox > sc.wu || hiy < 0 || loy > sc.hu) return;
    if (sc.n >= RENDER_MAX_PRIMS) return;
    int32_t *p = sc.prims + (size_t)sc.n * RENDER_WORDS;
    p[0] = kind; p[1] = colour;
    p[2] = clamp_coord(x0); p[3] = clamp_coord(y0); p[4] = clamp_coord(x1); p[5] = clamp_coord(y1);
    p[6] = clamp_coord(x2); p[7] = clamp_coord(y2);
    sc.n += 1;
}
__device__ __forceinline__ void emit_fill(Scene &sc, int colour) { emit(sc, RENDER_FILL, colour, 0, 0, 0, 0, 0, 0); }
__device__ __forceinline__ void emit_tri(Scene &sc, int colour, int x0, int y0, int x1, int y1, int x2, int y2)
{
    emit(sc, RENDER_TRI, colour, x0, y0, x1, y1, x2, y2);
}
__device__ __forceinline__ void emit_disc(Scene &sc, int colour, int x, int y, int r) { emit(sc, RENDER_DISC, colour, x, y, r, 0, 0, 0); }
__device__ __forceinline__ void emit_capsule(Scene &sc, int colour, int ax, int ay, int bx, int by, int r)
{
    emit(sc, RENDER_CAPSULE, colour, ax, ay, bx, by, r, 0);
}

// CartPole (gym's classic_control rendering): 600 x 400, 125 px per unit of x, the cart 100 px above the bottom edge
__device__ __forceinline__ void scene_of(Scene &sc, const CartPoleBlob &b)
{
    const float x_px = radd(CP_CENTRE_X, rmul(CP_PX_PER_UNIT, b.st.x));
    emit_fill(sc, PAL_WHITE);
    emit_capsule(sc, PAL_BLACK, ux(0.0f), uy(sc, CP_CART_Y), ux((float)CP_W), uy(sc, CP_CART_Y), CP_TRACK_R);
    const int L = ux(rsub(x_px, CP_CART_HALF_W)), R = ux(radd(x_px, CP_CART_HALF_W));
    const int B = uy(sc, rsub(CP_CART_Y, CP_CART_HALF_H)), T = uy(sc, radd(CP_CART_Y, CP_CART_HALF_H));
    emit_tri(sc, PAL_BLACK, L, B, R, B, R, T);
    emit_tri(sc, PAL_BLACK, L, B, R, T, L, T);
    float s, c;
    sincos_(b.st.th, s, c);
    const float ex = radd(x_px, rmul(CP_POLE_LEN, s)), ey = radd(CP_PIVOT_Y, rmul(CP_POLE_LEN, c));   // positive theta leans right
    emit_capsule(sc, PAL_POLE, ux(x_px), uy(sc, CP_PIVOT_Y), ux(ex), uy(sc, ey), CP_POLE_R);
    emit_disc(sc, PAL_AXLE, ux(x_px), uy(sc, CP_PIVOT_Y), CP_AXLE_R);
}

// simple_spread (pettingzoo's mpe rendering): the world square [-2, 2]^2 on 400 x 400
template <int NA>
__device__ __forceinline__ void scene_of(Scene &sc, const SpreadBlob<NA> &b)
{
    emit_fill(sc, PAL_WHITE);
    for (int a = 0; a < NA; ++a)
        emit_disc(sc, PAL_LANDMARK, ux(radd(SP_CENTRE, rmul(SP_PX_PER_UNIT, b.st.lx[a]))),
                  uy(sc, radd(SP_CENTRE, rmul(SP_PX_PER_UNIT, b.st.ly[a]))), SP_LANDMARK_R);
    for (int a = 0; a < NA; ++a)
        emit_disc(sc, PAL_AGENT, ux(radd(SP_CENTRE, rmul(SP_PX_PER_UNIT, b.st.ax[a]))),
                  uy(sc, radd(SP_CENTRE, rmul(SP_PX_PER_UNIT, b.st.ay[a]))), SP_AGENT_R);
}

// a body polygon of the Box2D-style world as a fan of triangles: the unit's own polygon table, transformed by the body's
// stored pose (xf_of: the world keeps the centre of mass and the angle; World::xf is the transform of the step's START)
__device__ __forceinline__ void emit_body(Scene &sc, int colour, const b2l::Body &body, const b2l::BodyDef &def, const b2l::Poly &poly,
                                          float scroll)
{
    b2l::Xf xf;
    b2l::xf_of(body, def, xf);
    int X[6], Y[6];
    for (int v = 0; v < poly.n; ++v) {
        const float wx = radd(xf.px, rsub(rmul(xf.c, poly.vx[v]), rmul(xf.s, poly.vy[v])));
        const float wy = radd(xf.py, radd(rmul(xf.s, poly.vx[v]), rmul(xf.c, poly.vy[v])));
        X[v] = ux(rmul(BOX2D_PX_PER_UNIT, rsub(wx, scroll)));
        Y[v] = uy(sc, rmul(BOX2D_PX_PER_UNIT, wy));
    }
    for (int v = 1; v + 1 < poly.n; ++v) emit_tri(sc, colour, X[0], Y[0], X[v], Y[v], X[v + 1], Y[v + 1]);
}

// the terrain edge (x1, y1) - (x2, y2) as a quad down to y = 0
__device__ __forceinline__ void emit_ground(Scene &sc, int colour, float x1, float y1, float x2, float y2, float scroll)
{
    const int X1 = ux(rmul(BOX2D_PX_PER_UNIT, rsub(x1, scroll))), X2 = ux(rmul(BOX2D_PX_PER_UNIT, rsub(x2, scroll)));
    const int Y1 = uy(sc, rmul(BOX2D_PX_PER_UNIT, y1)), Y2 = uy(sc, rmul(BOX2D_PX_PER_UNIT, y2)), Y0 = uy(sc, 0.0f);
    emit_tri(sc, colour, X1, Y1, X2, Y2, X2, Y0);
    emit_tri(sc, colour, X1, Y1, X2, Y0, X1, Y0);
}

// a flag as gym draws it in both Box2D envs: a pole from (x, y) 50 px up, a 25 x 10 px triangular pennant at its top
__device__ __forceinline__ void emit_flag(Scene &sc, int pole_colour, int pole_r, int flag_colour, float x, float y, float scroll)
{
    const float top = radd(y, LL_FLAG_POLE);
    const int X = ux(rmul(BOX2D_PX_PER_UNIT, rsub(x, scroll)));
    emit_capsule(sc, pole_colour, X, uy(sc, rmul(BOX2D_PX_PER_UNIT, y)), X, uy(sc, rmul(BOX2D_PX_PER_UNIT, top)), pole_r);
    emit_tri(sc, flag_colour, X, uy(sc, rmul(BOX2D_PX_PER_UNIT, top)), X, uy(sc, rmul(BOX2D_PX_PER_UNIT, rsub(top, LL_FLAG_DROP))),
             ux(rmul(BOX2D_PX_PER_UNIT, rsub(radd(x, LL_FLAG_LEN), scroll))), uy(sc, rmul(BOX2D_PX_PER_UNIT, rsub(top, LL_FLAG_MID))));
}

// LunarLander (gym's lunar_lander.py render, without the particles): 600 x 400, 30 px per unit
__device__ __forceinline__ void scene_of(Scene &sc, const LanderBlob &b)
{
    emit_fill(sc, PAL_BLACK);
    for (int k = 0; k < b2l::LL_SEGMENTS; ++k)
        emit_ground(sc, PAL_WHITE, 2.0f * (float)k, b.ty[k], 2.0f * (float)(k + 1), b.ty[k + 1], 0.0f);
    emit_flag(sc, PAL_WHITE, LL_POLE_R, PAL_YELLOW, LL_HELIPAD_X1, b2l::LL_HELIPAD_Y, 0.0f);
    emit_flag(sc, PAL_WHITE, LL_POLE_R, PAL_YELLOW, LL_HELIPAD_X2, b2l::LL_HELIPAD_Y, 0.0f);
    for (int k = 1; k <= 2; ++k) emit_body(sc, PAL_LANDER_LEG, b.env.w.body[k], b2l::LANDER_BODY[k], b2l::LANDER_POLY[k], 0.0f);
    emit_body(sc, PAL_HULL, b.env.w.body[0], b2l::LANDER_BODY[0], b2l::LANDER_POLY[0], 0.0f);
}

// BipedalWalker (gym's bipedal_walker.py render, without the clouds): 600 x 400, 30 px per unit, scrolling with the hull
__device__ __forceinline__ void scene_of(Scene &sc, const WalkerBlob &b)
{
    const b2l::WalkerEnv &e = b.env;
    const float scroll = rsub(e.posx, BW_SCROLL_LEAD);
    emit_fill(sc, PAL_SKY);
    // the edges that can be in view (a superset: emit() drops the rest)
    int k_lo = (int)__builtin_floorf(scroll / b2l::BW_TERRAIN_STEP) - 1;
    int k_hi = (int)__builtin_floorf((scroll + b2l::BW_VIEWPORT_W) / b2l::BW_TERRAIN_STEP) + 1;
    k_lo = max(k_lo, 0);
    k_hi = min(k_hi, b2l::BW_TERRAIN_LENGTH - 2);
    for (int k = k_lo; k <= k_hi; ++k)
        emit_ground(sc, PAL_GRASS, rmul((float)k, b2l::BW_TERRAIN_STEP), b.ty[k], rmul((float)(k + 1), b2l::BW_TERRAIN_STEP), b.ty[k + 1],
                    scroll);
    emit_flag(sc, PAL_BLACK, BW_FLAG_POLE_R, PAL_FLAG, rmul(3.0f, b2l::BW_TERRAIN_STEP), b2l::BW_TERRAIN_HEIGHT, scroll);
    const int HX = ux(rmul(BOX2D_PX_PER_UNIT, rsub(e.posx, scroll))), HY = uy(sc, rmul(BOX2D_PX_PER_UNIT, e.posy));
    for (int i = 0; i < 10; ++i) {
        float s, c;
        sincos_(1.5f * (float)i / 10.0f, s, c);
        const float ex = radd(e.posx, rmul(e.lidar[i], rmul(s, b2l::BW_LIDAR_RANGE)));
        const float ey = rsub(e.posy, rmul(e.lidar[i], rmul(c, b2l::BW_LIDAR_RANGE)));
        emit_capsule(sc, PAL_RED, HX, HY, ux(rmul(BOX2D_PX_PER_UNIT, rsub(ex, scroll))), uy(sc, rmul(BOX2D_PX_PER_UNIT, ey)), BW_LIDAR_R);
    }
    for (int k = 1; k <= 4; ++k)
        emit_body(sc, k <= 2 ? PAL_LEG_NEAR : PAL_LEG_FAR, e.w.body[k], b2l::WALKER_BODY[k], b2l::WALKER_POLY[k], scroll);
    emit_body(sc, PAL_HULL, e.w.body[0], b2l::WALKER_BODY[0], b2l::WALKER_POLY[0], scroll);
}

// Reacher (csrc/ses_reacher.h): the target disc, the two links as capsules from the shoulder in the canvas centre, the fingertip
// disc on top.  In float64 with the env's own trig (the state is float64): every coordinate is one chain of correctly rounded
// operations and one rint, so a numpy restatement has the same integers.
__device__ __forceinline__ int rc_unit(double v) { return (int)__builtin_rint(v < -1.0e6 ? -1.0e6 : (v > 1.0e6 ? 1.0e6 : v)); }
__device__ __forceinline__ int rc_ux(double x) { return rc_unit(16.0 * (RC_CENTRE + RC_PX_PER_UNIT * x)); }
__device__ __forceinline__ int rc_uy(const Scene &sc, double y) { return rc_unit((double)sc.hu - 16.0 * (RC_CENTRE + RC_PX_PER_UNIT * y)); }
__device__ __forceinline__ void scene_of(Scene &sc, const ReacherState &s)
{
    ReacherTrig t;
    reacher_trig(s, t);
    const double ex = RC_L1 * t.ct, ey = RC_L1 * t.st;                              // the elbow
    const double fx = ex + RC_L2 * t.cb, fy = ey + RC_L2 * t.sb;                    // the fingertip
    emit_fill(sc, PAL_WHITE);
    emit_disc(sc, PAL_RED, rc_ux(s.tx), rc_uy(sc, s.ty), RC_TARGET_R);
    emit_capsule(sc, PAL_POLE, rc_ux(0.0), rc_uy(sc, 0.0), rc_ux(ex), rc_uy(sc, ey), RC_LINK_R);
    emit_capsule(sc, PAL_AXLE, rc_ux(ex), rc_uy(sc, ey), rc_ux(fx), rc_uy(sc, fy), RC_LINK_R);
    emit_disc(sc, PAL_AGENT, rc_ux(fx), rc_uy(sc, fy), RC_TIP_R);
}

// one lane = one state: the lists are short and serial by nature (painter's order); the frames are where the work is
template <class Blob>
__global__ __launch_bounds__(64) void k_render_scene(const Blob *__restrict__ state, int n, int width, int height,
                                                     int32_t *__restrict__ prims, int32_t *__restrict__ counts)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    Scene sc{prims + (size_t)i * RENDER_MAX_PRIMS * RENDER_WORDS, 0, 16 * width, 16 * height, (float)(16 * height)};
    scene_of(sc, state[i]);
    counts[i] = sc.n;
}

// ---- the rasteriser ---------------------------------------------------------------------------------------------------
// A workgroup of 256 owns one 64 x 64 tile of one frame and resolves it in four passes of 16 rows.  Thread i reads record i of the frame's list (cap <= 256), drops it
// when it cannot touch the tile -- not counted, a kind that draws nothing, a value outside the defined range, a bounding box
// that misses the tile, or anything in front of the list's last FILL -- and otherwise sets it up RELATIVE TO THE TILE: edge
// functions at the tile's first sample with their per-pixel steps, centres and squared radii.  The survivors are compacted in
// list order by ballot into LDS.  Then, pass by pass, every lane resolves four horizontally adjacent pixels against that list in painter's order (all
// lanes read the same record: an LDS broadcast), behind a 32-bit bounding-box test of its own span, and writes them with one
// 32-bit store; a span that crosses the right edge of the frame is written byte by byte.
// Everything is exact: with coordinates and radii in [-16384, 16383] and samples inside a 1024 x 1024 frame, differences stay
// below 2^16, cross products below 2^31 (int32), squared distances below 2^32 (uint32); the capsule's projection and the two
// sides of its distance test (cross^2 < 2^62, r^2 |d|^2 < 2^59) and the triangles' edge functions are held in 64 bits.
constexpr int RT_W = 64, RT_H = 64, RT_ROWS = 16, RT_THREADS = 256, RT_SPAN = 4;   // RT_ROWS: rows of a pass = RT_THREADS * RT_SPAN / RT_W
static_assert(RENDER_MAX_PRIMS <= RT_THREADS, "one thread sets up one record");

struct alignas(16) RasterRec {
    int32_t kind, colour;
    int32_t bx0, bx1, by0, by1;      // bounding box, units relative to the tile's first sample
    int32_t w[14];                   // TRI: E0[3] as {lo, hi}, step x [3], step y [3]; DISC: cx, cy, r^2;
                                     // CAPSULE: ax, ay, dx, dy, r^2, |d|^2, r^2 |d|^2 as {lo, hi}
};

__device__ __forceinline__ bool in_range(int v) { return v >= RENDER_COORD_MIN && v <= RENDER_COORD_MAX; }
__device__ __forceinline__ int64_t cross64(int ux_, int uy_, int vx, int vy) { return (int64_t)ux_ * vy - (int64_t)uy_ * vx; }

typedef uint32_t __attribute__((aligned(1))) u32_unaligned;

__global__ __launch_bounds__(RT_THREADS) void k_render_frames(const int32_t *__restrict__ prims, const int32_t *__restrict__ counts,
                                                              int cap, int width, int height, int tiles_x, int tiles_y,
                                                              uint8_t *__restrict__ frames)
{
    __shared__ RasterRec recs[RENDER_MAX_PRIMS];
    __shared__ int s_fill[RT_THREADS / 64], s_kept[RT_THREADS / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tiles = tiles_x * tiles_y;
    const int f = blockIdx.x / tiles, t = blockIdx.x - f * tiles;
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    const int px_first = tx * RT_W, py_first = ty * RT_H;
    const int ox = 16 * px_first + 8, oy = 16 * py_first + 8;              // the tile's first sample, absolute units
    const int last_x = 16 * (min(RT_W, width - px_first) - 1), last_y = 16 * (min(RT_H, height - py_first) - 1);   // its last, relative

    int cnt = counts[f];
    cnt = cnt > cap ? cap : cnt;
    const bool listed = tid < cnt;
    int p[RENDER_WORDS] = {-1, 0, 0, 0, 0, 0, 0, 0};
    if (listed) {
        const int32_t *src = prims + ((size_t)f * cap + tid) * RENDER_WORDS;
#pragma unroll
        for (int k = 0; k < RENDER_WORDS; ++k) p[k] = src[k];
    }
    const int kind = p[0];
    // nothing in front of the last FILL of the list can show
    const unsigned long long fills = __ballot(listed && kind == RENDER_FILL);
    if (lane == 0) s_fill[wave] = fills ? wave * 64 + 63 - __clzll((long long)fills) : -1;
    __syncthreads();
    int last_fill = s_fill[0];
#pragma unroll
    for (int w = 1; w < RT_THREADS / 64; ++w) last_fill = max(last_fill, s_fill[w]);

    RasterRec r;
    r.kind = kind; r.colour = p[1] & 15;
    bool keep = listed && tid >= last_fill;
    // the values a kind uses must be in the defined range (outside it the pixels are undefined: here, not drawn)
    if (kind == RENDER_TRI)
        keep = keep && in_range(p[2]) && in_range(p[3]) && in_range(p[4]) && in_range(p[5]) && in_range(p[6]) && in_range(p[7]);
    else if (kind == RENDER_DISC)
        keep = keep && in_range(p[2]) && in_range(p[3]) && in_range(p[4]) && p[4] >= 0;
    else if (kind == RENDER_CAPSULE)
        keep = keep && in_range(p[2]) && in_range(p[3]) && in_range(p[4]) && in_range(p[5]) && in_range(p[6]) && p[6] >= 0;
    else
        keep = keep && kind == RENDER_FILL;
    if (keep) {                                                            // (p[] is in range from here on: no sum below can overflow)
        int lox = ox, hix = ox + last_x, loy = oy, hiy = oy + last_y;      // bounding box, absolute units; FILL: the tile
        if (kind == RENDER_TRI) {
            lox = min(p[2], min(p[4], p[6])); hix = max(p[2], max(p[4], p[6]));
            loy = min(p[3], min(p[5], p[7])); hiy = max(p[3], max(p[5], p[7]));
        } else if (kind == RENDER_DISC) {
            lox = p[2] - p[4]; hix = p[2] + p[4]; loy = p[3] - p[4]; hiy = p[3] + p[4];
        } else if (kind == RENDER_CAPSULE) {
            lox = min(p[2], p[4]) - p[6]; hix = max(p[2], p[4]) + p[6];
            loy = min(p[3], p[5]) - p[6]; hiy = max(p[3], p[5]) + p[6];
        }
        r.bx0 = lox - ox; r.bx1 = hix - ox; r.by0 = loy - oy; r.by1 = hiy - oy;
        keep = r.bx1 >= 0 && r.bx0 <= last_x && r.by1 >= 0 && r.by0 <= last_y;
    }
    if (keep && kind == RENDER_TRI) {
        const int vx[3] = {p[2] - ox, p[4] - ox, p[6] - ox}, vy[3] = {p[3] - oy, p[5] - oy, p[7] - oy};
        const int64_t area = cross64(vx[1] - vx[0], vy[1] - vy[0], vx[2] - vx[0], vy[2] - vy[0]);
        keep = area != 0;
        const int s = area > 0 ? 1 : -1;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const int a = e, b = (e + 1) % 3;
            const int ex = s * (vx[b] - vx[a]), ey = s * (vy[b] - vy[a]);
            const int64_t e0 = cross64(ex, ey, -vx[a], -vy[a]);           // s * cross(vb - va, p - va) at the tile's first sample
            r.w[2 * e] = (int32_t)(uint32_t)e0; r.w[2 * e + 1] = (int32_t)(e0 >> 32);
            r.w[6 + e] = -16 * ey;                                         // ... one pixel to the right
            r.w[9 + e] = 16 * ex;                                          // ... one pixel down
        }
    } else if (keep && kind == RENDER_DISC) {
        r.w[0] = p[2] - ox; r.w[1] = p[3] - oy; r.w[2] = p[4] * p[4];
    } else if (keep && kind == RENDER_CAPSULE) {
        const int dx = p[4] - p[2], dy = p[5] - p[3];
        const uint32_t r2 = (uint32_t)(p[6] * p[6]), l2 = (uint32_t)(dx * dx) + (uint32_t)(dy * dy);
        const uint64_t r2l2 = (uint64_t)r2 * l2;
        r.w[0] = p[2] - ox; r.w[1] = p[3] - oy; r.w[2] = dx; r.w[3] = dy;
        r.w[4] = (int32_t)r2; r.w[5] = (int32_t)l2; r.w[6] = (int32_t)(uint32_t)r2l2; r.w[7] = (int32_t)(r2l2 >> 32);
    }
    const unsigned long long kept = __ballot(keep);
    if (lane == 0) s_kept[wave] = __popcll(kept);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < RT_THREADS / 64; ++w) {
        base += w < wave ? s_kept[w] : 0;
        total += s_kept[w];
    }
    if (keep) recs[base + __popcll(kept & ((1ull << lane) - 1ull))] = r;
    __syncthreads();

    // this lane's spans: four pixels of one row in each of the tile's passes (rows pass * 16 + tid / 16); a pass below the frame's
    // last row is skipped by the whole workgroup
    const int col = (tid & 15) * RT_SPAN;
    const int lx = 16 * col;                                               // the spans' first sample, relative to the tile's
    for (int pass = 0; pass < RT_H / RT_ROWS && py_first + pass * RT_ROWS < height; ++pass) {
        const int row = pass * RT_ROWS + (tid >> 4);
        const int ly = 16 * row;
        int c[RT_SPAN] = {0, 0, 0, 0};
        for (int j = 0; j < total; ++j) {
            const RasterRec &q = recs[j];
            if (q.bx1 < lx || q.bx0 > lx + 16 * (RT_SPAN - 1) || q.by1 < ly || q.by0 > ly) continue;
            const int k = __builtin_amdgcn_readfirstlane(q.kind);              // the same record in every lane: a scalar branch
            const int colour = q.colour;
            if (k == RENDER_FILL) {
#pragma unroll
                for (int i = 0; i < RT_SPAN; ++i) c[i] = colour;
            } else if (k == RENDER_TRI) {
                int64_t e[3];
#pragma unroll
                for (int n = 0; n < 3; ++n) {
                    const int64_t e0 = (int64_t)(((uint64_t)(uint32_t)q.w[2 * n + 1] << 32) | (uint32_t)q.w[2 * n]);
                    e[n] = e0 + (int64_t)(q.w[6 + n] * col + q.w[9 + n] * row);
                }
#pragma unroll
                for (int i = 0; i < RT_SPAN; ++i) {
                    c[i] = (e[0] | e[1] | e[2]) >= 0 ? colour : c[i];          // all three edge functions >= 0: no sign bit set
#pragma unroll
                    for (int n = 0; n < 3; ++n) e[n] += q.w[6 + n];
                }
            } else if (k == RENDER_DISC) {
                const int dy = ly - q.w[1];
                const uint32_t dy2 = (uint32_t)(dy * dy), r2 = (uint32_t)q.w[2];
#pragma unroll
                for (int i = 0; i < RT_SPAN; ++i) {
                    const int dx = lx + 16 * i - q.w[0];
                    c[i] = (uint32_t)(dx * dx) + dy2 <= r2 ? colour : c[i];
                }
            } else {
                const int dx = q.w[2], dy = q.w[3];
                const uint32_t r2 = (uint32_t)q.w[4], l2 = (uint32_t)q.w[5];
                const uint64_t r2l2 = ((uint64_t)(uint32_t)q.w[7] << 32) | (uint32_t)q.w[6];
                const int qy = ly - q.w[1];
#pragma unroll
                for (int i = 0; i < RT_SPAN; ++i) {
                    const int qx = lx + 16 * i - q.w[0];
                    const int64_t proj = (int64_t)dx * qx + (int64_t)dy * qy;                   // d . (p - a)
                    const int cr = dx * qy - dy * qx;                                           // cross(d, p - a), below 2^31
                    const uint32_t da2 = (uint32_t)(qx * qx) + (uint32_t)(qy * qy);
                    const uint32_t db2 = (uint32_t)((qx - dx) * (qx - dx)) + (uint32_t)((qy - dy) * (qy - dy));
                    const bool in = proj <= 0 ? da2 <= r2 : (proj >= (int64_t)l2 ? db2 <= r2 : (uint64_t)((int64_t)cr * cr) <= r2l2);
                    c[i] = in ? colour : c[i];
                }
            }
        }
        const int px = px_first + col, py = py_first + row;
        if (py < height && px < width) {
            uint8_t *dst = frames + ((size_t)f * height + py) * width + px;
            if (px + RT_SPAN <= width) {
                *(u32_unaligned *)dst = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24);
            } else {
                for (int i = 0; px + i < width; ++i) dst[i] = (uint8_t)c[i];
            }
        }
    }
}

static const char RENDER_ENVS[] = "CartPole-v0 / CartPole-v1, LunarLanderContinuous-v2 / LunarLander-v2, BipedalWalker-v3, simple_spread "
                                  "with 2 or 3 agents and ReacherBulletEnv-v0";

static bool render_canvas(const ses_handle *h, int *width, int *height)
{
    switch (h->cfg.env_id) {
        case SES_ENV_CARTPOLE: *width = CP_W; *height = CP_H; return true;
        case SES_ENV_LUNARLANDER:
        case SES_ENV_BIPEDALWALKER: *width = BOX2D_W; *height = BOX2D_H; return true;
        case SES_ENV_SIMPLE_SPREAD:
            if (h->cfg.n_agents != 2 && h->cfg.n_agents != 3) return false;
            *width = SP_W; *height = SP_H; return true;
        case SES_ENV_REACHER: *width = RC_W; *height = RC_H; return true;
        default: return false;
    }
}

template <class Blob>
static void launch_scene(ses_handle *h, const void *state, int n, int width, int height, int32_t *prims, int32_t *counts)
{
    hipLaunchKernelGGL(k_render_scene<Blob>, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, (const Blob *)state, n, width, height, prims,
                       counts);
}

}  // namespace ses

extern "C" {

int ses_render_palette(uint8_t *rgb)
{
    using namespace ses;
    SES_REQUIRE(rgb, "ses_render_palette: null argument");
    for (int k = 0; k < 48; ++k) rgb[k] = RENDER_PALETTE[k];
    return SES_OK;
}

int ses_render_size(ses_handle *h, int32_t *width, int32_t *height)
{
    using namespace ses;
    SES_REQUIRE(h && width && height, "ses_render_size: null argument");
    int w, ht;
    if (!render_canvas(h, &w, &ht)) return set_error(SES_ERR_UNSUPPORTED, "ses_render_size: no scene for this env; scenes exist for %s", RENDER_ENVS);
    *width = w; *height = ht;
    return SES_OK;
}

int ses_render_scene(ses_handle *h, const void *state, int32_t n, int32_t *prims, int32_t *counts)
{
    using namespace ses;
    SES_REQUIRE(h && state && prims && counts, "ses_render_scene: null argument");
    SES_REQUIRE(n >= 1, "ses_render_scene: n must be >= 1");
    int w, ht;
    if (!render_canvas(h, &w, &ht)) return set_error(SES_ERR_UNSUPPORTED, "ses_render_scene: no scene for this env; scenes exist for %s", RENDER_ENVS);
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    switch (h->cfg.env_id) {
        case SES_ENV_CARTPOLE: launch_scene<CartPoleBlob>(h, state, n, w, ht, prims, counts); break;
        case SES_ENV_SIMPLE_SPREAD:
            if (h->cfg.n_agents == 2) launch_scene<SpreadBlob<2>>(h, state, n, w, ht, prims, counts);
            else launch_scene<SpreadBlob<3>>(h, state, n, w, ht, prims, counts);
            break;
        case SES_ENV_LUNARLANDER: launch_scene<LanderBlob>(h, state, n, w, ht, prims, counts); break;
        case SES_ENV_REACHER: launch_scene<ReacherState>(h, state, n, w, ht, prims, counts); break;
        default: launch_scene<WalkerBlob>(h, state, n, w, ht, prims, counts); break;
    }
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int ses_render_frames(ses_handle *h, const int32_t *prims, const int32_t *counts, int32_t n, int32_t cap, int32_t width, int32_t height,
                      uint8_t *frames)
{
    using namespace ses;
    SES_REQUIRE(h && prims && counts && frames, "ses_render_frames: null argument");
    SES_REQUIRE(n >= 1, "ses_render_frames: n must be >= 1");
    SES_REQUIRE(cap >= 1 && cap <= RENDER_MAX_PRIMS, "ses_render_frames: cap must be in 1..%d, got %d", RENDER_MAX_PRIMS, cap);
    SES_REQUIRE(width >= 1 && width <= RENDER_MAX_SIDE, "ses_render_frames: width must be in 1..%d, got %d", RENDER_MAX_SIDE, width);
    SES_REQUIRE(height >= 1 && height <= RENDER_MAX_SIDE, "ses_render_frames: height must be in 1..%d, got %d", RENDER_MAX_SIDE, height);
    const int tiles_x = ceil_div(width, RT_W), tiles_y = ceil_div(height, RT_H);
    const long long blocks = (long long)n * tiles_x * tiles_y;
    SES_REQUIRE(blocks <= 0x7fffffffLL, "ses_render_frames: %d frames of %d x %d are more tiles than one launch holds", n, width, height);
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    hipLaunchKernelGGL(k_render_frames, dim3((unsigned)blocks), dim3(RT_THREADS), 0, h->stream, prims, counts, cap, width, height, tiles_x,
                       tiles_y, frames);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

}  // extern "C"
