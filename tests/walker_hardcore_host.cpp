// walker_hardcore_host.cpp -- TEST INFRASTRUCTURE.  Host build of BipedalWalkerHardcore-v3 (simple-es_amd/csrc/ses_walker_hardcore_env.h
// on the Box2D-style world of ses_b2.h) with C entry points for tests/walker_hardcore_host.py.  The B2_* macros are the host's, as
// oracle/ses_b2_oracle.cpp defines them; the keyed Philox stream is restated here (Philox4x32-10, Salmon et al. 2011; counter and
// key laid out as ses_rng.h's philox_words(seed, TAG_ENV_TERRAIN, 0, 0, i)) so that this file links against nothing:
// tests/test_walker_hardcore_host.py holds it to the oracle's through BipedalWalker-v3's terrain.
#include <math.h>
#include <stdint.h>
#include <string.h>

extern "C" {
#include "ses_oracle_math.h"
}

#define B2_FN static inline
#define B2_NOINLINE static __attribute__((noinline))
#define B2_FN_MEMBER inline
#define B2_CONST static const
#define B2_UNROLL
#define B2_SINCOS(a, s, c) o_sincosf((a), &(s), &(c))
#define B2_SQRT(x) sqrtf(x)
#define B2_FLOOR(x) floorf(x)
#define B2_RARE_PATH asm volatile("")
#define B2_F2U(f) o_f2u(f)

static inline void bwh_philox(uint32_t key0, uint32_t key1, uint32_t i, uint32_t (&out)[4])
{
    uint32_t c[4] = {i, 0u, 0u, (uint32_t)(3ull << 24)}, k0 = key0, k1 = key1;
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    for (int j = 0; j < 4; ++j) out[j] = c[j];
}
static inline float bwh_unit(uint32_t r) { return o_fma((float)r, 0x1.0p-32f, 0x1.0p-33f); }
#define B2_TERRAIN_RAND3(k0, k1, i, u, r, q)                       \
    do {                                                           \
        uint32_t w_[4];                                            \
        bwh_philox((k0), (k1), (uint32_t)(i), w_);                 \
        u = o_fma(bwh_unit(w_[0]), 2.0f, -1.0f);                   \
        r = w_[1];                                                 \
        q = w_[2];                                                 \
    } while (0)
#define B2_TERRAIN_RAND(k0, k1, i, u, r)                           \
    do {                                                           \
        uint32_t q_;                                               \
        B2_TERRAIN_RAND3(k0, k1, i, u, r, q_);                     \
        (void)q_;                                                  \
    } while (0)

#include "ses_walker_hardcore_env.h"

using namespace b2l;

// the first bwh_blob_size() bytes are the step-wise env's state blob on the device (ses_walker_hardcore.hip: HardcoreBlob)
struct HardcoreSim {
    WalkerHardcoreEnv env;
    float row[BWH_ROW];
    uint8_t kind[BW_TERRAIN_LENGTH];
};

template <class D>
static void shift_bodies(WalkerEnvT<D> &e, float dx, float dy)
{
    for (int b = 0; b < 5; ++b) {
        e.w.body[b].cx += dx; e.w.body[b].cy += dy;
        e.w.xf[b].px += dx; e.w.xf[b].py += dy;
    }
    e.posx += dx; e.posy += dy;
    e.prev_shaping += 130.0f * dx / BW_SCALE;        // the shift itself earns nothing
}

extern "C" {

int bwh_state_size(void) { return (int)sizeof(HardcoreSim); }
int bwh_blob_size(void) { return (int)(sizeof(WalkerHardcoreEnv) + sizeof(float) * BWH_ROW); }
int bwh_row_floats(void) { return BWH_ROW; }

void bwh_obs(const void *state, float *obs)
{
    float o[24];
    walker_obs(((const HardcoreSim *)state)->env, o);
    memcpy(obs, o, sizeof o);
}

// init row: [0] initial-force uniform, [1], [2] the bit patterns of the terrain key, [3] unused
void bwh_reset(void *state, const float *u4, float *obs)
{
    HardcoreSim *s = (HardcoreSim *)state;
    memset(s, 0, sizeof *s);
    hardcore_terrain_generate(o_f2u(u4[1]), o_f2u(u4[2]), s->row, s->kind);
    const HardcoreTerrain terr{s->row};
    walker_reset(s->env, terr, u4);
    if (obs) bwh_obs(state, obs);
}

float bwh_step(void *state, const float *action4, float *obs, int32_t *done)
{
    HardcoreSim *s = (HardcoreSim *)state;
    const HardcoreTerrain terr{s->row};
    const float a[4] = {action4[0], action4[1], action4[2], action4[3]};
    bool d;
    const float r = walker_step(s->env, terr, a, d);
    if (obs) bwh_obs(state, obs);
    *done = d ? 1 : 0;
    return r;
}

// test-only: every body moved by (dx, dy), velocities kept; the manifolds keep their old edges and end at the next step
void bwh_shift(void *state, float dx, float dy) { shift_bodies(((HardcoreSim *)state)->env, dx, dy); }
// ... and the same on BipedalWalker-v3's env (the head of the oracle's WalkerSim), the yardstick of the physics tests
void bw_shift(void *walker_env, float dx, float dy) { shift_bodies(*(WalkerEnv *)walker_env, dx, dy); }

// ---- terrain rows ----
void bwh_row_generate(uint32_t key0, uint32_t key1, float *row, uint8_t *kind199) { hardcore_terrain_generate(key0, key1, row, kind199); }
// spans given: yl[199], yr[199]
void bwh_row_from_spans(const float *yl, const float *yr, float *row)
{
    memset(row, 0, sizeof(float) * BWH_ROW);
    memcpy(row, yl, sizeof(float) * BWH_COLS);
    memcpy(row + BWH_COLS, yr, sizeof(float) * BWH_COLS);
    hardcore_terrain_index(row);
}
// edges[n][4] = x1, y1, x2, y2 (room for 400); returns n
int bwh_row_edges(const float *row, float *edges)
{
    const HardcoreTerrain terr{row};
    const int n = terr.n_edges();
    for (int k = 0; k < n; ++k) terr.edge(k, edges[4 * k], edges[4 * k + 1], edges[4 * k + 2], edges[4 * k + 3]);
    return n;
}
int bwh_row_index_of(const float *row, float x) { return HardcoreTerrain{row}.index_of(x); }
float bwh_row_raycast(const float *row, float p1x, float p1y, float p2x, float p2y)
{
    return walker_raycast(HardcoreTerrain{row}, p1x, p1y, p2x, p2y);
}
void bwh_state_row(const void *state, float *row, uint8_t *kind199)
{
    const HardcoreSim *s = (const HardcoreSim *)state;
    memcpy(row, s->row, sizeof s->row);
    if (kind199) memcpy(kind199, s->kind, BWH_COLS);
}

// BipedalWalker-v3's terrain type and generator, for comparison
void bw_terrain_heights(uint32_t key0, uint32_t key1, float *ty200) { walker_terrain_heights(key0, key1, ty200); }
int bw_edges(const float *ty200, float *edges)
{
    const WalkerTerrain terr{ty200};
    for (int k = 0; k < terr.n_edges(); ++k) terr.edge(k, edges[4 * k], edges[4 * k + 1], edges[4 * k + 2], edges[4 * k + 3]);
    return terr.n_edges();
}
int bw_index_of(const float *ty200, float x) { return WalkerTerrain{ty200}.index_of(x); }

// ---- diagnostics ----
// per leg manifold [4][8]: -1 not touching; 0 touching a ground edge (pad, grass, pit lip, first tread); 1 touching an obstacle
// edge: a riser, a stump top, a tread after the first or a pit floor.  edges [4][8]: the manifold's edge index (or -1)
void bwh_manifold_flags(const void *state, int32_t *flags, int32_t *edges)
{
    const HardcoreSim *s = (const HardcoreSim *)state;
    const uint8_t *n = HardcoreTerrain{s->row}.bytes();
    for (int b = 0; b < 4; ++b)
        for (int r = 0; r < WalkerHardcoreDef::NSLOT; ++r) {
            const Manifold &m = s->env.w.mf[b][r];
            int f = -1;
            if (m.edge >= 0 && m.count > 0) {
                const int c = n[BW_TERRAIN_LENGTH + m.edge];
                const bool span = m.edge == c + (int)n[c];
                f = (!span || s->kind[c] != BWH_KIND_GROUND) ? 1 : 0;
            }
            flags[b * WalkerHardcoreDef::NSLOT + r] = f;
            edges[b * WalkerHardcoreDef::NSLOT + r] = m.count > 0 ? m.edge : -1;
        }
}

// bodies [5][6] = (cx, cy, angle, vx, vy, omega); ints = {game_over, leg contact x4}
void bwh_debug(const void *state, float *bodies, int32_t *ints)
{
    const HardcoreSim *s = (const HardcoreSim *)state;
    for (int b = 0; b < 5; ++b) {
        const Body &B = s->env.w.body[b];
        const float v[6] = {B.cx, B.cy, B.a, B.vx, B.vy, B.w};
        memcpy(bodies + 6 * b, v, sizeof v);
    }
    ints[0] = s->env.w.game_over;
    for (int b = 1; b < 5; ++b) ints[b] = s->env.w.ground_contact[b];
}

// the terrain edges the hull touches in its present pose (collide_body's hull loop, which only sets game_over): edges[] gets the
// indices, returns their number (room for 16)
int bwh_hull_touching(const void *state, int32_t *edges)
{
    const HardcoreSim *s = (const HardcoreSim *)state;
    const HardcoreTerrain terr{s->row};
    const Poly &P = WALKER_POLY[0];
    Xf xf;
    xf_of(s->env.w.body[0], WALKER_BODY[0], xf);
    float wx[6], wy[6], wnx[6], wny[6];
    float xmin = FLT_BIG, xmax = -FLT_BIG;
    for (int i = 0; i < 6; ++i) {
        const bool in = i < P.n;
        wx[i] = in ? (xf.c * P.vx[i] - xf.s * P.vy[i]) + xf.px : 0.0f;
        wy[i] = in ? (xf.s * P.vx[i] + xf.c * P.vy[i]) + xf.py : 0.0f;
        wnx[i] = in ? xf.c * P.nx[i] - xf.s * P.ny[i] : 0.0f;
        wny[i] = in ? xf.s * P.nx[i] + xf.c * P.ny[i] : 0.0f;
        if (in) { xmin = b2min(xmin, wx[i]); xmax = b2max(xmax, wx[i]); }
    }
    const float ccx = (xf.c * P.cx - xf.s * P.cy) + xf.px, ccy = (xf.s * P.cx + xf.c * P.cy) + xf.py;
    int k_lo = terr.index_of(xmin - AABB_EXTENSION), k_hi = terr.index_of(xmax + AABB_EXTENSION), n = 0;
    k_lo = k_lo < 0 ? 0 : k_lo;
    k_hi = k_hi > terr.n_edges() - 1 ? terr.n_edges() - 1 : k_hi;
    for (int k = k_lo; k <= k_hi && n < 16; ++k) {
        float x1, y1, x2, y2;
        terr.edge(k, x1, y1, x2, y2);
        Manifold tmp;
        collide_edge_polygon(P, xf, wx, wy, wnx, wny, ccx, ccy, x1, y1, x2, y2, tmp);
        if (tmp.count > 0) edges[n++] = k;
    }
    return n;
}

// world vertices of the five polygons of bodies [5][6] (either walker: the bodies are the same): verts [5][6][2], counts [5]
void bwh_vertices(const float *bodies, float *verts, int32_t *counts)
{
    for (int b = 0; b < 5; ++b) {
        Body B;
        memset(&B, 0, sizeof B);
        B.cx = bodies[6 * b]; B.cy = bodies[6 * b + 1]; B.a = bodies[6 * b + 2];
        Xf xf;
        xf_of(B, WALKER_BODY[b], xf);
        const Poly &P = WALKER_POLY[b];
        counts[b] = P.n;
        for (int i = 0; i < 6; ++i) {
            const bool in = i < P.n;
            verts[(b * 6 + i) * 2] = in ? (xf.c * P.vx[i] - xf.s * P.vy[i]) + xf.px : 0.0f;
            verts[(b * 6 + i) * 2 + 1] = in ? (xf.s * P.vx[i] + xf.c * P.vy[i]) + xf.py : 0.0f;
        }
    }
}

}  // extern "C"
