// ses_walker_hardcore_env.h -- BipedalWalkerHardcore-v3: BipedalWalker-v3 (ses_walker_env.h: bodies, joints, motors, lidar,
// observation, reward, termination, init row) on a terrain with stumps, pits and stairs, modelled on gym 0.18-0.21's
// bipedal_walker.py with hardcore=True.  The build's own definition (DESIGN.md 7 is the specification; constants recalled, gym and
// Box2D absent: PARITY UNPINNED).
//
// What gym builds as static polygons resting on a height field is here ONE x-monotone polyline: a span per column, from
// (x_c, yl[c]) to (x_c+1, yr[c]), and a vertical riser at x_c exactly where yr[c - 1] != yl[c].  Walked left to right, its left-hand
// normal points out of the solid on every piece; the world's edge collision is two-sided anyway.  The world (ses_b2.h) is a
// template over the terrain type, so this is a new terrain type and a world definition with more manifold slots, nothing else:
//   - edges are indexed compactly in polyline order; index_of(x) is the SPAN of x's column.  The riser on that column's left
//     boundary has the next lower index and lies at x_c <= x, i.e. left of the fattened box the caller asks about: leaving it
//     out of the candidates loses nothing;
//   - the widest fattened box of a solved body is a lower leg lying flat, 34/30 + 2 * 0.1 = 1.33 m = 2.86 columns: it overlaps
//     at most 4 columns = 4 spans and the 3 risers between them = 7 candidate edges, hence NSLOT = 8 (the slot map wants a power
//     of two).  BipedalWalker-v3's 4 slots would cut candidates off silently once an obstacle sits under a leg.
//     What this bound covers is collide_body on a solved body's box at one pose.  The time-of-impact pass (world_solve_toi) applies
//     the same cut to the hull too, whose fattened box is 2.33 m = up to 6 columns and 11 edges, and to boxes that cover both ends
//     of a sweep: there the candidates past the eighth, at the right end, are still dropped -- a stump's riser in front of a fast
//     hull among them.  BipedalWalker-v3 cuts the same boxes to 4; what the cut costs is that a hull contact is found by the next
//     step's discrete pass (which looks at every edge under the hull, without slots) instead of inside the sweep;
//   - no edge has zero length: a span is one column long, and a riser exists only where the two heights differ.
// One text compiled for gfx950 (ses_walker_hardcore.hip) and for the host (tests/walker_hardcore_host.cpp).
//
// Randomness: B2_TERRAIN_RAND3(key0, key1, c, u, r, q) is the keyed Philox call BipedalWalker-v3 makes for point c (same key, tag
// and counter), one call per column: word 0 -> u, a uniform in (-1, 1): the grass law's noise of column c; word 1 -> r (raw) and
// word 2 -> q (raw) are used at an obstacle's first column only: kind = q % 3 (0 stump, 1 pit, 2 stairs), size = (q / 3) & 1 (stump
// 1 + size columns, pit opening 2 + size columns, stairs 3 + size treads), stairs go up if (q / 6) & 1 else down, and 5 + r % 5 is
// the length of the grass stretch that follows the obstacle.
#pragma once
#include "ses_walker_env.h"

namespace b2l {

constexpr int BWH_COLS = BW_TERRAIN_LENGTH - 1;      // 199 spans between the 200 grid abscissae
constexpr int BWH_LAST_OBSTACLE_START = 180;         // the widest obstacle (4 treads) is 16 columns: it ends at column 196 at the latest
constexpr int BWH_PIT_DEPTH = 4;                     // in units of TERRAIN_STEP
constexpr int BWH_STAIR_WIDTH = 4;                   // columns per tread
constexpr int BWH_MAX_EDGES = 2 * BW_TERRAIN_LENGTH; // 199 spans + at most 198 risers, rounded up
// one terrain row: yl[199], yr[199] (float), then bytes: nr[200] (nr[c] = risers at x_0 .. x_c: span c is edge c + nr[c]; nr[199]
// repeats nr[198]) and ecol[400] (edge k is the span of column ecol[k], or the riser on that column's left boundary)
constexpr int BWH_ROW_BYTES = 2 * BWH_COLS * 4 + BW_TERRAIN_LENGTH + BWH_MAX_EDGES;
constexpr int BWH_ROW = BWH_ROW_BYTES / 4;           // 548 floats = 2192 bytes
static_assert(BWH_ROW * 4 == BWH_ROW_BYTES, "a terrain row is a whole number of floats");
// what a column is, for the tests (the device never asks)
constexpr int BWH_KIND_GROUND = 0, BWH_KIND_STUMP = 1, BWH_KIND_PIT_FLOOR = 2, BWH_KIND_TREAD = 3;

struct WalkerHardcoreDef : WalkerDef {
    static constexpr int NSLOT = 8;                  // 4 spans + 3 risers under a leg lying flat (see above)
};
using WalkerHardcoreEnv = WalkerEnvT<WalkerHardcoreDef>;

struct HardcoreTerrain {
    const float *row;                                // BWH_ROW floats (see BWH_ROW_BYTES)
    B2_FN_MEMBER const uint8_t *bytes() const { return (const uint8_t *)(row + 2 * BWH_COLS); }
    B2_FN_MEMBER int n_edges() const { return BWH_COLS + (int)bytes()[BWH_COLS - 1]; }
    B2_FN_MEMBER int index_of(float x) const
    {
        const int c = (int)B2_FLOOR(x / BW_TERRAIN_STEP);
        if (c < 0) return -1;
        if (c >= BWH_COLS) return n_edges();
        return c + (int)bytes()[c];
    }
    B2_FN_MEMBER void edge(int k, float &x1, float &y1, float &x2, float &y2) const
    {
        const uint8_t *n = bytes();
        const int c = (int)n[BW_TERRAIN_LENGTH + k];
        if (k == c + (int)n[c]) {                    // the span of column c
            x1 = (float)c * BW_TERRAIN_STEP; y1 = row[c];
            x2 = (float)(c + 1) * BW_TERRAIN_STEP; y2 = row[BWH_COLS + c];
        } else {                                     // the riser at x_c (c >= 1): from the previous span's right end to this span's left
            x1 = (float)c * BW_TERRAIN_STEP; y1 = row[BWH_COLS + c - 1];
            x2 = x1; y2 = row[c];
        }
    }
};

// the edge index of a row whose heights are written: a riser wherever two neighbouring spans do not meet
B2_FN void hardcore_terrain_index(float *row)
{
    const float *yl = row, *yr = row + BWH_COLS;
    uint8_t *nr = (uint8_t *)(row + 2 * BWH_COLS), *ecol = nr + BW_TERRAIN_LENGTH;
    int ne = 0, risers = 0;
    for (int c = 0; c < BWH_COLS; ++c) {
        if (c > 0 && yr[c - 1] != yl[c]) { ecol[ne++] = (uint8_t)c; ++risers; }
        ecol[ne++] = (uint8_t)c;
        nr[c] = (uint8_t)risers;
    }
    nr[BWH_COLS] = (uint8_t)risers;
    for (; ne < BWH_MAX_EDGES; ++ne) ecol[ne] = 0;   // ne <= 199 + 198
}

// The terrain of one episode.  Columns 0 .. 19: the flat start pad at TERRAIN_HEIGHT.  From column 20 on an obstacle and a grass
// stretch of 5 .. 9 columns alternate, the first obstacle at column 20; no obstacle starts after column BWH_LAST_OBSTACLE_START.
// The grass law is walker_terrain_heights': velocity = 0.8 velocity + 0.01 sign(TERRAIN_HEIGHT - y) + u / SCALE, y += velocity, one
// step per grass column.  An obstacle stands on the ground height y where it starts:
//   stump  : w = 1 or 2 columns at y + w STEP; the ground stays at y;
//   pit    : a lip column at y, an opening of 2 or 3 columns at y - 4 STEP, a lip column at y;
//   stairs : 3 or 4 treads of 4 columns, tread j at y + j STEP or y - j STEP; grass goes on from the last tread's height.
// kind (may be null): BWH_KIND_* per column, for the tests.
B2_FN void hardcore_terrain_generate(uint32_t key0, uint32_t key1, float *row, uint8_t *kind)
{
    float *yl = row, *yr = row + BWH_COLS;
    float y = BW_TERRAIN_HEIGHT, velocity = 0.0f;
    int c = 0, grass = 0;                            // grass: columns of the current stretch still to come
    for (; c < BW_TERRAIN_STARTPAD; ++c) {
        yl[c] = y; yr[c] = y;
        if (kind) kind[c] = BWH_KIND_GROUND;
    }
    while (c < BWH_COLS) {
        float u;
        uint32_t r, q;
        B2_TERRAIN_RAND3(key0, key1, c, u, r, q);
        if (grass == 0 && c <= BWH_LAST_OBSTACLE_START) {
            const int what = (int)(q % 3u), size = (int)((q / 3u) & 1u);
            const int dir = ((q / 6u) & 1u) ? 1 : -1;
            const int runs = what == 0 ? 1 : (what == 1 ? 3 : 3 + size);       // flat runs of the obstacle
            int off = 0;
            for (int j = 0; j < runs; ++j) {
                int w;
                if (what == 0) { w = 1 + size; off = w; }
                else if (what == 1) { w = j == 1 ? 2 + size : 1; off = j == 1 ? -BWH_PIT_DEPTH : 0; }
                else { w = BWH_STAIR_WIDTH; off = dir * j; }
                const float h = off == 0 ? y : y + (float)off * BW_TERRAIN_STEP;
                for (int i = 0; i < w; ++i, ++c) {                             // c < 180 + 16
                    yl[c] = h; yr[c] = h;
                    if (kind) kind[c] = (uint8_t)(off == 0 ? BWH_KIND_GROUND : (what == 0 ? BWH_KIND_STUMP : (what == 1 ? BWH_KIND_PIT_FLOOR : BWH_KIND_TREAD)));
                }
            }
            if (what == 2 && off != 0) y = y + (float)off * BW_TERRAIN_STEP;   // the last tread's height
            grass = BW_TERRAIN_GRASS / 2 + (int)(r % (uint32_t)(BW_TERRAIN_GRASS - BW_TERRAIN_GRASS / 2));
        } else {
            yl[c] = y;
            const float d = BW_TERRAIN_HEIGHT - y;
            const float sgn = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
            velocity = 0.8f * velocity + 0.01f * sgn;
            velocity += u / BW_SCALE;
            y += velocity;
            yr[c] = y;
            if (kind) kind[c] = BWH_KIND_GROUND;
            ++c;
            grass -= grass > 0 ? 1 : 0;
        }
    }
    hardcore_terrain_index(row);
}

}  // namespace b2l
