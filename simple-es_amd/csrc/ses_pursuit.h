// ses_pursuit.h -- pursuit: eight pursuers on a 16 x 16 grid hunt thirty randomly moving evaders round one rectangular block,
// the build's own integer definition modelled on pettingzoo's sisl pursuit_v3 with its defaults (DESIGN.md 7 is the
// specification; tests/pursuit_np.py is the independent numpy restatement that every transition is compared with bit for
// bit).  Parity with pettingzoo itself is UNPINNED: pettingzoo is not part of the reference tree.
//
// Arithmetic: the state is small integers; the only floating point of the env is the reward, float64, one correctly rounded
// IEEE operation at a time in the order written here (no fma: the build passes -ffp-contract=off), and the observation's counts
// cast to float32 (exact).
//
// Init row (PU_INIT_W = 40 floats in U(0, 1)): pursuer cells x 8 | evader cells x 30 | two key words of the evader-move stream
// (their bit patterns, as BipedalWalker's terrain key).  Cell = PU_FREE[clamp((int)(u * 193.0f), 0, 192)] of the 193 free cells
// in ascending (x, y) order; an evader whose entry is negative does not exist.  Several actors may share a cell.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ses_rng.h"

namespace ses {

constexpr int PU_GRID = 16, PU_NP = 8, PU_NE = 30, PU_RANGE = 7, PU_OBS = PU_RANGE * PU_RANGE * 3, PU_INIT_W = 40;
constexpr int PU_MAX_CYCLES = 500, PU_NFREE = 193, PU_NQUAD = (PU_NE + 3) / 4;
constexpr int PU_BLOCK_X0 = 5, PU_BLOCK_X1 = 11, PU_BLOCK_Y0 = 4, PU_BLOCK_Y1 = 12;   // the obstacle block, bounds inclusive
constexpr double PU_TAG = 0.01, PU_CATCH = 5.0, PU_URGENCY = -0.1;
constexpr uint64_t TAG_PURSUIT_MOVES = 2ull;      // stream tag of the evader moves (ses_rng.h: 0 = parameter noise, 1 = env init)
constexpr uint32_t PU_ALL_EVADERS = (1u << PU_NE) - 1u;

struct PursuitState {
    uint8_t px[PU_NP], py[PU_NP];                 // the pursuers' cells
    uint8_t ex[32], ey[32];                       // the evaders' cells (30 used)
    uint32_t alive;                               // bit e: evader e exists and is not caught yet
    uint32_t key0, key1, cycle;                   // evader-move stream: Philox key, cycles played
};

__device__ __forceinline__ bool pu_on_grid(int x, int y) { return (unsigned)x < (unsigned)PU_GRID && (unsigned)y < (unsigned)PU_GRID; }
__device__ __forceinline__ bool pu_in_block(int x, int y)
{
    return x >= PU_BLOCK_X0 && x <= PU_BLOCK_X1 && y >= PU_BLOCK_Y0 && y <= PU_BLOCK_Y1;
}
__device__ __forceinline__ bool pu_free(int x, int y) { return pu_on_grid(x, y) && !pu_in_block(x, y); }

// the 193 free cells in ascending (x, y) order, a cell as x * 16 + y
struct PursuitFreeTable {
    uint8_t cell[PU_NFREE];
};
constexpr PursuitFreeTable pu_make_free_table()
{
    PursuitFreeTable t{};
    int n = 0;
    for (int x = 0; x < PU_GRID; ++x)
        for (int y = 0; y < PU_GRID; ++y)
            if (!(x >= PU_BLOCK_X0 && x <= PU_BLOCK_X1 && y >= PU_BLOCK_Y0 && y <= PU_BLOCK_Y1)) t.cell[n++] = (uint8_t)(x * PU_GRID + y);
    return t;
}
static_assert(PU_GRID * PU_GRID - (PU_BLOCK_X1 - PU_BLOCK_X0 + 1) * (PU_BLOCK_Y1 - PU_BLOCK_Y0 + 1) == PU_NFREE, "193 free cells");
__device__ const PursuitFreeTable PU_FREE = pu_make_free_table();

__device__ __forceinline__ void pu_free_cell(int i, int &x, int &y)
{
    const int c = PU_FREE.cell[i];
    x = c / PU_GRID;
    y = c % PU_GRID;
}

// the cell an init entry names; any float is answered with a cell of the table (NaN and negatives with cell 0)
__device__ __forceinline__ int pu_cell_index(float u)
{
    const float v = u * 193.0f;
    return !(v >= 0.0f) ? 0 : (v >= 192.0f ? 192 : (int)v);
}

__device__ __forceinline__ void pu_reset(PursuitState &s, const float *__restrict__ u)
{
    for (int i = 0; i < PU_NP; ++i) {
        int x, y;
        pu_free_cell(pu_cell_index(u[i]), x, y);
        s.px[i] = (uint8_t)x;
        s.py[i] = (uint8_t)y;
    }
    s.alive = 0u;
    for (int e = 0; e < 32; ++e) {
        int x = 0, y = 0;
        if (e < PU_NE) {
            const float v = u[PU_NP + e];
            pu_free_cell(pu_cell_index(v), x, y);
            if (!(v < 0.0f)) s.alive |= 1u << e;
        }
        s.ex[e] = (uint8_t)x;
        s.ey[e] = (uint8_t)y;
    }
    s.key0 = __builtin_bit_cast(uint32_t, u[PU_NP + PU_NE]);
    s.key1 = __builtin_bit_cast(uint32_t, u[PU_NP + PU_NE + 1]);
    s.cycle = 0u;
}

// move m from (x, y): 0 = (-1, 0), 1 = (+1, 0), 2 = (0, +1), 3 = (0, -1), anything else stays; a move off the grid or into the
// block stays
__device__ __forceinline__ void pu_move(uint8_t &x, uint8_t &y, int m)
{
    const int nx = (int)x + (m == 1 ? 1 : (m == 0 ? -1 : 0));
    const int ny = (int)y + (m == 2 ? 1 : (m == 3 ? -1 : 0));
    if (pu_free(nx, ny)) {
        x = (uint8_t)nx;
        y = (uint8_t)ny;
    }
}

// the moves of evaders 4 q .. 4 q + 3 in cycle s.cycle.  A cycle has ONE Philox draw, counter (0, 0, cycle, tag), key (key0, key1);
// evader e's move is base-5 digit e & 7 of word e >> 3: (word / 5^(e & 7)) mod 5.  A removed evader does not move, and nobody's
// digit depends on who is removed.  No evader's move reads another actor, so the quads may run in any order or side by side.
__device__ __forceinline__ void pu_move_evaders(PursuitState &s, int q)
{
    if (((s.alive >> (4 * q)) & 0xFu) == 0u) return;
    const uint4 w = philox_words((uint64_t)s.key0 | ((uint64_t)s.key1 << 32), TAG_PURSUIT_MOVES, (uint64_t)s.cycle, 0u, 0u);
    uint32_t v = (q >> 1) == 0 ? w.x : ((q >> 1) == 1 ? w.y : ((q >> 1) == 2 ? w.z : w.w));
    if (q & 1) v /= 625u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = 4 * q + j;
        const int m = (int)(v % 5u);
        v /= 5u;
        if (e < PU_NE && ((s.alive >> e) & 1u)) pu_move(s.ex[e], s.ey[e], m);
    }
}

__device__ __forceinline__ bool pu_pursuer_at(const PursuitState &s, int x, int y)
{
    bool any = false;
#pragma unroll
    for (int i = 0; i < PU_NP; ++i) any |= (int)s.px[i] == x && (int)s.py[i] == y;
    return any;
}

// evader e (alive) is caught: every one of its four neighbour cells that is on the grid and free holds a pursuer
__device__ __forceinline__ bool pu_caught(const PursuitState &s, int e)
{
    const int x = s.ex[e], y = s.ey[e];
    bool caught = true;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int nx = x + (d == 0 ? -1 : (d == 1 ? 1 : 0)), ny = y + (d == 2 ? 1 : (d == 3 ? -1 : 0));
        if (pu_free(nx, ny)) caught &= pu_pursuer_at(s, nx, ny);
    }
    return caught;
}

// pursuer i's own reward of the cycle before the team mean: alive = the evaders alive before this cycle's removals, caught = those
// of them caught in it
__device__ __forceinline__ double pu_pursuer_reward(const PursuitState &s, int i, uint32_t alive, uint32_t caught)
{
    const int x = s.px[i], y = s.py[i];
    int n_tag = 0, n_catch = 0;
    for (int e = 0; e < PU_NE; ++e) {
        const int dx = (int)s.ex[e] - x, dy = (int)s.ey[e] - y;
        const int dist = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
        n_tag += (int)((alive >> e) & 1u) & (int)(dist <= 1);
        n_catch += (int)((caught >> e) & 1u) & (int)(dist == 1);
    }
    return (PU_TAG * (double)n_tag + PU_CATCH * (double)n_catch) + PU_URGENCY;
}

// shared_reward: every pursuer gets the mean of the eight; the team reward is the sum of those eight equal shares
__device__ __forceinline__ double pu_team_reward(const double (&r)[PU_NP])
{
    double sum = r[0];
#pragma unroll
    for (int i = 1; i < PU_NP; ++i) sum = sum + r[i];
    const double mean = sum / 8.0;
    double team = mean;
#pragma unroll
    for (int i = 1; i < PU_NP; ++i) team = team + mean;
    return team;
}

// removes the caught, counts the cycle; true when no evader is left
__device__ __forceinline__ bool pu_settle(PursuitState &s, uint32_t caught)
{
    s.alive &= ~caught;
    s.cycle += 1u;
    return s.alive == 0u;
}

// One cycle with one lane for the whole env: action[i] = pursuer i's move.  Returns the team reward; done = no evader is left.
__device__ __forceinline__ double pu_step(PursuitState &s, const int32_t (&action)[PU_NP], bool &done)
{
    for (int i = 0; i < PU_NP; ++i) pu_move(s.px[i], s.py[i], action[i]);
    for (int q = 0; q < PU_NQUAD; ++q) pu_move_evaders(s, q);
    uint32_t caught = 0u;
    for (int e = 0; e < PU_NE; ++e)
        if (((s.alive >> e) & 1u) && pu_caught(s, e)) caught |= 1u << e;
    double r[PU_NP];
    for (int i = 0; i < PU_NP; ++i) r[i] = pu_pursuer_reward(s, i, s.alive, caught);
    const double team = pu_team_reward(r);
    done = pu_settle(s, caught);
    return team;
}

// observation component (dx, dy) of a pursuer at (x, y): the cell it looks at and whether it is a wall (off the grid or in the block)
__device__ __forceinline__ bool pu_window_cell(int x, int y, int dx, int dy, int &cx, int &cy)
{
    cx = x - PU_RANGE / 2 + dx;
    cy = y - PU_RANGE / 2 + dy;
    return !pu_free(cx, cy);
}

// pursuer i's 147 observations, written by one lane: [dx][dy][wall, pursuers in the cell (itself included), live evaders in it]
__device__ __forceinline__ void pu_observe(const PursuitState &s, int i, float *__restrict__ o)
{
    const int x = s.px[i], y = s.py[i];
    for (int c = 0; c < PU_RANGE * PU_RANGE; ++c) {
        int cx, cy;
        o[3 * c] = pu_window_cell(x, y, c / PU_RANGE, c % PU_RANGE, cx, cy) ? 1.0f : 0.0f;
        o[3 * c + 1] = 0.0f;
        o[3 * c + 2] = 0.0f;
    }
    for (int j = 0; j < PU_NP + PU_NE; ++j) {
        const bool evader = j >= PU_NP;
        if (evader && !((s.alive >> (j - PU_NP)) & 1u)) continue;
        const int dx = (int)(evader ? s.ex[j - PU_NP] : s.px[j]) - x + PU_RANGE / 2;
        const int dy = (int)(evader ? s.ey[j - PU_NP] : s.py[j]) - y + PU_RANGE / 2;
        if ((unsigned)dx < (unsigned)PU_RANGE && (unsigned)dy < (unsigned)PU_RANGE) o[3 * (dx * PU_RANGE + dy) + (evader ? 2 : 1)] += 1.0f;
    }
}

}  // namespace ses
