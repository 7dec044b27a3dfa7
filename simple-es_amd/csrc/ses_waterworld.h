// ses_waterworld.h -- waterworld: five pursuers in a unit box with five evaders, ten poisons and one round obstacle, the
// build's own float64 definition modelled on pettingzoo's sisl waterworld_v3 with its defaults (DESIGN.md 7 is the
// specification; tests/waterworld_np.py is the independent numpy restatement that every transition is compared with bit
// for bit).  Parity with pettingzoo itself is UNPINNED: pettingzoo is not part of the reference tree.
//
// Arithmetic: the state is float64; every operation is ONE correctly rounded IEEE add, sub, mul, div, sqrt or compare in
// the order written here (the ses_classic.h rule).  No fma anywhere (the build passes -ffp-contract=off; numpy cannot
// restate one).  Observations are cast to float32 at the end.
//
// Objects 0..4 are the pursuers, 5..9 the evaders, 10..19 the poisons.  Init row (WW_INIT_W = 72 floats in U(0, 1)):
// pursuer (x, y) x 5 | evader (x, y, u, v) x 5 | poison (x, y, u, v) x 10 | two key words (their bit patterns, as
// BipedalWalker's terrain key).  (u, v) gives a direction: d = (u - 0.5, v - 0.5), velocity (d / |d|) * speed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ses {

constexpr int WW_NP = 5, WW_NE = 5, WW_NPO = 10, WW_NOBJ = WW_NP + WW_NE + WW_NPO;
constexpr int WW_SENSORS = 30, WW_OBS = 8 * WW_SENSORS + 2, WW_INIT_W = 72, WW_MAX_CYCLES = 500;
constexpr double WW_R = 0.015;                    // pursuer radius
constexpr double WW_R_EV = 2.0 * WW_R;            // evader radius
constexpr double WW_R_PO = 0.75 * WW_R;           // poison radius
constexpr double WW_R_OB = 0.2;                   // the obstacle, centred at (0.5, 0.5)
constexpr double WW_SPEED = 0.01;                 // evaders and poisons
constexpr double WW_MAX_ACCEL = 0.01;
constexpr double WW_L = 0.2;                      // sensor range
constexpr double WW_TOUCH_EV = (3.0 * WW_R) * (3.0 * WW_R);          // squared centre distance pursuer - evader
constexpr double WW_TOUCH_PO = (1.75 * WW_R) * (1.75 * WW_R);        // ... pursuer - poison
constexpr double WW_FOOD = 10.0, WW_ENCOUNTER = 0.01, WW_POISON = -1.0, WW_THRUST = -0.5;
constexpr float WW_ACTION_SCALE = 0.001f;         // the reference wrapper's in-place `act *= 0.001` on a float32 array
constexpr uint32_t WW_PHILOX_TAG = 0x57415452u;   // counter word 3 of a respawn draw

// sensor k looks along (cos, sin)(k * (6.283185307179586 / 30.0)).  THE TABLE IS THE DEFINITION: nothing calls cos at run time
// (tests/test_waterworld_host.py compares these literals with the restatement's, and both with numpy's cos / sin).
// WW_SENSOR_TABLE_BEGIN
__device__ const double WW_SENSOR_DIR[WW_SENSORS][2] = {
    {0x1.0000000000000p+0, 0x0.0p+0},
    {0x1.f4cfc327a0080p-1, 0x1.a9cd9ac4258f5p-3},
    {0x1.d3bc3aeff7f95p-1, 0x1.a07f921061ad0p-2},
    {0x1.9e3779b97f4a8p-1, 0x1.2cf2304755a5ep-1},
    {0x1.5698496e20bd8p-1, 0x1.7c7d7a833bec1p-1},
    {0x1.0000000000001p-1, 0x1.bb67ae8584caap-1},
    {0x1.3c6ef372fe950p-2, 0x1.e6f0e134454ffp-1},
    {0x1.ac2609b3c577bp-4, 0x1.fd31f94f867c6p-1},
    {-0x1.ac2609b3c5762p-4, 0x1.fd31f94f867c7p-1},
    {-0x1.3c6ef372fe94ep-2, 0x1.e6f0e13445500p-1},
    {-0x1.ffffffffffffcp-2, 0x1.bb67ae8584cabp-1},
    {-0x1.5698496e20bd5p-1, 0x1.7c7d7a833bec4p-1},
    {-0x1.9e3779b97f4a7p-1, 0x1.2cf2304755a5fp-1},
    {-0x1.d3bc3aeff7f94p-1, 0x1.a07f921061ad5p-2},
    {-0x1.f4cfc327a007fp-1, 0x1.a9cd9ac425904p-3},
    {-0x1.0000000000000p+0, 0x1.1a62633145c07p-53},
    {-0x1.f4cfc327a0080p-1, -0x1.a9cd9ac4258ecp-3},
    {-0x1.d3bc3aeff7f97p-1, -0x1.a07f921061acap-2},
    {-0x1.9e3779b97f4a9p-1, -0x1.2cf2304755a5dp-1},
    {-0x1.5698496e20bdap-1, -0x1.7c7d7a833bec0p-1},
    {-0x1.0000000000004p-1, -0x1.bb67ae8584ca8p-1},
    {-0x1.3c6ef372fe952p-2, -0x1.e6f0e134454ffp-1},
    {-0x1.ac2609b3c57a3p-4, -0x1.fd31f94f867c6p-1},
    {0x1.ac2609b3c5749p-4, -0x1.fd31f94f867c7p-1},
    {0x1.3c6ef372fe94cp-2, -0x1.e6f0e13445500p-1},
    {0x1.ffffffffffff4p-2, -0x1.bb67ae8584caep-1},
    {0x1.5698496e20bd4p-1, -0x1.7c7d7a833bec5p-1},
    {0x1.9e3779b97f4a7p-1, -0x1.2cf2304755a60p-1},
    {0x1.d3bc3aeff7f92p-1, -0x1.a07f921061adep-2},
    {0x1.f4cfc327a007fp-1, -0x1.a9cd9ac425909p-3},
};
// WW_SENSOR_TABLE_END

struct WaterState {
    double px[WW_NOBJ], py[WW_NOBJ], vx[WW_NOBJ], vy[WW_NOBJ];
    uint32_t key0, key1, ctr;                     // respawn stream: Philox key, draws made so far
    int32_t touch_ev[WW_NP], touch_po[WW_NP];     // obs[240], obs[241] of each pursuer: touched an evader / a poison this cycle
};

__device__ __forceinline__ double ww_radius(int i) { return i < WW_NP ? WW_R : (i < WW_NP + WW_NE ? WW_R_EV : WW_R_PO); }

// Philox4x32-10 (Salmon et al., SC'11) on a raw counter and key
__device__ __forceinline__ void ww_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4])
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t m0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t m1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(m1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)m1;
        const uint32_t n2 = (uint32_t)(m0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)m0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// true when a centre at (x, y) of an object of radius rho lies clear of the obstacle
__device__ __forceinline__ bool ww_clear_of_obstacle(double x, double y, double rho)
{
    const double dx = x - 0.5, dy = y - 0.5, lim = WW_R_OB + rho;
    return dx * dx + dy * dy > lim * lim;
}

__device__ __forceinline__ void ww_direction(double u, double v, double speed, double &ox, double &oy)
{
    const double dx = u - 0.5, dy = v - 0.5;
    const double n = __dsqrt_rn(dx * dx + dy * dy);
    if (n == 0.0) {
        ox = speed;
        oy = 0.0;
    } else {
        ox = (dx / n) * speed;
        oy = (dy / n) * speed;
    }
}

// object i gets a new place (and, unless it is a pursuer, a new heading): up to eight draws of the env's own stream
__device__ __forceinline__ void ww_respawn(WaterState &s, int i)
{
    const double rho = ww_radius(i);
    double u[4] = {0.0, 0.0, 0.0, 0.0};
    bool ok = false;
    for (uint32_t t = 0; t < 8u && !ok; ++t) {
        uint32_t w[4];
        ww_philox(s.ctr, t, 0u, WW_PHILOX_TAG, s.key0, s.key1, w);
        for (int q = 0; q < 4; ++q) u[q] = (double)(w[q] >> 8) * 0x1.0p-24;
        ok = ww_clear_of_obstacle(u[0], u[1], rho);
    }
    s.px[i] = ok ? u[0] : u[0] * 0.25;
    s.py[i] = ok ? u[1] : u[1] * 0.25;
    if (i >= WW_NP) ww_direction(u[2], u[3], WW_SPEED, s.vx[i], s.vy[i]);
    s.ctr += 1u;
}

__device__ __forceinline__ void ww_reset(WaterState &s, const float *__restrict__ u)
{
    for (int a = 0; a < WW_NP; ++a) {
        s.px[a] = (double)u[2 * a];
        s.py[a] = (double)u[2 * a + 1];
        s.vx[a] = 0.0;
        s.vy[a] = 0.0;
        s.touch_ev[a] = 0;
        s.touch_po[a] = 0;
    }
    for (int i = WW_NP; i < WW_NOBJ; ++i) {
        const float *o = u + 2 * WW_NP + 4 * (i - WW_NP);
        s.px[i] = (double)o[0];
        s.py[i] = (double)o[1];
        ww_direction((double)o[2], (double)o[3], WW_SPEED, s.vx[i], s.vy[i]);
    }
    s.key0 = __builtin_bit_cast(uint32_t, u[70]);
    s.key1 = __builtin_bit_cast(uint32_t, u[71]);
    s.ctr = 0u;
    for (int i = 0; i < WW_NOBJ; ++i)
        if (!ww_clear_of_obstacle(s.px[i], s.py[i], ww_radius(i))) ww_respawn(s, i);
}

// an object that has entered the obstacle is pushed along its offset from the centre and its velocity mirrored at it
__device__ __forceinline__ void ww_rebound(WaterState &s, int i, double rho)
{
    const double dx = s.px[i] - 0.5, dy = s.py[i] - 0.5;
    const double dist = __dsqrt_rn(dx * dx + dy * dy);
    const double lim = rho + WW_R_OB;
    if (dist <= lim) {
        const double scale = lim - dist;
        s.px[i] = s.px[i] + scale * dx;
        s.py[i] = s.py[i] + scale * dy;
        const double nx = s.px[i] - 0.5, ny = s.py[i] - 0.5;
        const double k = (s.vx[i] * nx + s.vy[i] * ny) / (nx * nx + ny * ny);
        const double projx = k * nx, projy = k * ny;
        const double perpx = s.vx[i] - projx, perpy = s.vy[i] - projy;
        s.vx[i] = perpx - projx;
        s.vy[i] = perpy - projy;
    }
}

// One cycle is three phases, each a function of its own so that the fused rollout can spread the first two over lanes
// (the step-wise env and ww_step run them in index order; no object's move reads another object):
//   ww_move_pursuer / ww_move_drifter : an object's move, walls and obstacle
//   ww_touches                        : whom a pursuer touches in the new positions
//   ww_settle                         : catches, rewards, touch flags, respawns
// (ax, ay): the pursuer's two float32 actions ALREADY multiplied by WW_ACTION_SCALE.  Returns the thrust term of its reward.
__device__ __forceinline__ double ww_move_pursuer(WaterState &s, int a, float actx, float acty)
{
    double ax = (double)actx, ay = (double)acty;
    double m = __dsqrt_rn(ax * ax + ay * ay);
    if (m > WW_MAX_ACCEL) {
        ax = (ax / m) * WW_MAX_ACCEL;
        ay = (ay / m) * WW_MAX_ACCEL;
        m = __dsqrt_rn(ax * ax + ay * ay);
    }
    s.vx[a] = s.vx[a] + ax;
    s.vy[a] = s.vy[a] + ay;
    s.px[a] = s.px[a] + s.vx[a];
    s.py[a] = s.py[a] + s.vy[a];
    if (s.px[a] < 0.0) { s.px[a] = 0.0; s.vx[a] = 0.0; } else if (s.px[a] > 1.0) { s.px[a] = 1.0; s.vx[a] = 0.0; }
    if (s.py[a] < 0.0) { s.py[a] = 0.0; s.vy[a] = 0.0; } else if (s.py[a] > 1.0) { s.py[a] = 1.0; s.vy[a] = 0.0; }
    ww_rebound(s, a, WW_R);
    return WW_THRUST * m;
}

// an evader or a poison
__device__ __forceinline__ void ww_move_drifter(WaterState &s, int i)
{
    s.px[i] = s.px[i] + s.vx[i];
    s.py[i] = s.py[i] + s.vy[i];
    if (s.px[i] >= 1.0) { s.px[i] = 1.0; s.vx[i] = -s.vx[i]; } else if (s.px[i] <= 0.0) { s.px[i] = 0.0; s.vx[i] = -s.vx[i]; }
    if (s.py[i] >= 1.0) { s.py[i] = 1.0; s.vy[i] = -s.vy[i]; } else if (s.py[i] <= 0.0) { s.py[i] = 0.0; s.vy[i] = -s.vy[i]; }
    ww_rebound(s, i, ww_radius(i));
}

// touches, on squared distances: bit e of ev = pursuer a touches evader e, bit j of po likewise for poison j
__device__ __forceinline__ void ww_touches(const WaterState &s, int a, uint32_t &ev, uint32_t &po)
{
    ev = 0u;
    po = 0u;
    for (int j = 0; j < WW_NE + WW_NPO; ++j) {
        const int i = WW_NP + j;
        const double dx = s.px[a] - s.px[i], dy = s.py[a] - s.py[i];
        const double d2 = dx * dx + dy * dy;
        if (j < WW_NE) ev |= d2 <= WW_TOUCH_EV ? 1u << j : 0u;
        else po |= d2 <= WW_TOUCH_PO ? 1u << (j - WW_NE) : 0u;
    }
}

// the team reward of the cycle; sets the touch flags and respawns what was caught or touched
__device__ __forceinline__ double ww_settle(WaterState &s, const double (&thrust)[WW_NP], const uint32_t (&ev)[WW_NP],
                                            const uint32_t (&po)[WW_NP])
{
    uint32_t caught = 0u, poisoned = 0u;
    for (int e = 0; e < WW_NE; ++e) {
        int n = 0;
        for (int a = 0; a < WW_NP; ++a) n += (int)((ev[a] >> e) & 1u);
        if (n >= 2) caught |= 1u << e;
    }
    double reward = 0.0;
    for (int a = 0; a < WW_NP; ++a) {
        const int nc = __builtin_popcount(ev[a] & caught), ne = __builtin_popcount(ev[a]), np = __builtin_popcount(po[a]);
        const double r = ((thrust[a] + WW_FOOD * (double)nc) + WW_ENCOUNTER * (double)ne) + WW_POISON * (double)np;
        reward = a == 0 ? r : reward + r;
        poisoned |= po[a];
        s.touch_ev[a] = ne > 0 ? 1 : 0;
        s.touch_po[a] = np > 0 ? 1 : 0;
    }
    for (int e = 0; e < WW_NE; ++e)
        if ((caught >> e) & 1u) ww_respawn(s, WW_NP + e);
    for (int j = 0; j < WW_NPO; ++j)
        if ((poisoned >> j) & 1u) ww_respawn(s, WW_NP + WW_NE + j);
    return reward;
}

// One cycle: act[a] = pursuer a's two float32 actions, ALREADY multiplied by WW_ACTION_SCALE.  Returns the team reward.
__device__ __forceinline__ double ww_step(WaterState &s, const float (&act)[WW_NP][2])
{
    double thrust[WW_NP];
    uint32_t ev[WW_NP], po[WW_NP];
    for (int a = 0; a < WW_NP; ++a) thrust[a] = ww_move_pursuer(s, a, act[a][0], act[a][1]);
    for (int i = WW_NP; i < WW_NOBJ; ++i) ww_move_drifter(s, i);
    for (int a = 0; a < WW_NP; ++a) ww_touches(s, a, ev[a], po[a]);
    return ww_settle(s, thrust, ev, po);
}

__device__ __forceinline__ double ww_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double ww_clip01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }

// bit i set: a sensor of pursuer a may see object i.  Seeing needs 0 <= proj <= L + rho and |rel|^2 - proj^2 <= rho^2, so
// |rel|^2 <= (L + rho)^2 + rho^2, which lies below the (L + 2 rho)^2 tested here by 2 rho (L + rho) > 4e-3: thirteen decimal
// orders above any rounding of these sums.  The filter therefore drops no object a sensor sees; it changes no result.
__device__ __forceinline__ uint32_t ww_candidates(const WaterState &s, int a)
{
    uint32_t m = 0u;
    for (int i = 0; i < WW_NOBJ; ++i) {
        const double relx = s.px[i] - s.px[a], rely = s.py[i] - s.py[a];
        const double lim = WW_L + 2.0 * ww_radius(i);
        if (i != a && relx * relx + rely * rely <= lim * lim) m |= 1u << i;
    }
    return m;
}

// the nearest object among the candidates `cand` (one class: equal radii rho; ascending index) that sensor (skx, sky) of
// pursuer a sees: its distance feature and its speed along the sensor relative to the pursuer; (1, 0) when it sees none.
// A tie goes to the lower index.
__device__ __forceinline__ void ww_sense_class(const WaterState &s, int a, double skx, double sky, uint32_t cand, double rho,
                                               double &dist_out, double &speed_out)
{
    const double cx = s.px[a], cy = s.py[a];
    double best = 0.0;
    int who = -1;
    while (cand) {
        const int i = __builtin_ctz(cand);
        cand &= cand - 1u;
        const double relx = s.px[i] - cx, rely = s.py[i] - cy;
        const double proj = skx * relx + sky * rely;
        const bool seen = proj >= 0.0 && proj - rho <= WW_L && (relx * relx + rely * rely) - proj * proj <= rho * rho;
        if (seen && (who < 0 || proj < best)) {
            best = proj;
            who = i;
        }
    }
    if (who < 0) {
        dist_out = 1.0;
        speed_out = 0.0;
    } else {
        dist_out = ww_min(best / WW_L, 1.0);
        speed_out = skx * (s.vx[who] - s.vx[a]) + sky * (s.vy[who] - s.vy[a]);
    }
}

// the 8 features of sensor k of pursuer a: obs[8 k .. 8 k + 7]; cand = ww_candidates(s, a)
__device__ __forceinline__ void ww_sensor(const WaterState &s, int a, int k, uint32_t cand, float (&f)[8])
{
    const double skx = WW_SENSOR_DIR[k][0], sky = WW_SENSOR_DIR[k][1];
    const double cx = s.px[a], cy = s.py[a];
    // the obstacle
    double ob = 1.0;
    {
        const double relx = 0.5 - cx, rely = 0.5 - cy;
        const double proj = skx * relx + sky * rely;
        if (proj >= 0.0 && proj - WW_R_OB <= WW_L && (relx * relx + rely * rely) - proj * proj <= WW_R_OB * WW_R_OB)
            ob = ww_min(proj / WW_L, 1.0);
    }
    // the walls
    const double lx = skx * WW_L, ly = sky * WW_L;
    const double vecx = ww_clip01(cx + lx) - cx, vecy = ww_clip01(cy + ly) - cy;
    const double ratx = __builtin_fabs(lx) > 1e-8 ? vecx / lx : 1.0;
    const double raty = __builtin_fabs(ly) > 1e-8 ? vecy / ly : 1.0;
    const double barrier = ww_clip01(ww_min(ratx, raty));
    double ed, es, pd, ps, ud, us;
    ww_sense_class(s, a, skx, sky, cand & (((1u << WW_NE) - 1u) << WW_NP), WW_R_EV, ed, es);
    ww_sense_class(s, a, skx, sky, cand & (((1u << WW_NPO) - 1u) << (WW_NP + WW_NE)), WW_R_PO, pd, ps);
    ww_sense_class(s, a, skx, sky, cand & ((1u << WW_NP) - 1u), WW_R, ud, us);
    f[0] = (float)ob; f[1] = (float)barrier; f[2] = (float)ed; f[3] = (float)es;
    f[4] = (float)pd; f[5] = (float)ps; f[6] = (float)ud; f[7] = (float)us;
}

}  // namespace ses
