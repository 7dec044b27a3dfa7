// walker2d_host.cpp -- TEST INFRASTRUCTURE.  Host build of Walker2DBulletEnv-v0 (simple-es_amd/csrc/ses_walker2d_env.h on the Box2D-style
// world of ses_b2.h) with C entry points for tests/walker2d_host.py.  The B2_* macros are the host's, as oracle/ses_b2_oracle.cpp
// defines them; o_sincosf and o_f2u come from the oracle's library (oracle/ses_oracle_math.h).
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

#include "ses_walker2d_env.h"

using namespace b2l;

extern "C" {

int w2d_state_size(void) { return (int)sizeof(Walker2dEnv); }

void w2d_obs(const void *state, float *obs)
{
    float o[22];
    walker2d_obs(*(const Walker2dEnv *)state, o);
    memcpy(obs, o, sizeof o);
}

void w2d_reset(void *state, const float *u6, float *obs)
{
    Walker2dEnv *e = (Walker2dEnv *)state;
    memset(e, 0, sizeof *e);
    walker2d_reset(*e, u6);
    if (obs) w2d_obs(state, obs);
}

// one env step; terms4 (may be null): the alive, progress, electricity and joints-at-limit terms whose sum is the reward
float w2d_step(void *state, const float *action6, float *obs, int32_t *done, float *terms4)
{
    Walker2dEnv *e = (Walker2dEnv *)state;
    float a[6];
    memcpy(a, action6, sizeof a);
    bool d;
    const float r = walker2d_step(*e, a, d, terms4);
    if (obs) w2d_obs(state, obs);
    *done = d ? 1 : 0;
    return r;
}

// one WORLD step (a quarter of an env step) with whatever motor settings the joints carry
void w2d_world_step(void *state)
{
    Walker2dEnv *e = (Walker2dEnv *)state;
    const Walker2dTerrain terr{};
    world_step(e->w, terr, W2D_DT);
}

// bodies [7][6] = (cx, cy, angle, vx, vy, omega) of torso, thigh, leg, foot, thigh_left, leg_left, foot_left
void w2d_set_bodies(void *state, const float *bodies)
{
    Walker2dEnv *e = (Walker2dEnv *)state;
    for (int b = 0; b < 7; ++b) {
        Body &B = e->w.body[b];
        const float *v = bodies + 6 * b;
        B.cx = v[0]; B.cy = v[1]; B.a = v[2]; B.vx = v[3]; B.vy = v[4]; B.w = v[5];
    }
}

// the float32 world's tables for the seven bodies: props[7][4] = mass, inertia about the centre of mass, half width, half height of the box
void w2d_body_props(float *props)
{
    for (int b = 0; b < 7; ++b) {
        const float v[4] = {1.0f / WALKER2D_BODY[b].inv_mass, 1.0f / WALKER2D_BODY[b].inv_i, WALKER2D_POLY[b].vx[1], WALKER2D_POLY[b].vy[2]};
        memcpy(props + 4 * b, v, sizeof v);
    }
}

// diagnostics: bodies [7][6]; masses [7]; sep [6] = distance between the two bodies' images of each joint's anchor; angles [6];
// limits [6][2]; floats = {lowest vertex height over the solved bodies (all but the torso), lowest over all seven, torso height at
// reset}; ints = {game_over, right-foot contact, left-foot contact, contact points, limit states x6}
void w2d_debug(const void *state, float *bodies, float *masses, float *sep, float *angles, float *limits, float *floats, int32_t *ints)
{
    const Walker2dEnv *e = (const Walker2dEnv *)state;
    const World<Walker2dDef> &w = e->w;
    float low_solved = FLT_BIG, low_all = FLT_BIG;
    for (int b = 0; b < 7; ++b) {
        const Body &B = w.body[b];
        const float v[6] = {B.cx, B.cy, B.a, B.vx, B.vy, B.w};
        memcpy(bodies + 6 * b, v, sizeof v);
        masses[b] = 1.0f / WALKER2D_BODY[b].inv_mass;
        const float s = sinf(B.a), c = cosf(B.a);
        for (int i = 0; i < 4; ++i) {
            const float y = (s * WALKER2D_POLY[b].vx[i] + c * WALKER2D_POLY[b].vy[i]) + B.cy;
            if (b >= 1 && y < low_solved) low_solved = y;
            if (y < low_all) low_all = y;
        }
    }
    for (int j = 0; j < 6; ++j) {
        const JointDef &jd = WALKER2D_JOINT[j];
        const Body &A = w.body[jd.a], &B = w.body[jd.b];
        const double sa = sin((double)A.a), ca = cos((double)A.a), sb = sin((double)B.a), cb = cos((double)B.a);
        const double ax = A.cx + (ca * jd.lax - sa * jd.lay), ay = A.cy + (sa * jd.lax + ca * jd.lay);
        const double bx = B.cx + (cb * jd.lbx - sb * jd.lby), by = B.cy + (sb * jd.lbx + cb * jd.lby);
        sep[j] = (float)sqrt((ax - bx) * (ax - bx) + (ay - by) * (ay - by));
        angles[j] = B.a - A.a;
        limits[2 * j] = jd.lower; limits[2 * j + 1] = jd.upper;
        ints[4 + j] = w.joint[j].state;
    }
    floats[0] = low_solved; floats[1] = low_all; floats[2] = e->init_y;
    ints[0] = w.game_over;
    ints[1] = w.ground_contact[W2D_FOOT];
    ints[2] = w.ground_contact[W2D_FOOT_LEFT];
    int points = 0;
    for (int b = 0; b < 6; ++b)
        for (int k = 0; k < 2; ++k) points += w.mf[b][k].count;
    ints[3] = points;
}

}  // extern "C"
