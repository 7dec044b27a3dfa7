// ses_walker2d_env.h -- Walker2DBulletEnv-v0: the build's own float32 definition of a planar two-legged walker, modelled on
// pybullet_envs' Walker2D (reached by the reference through envs/gym_wrapper.py:1-2,9), on the Box2D-style world of ses_b2.h: the
// hopper's leg (ses_hopper_env.h) twice on one torso.  Seven bodies -- 0 torso, 1 thigh, 2 leg, 3 foot, 4 thigh_left, 5 leg_left,
// 6 foot_left: rectangles standing in for the capsules of pybullet's walker2d.xml, ses_walker2d_shapes.h -- on six revolute joints
// with limits and torque motors (right leg j = 0, 1, 2, then left leg j = 3, 4, 5; both thighs hang on body 0, the tree BipedalWalker
// has), both feet in friction contact with a flat ground.  Bodies do not collide with each other: at the zero init row both legs
// occupy the same place.  pybullet and Bullet are third-party and absent, the sizes and constants are recalled: PARITY WITH BULLET
// IS UNPINNED (env_variant pybullet-restated).  DESIGN.md 7 is the specification.  ("walker" alone means BipedalWalker in this
// tree -- ses_walker.h -- so everything here is walker2d / W2D_ / w2d_.)
//
// One text compiled twice, like ses_hopper_env.h: for gfx950 by csrc/ses_walker2d.hip, for the host by tests/walker2d_host.cpp.
//
// Plane, angle signs and limits as the hopper's: x forward, y up, gravity -9.8; a joint's angle is (child angle - parent angle),
// thigh and leg in [-150 deg, 0], foot in [-45 deg, 45 deg].  One env step = 4 world steps of 0.0165 / 4 s with 8 velocity and 3
// position iterations each, discrete collision only.  Action: six values, clipped to [-1, 1]; joint j is driven with the torque
// 40 a_j (recalled from pybullet: gear 100 x power 0.40) through the joint motor exactly as the hopper's: motor speed
// sign(a_j) x W2D_MOTOR_SPEED, maximum torque 40 |a_j|.  pybullet's joint damping and armature are not modelled.  The torso's
// contacts are not solved and a touch ends the episode, as for the hopper (a stated deviation).
#pragma once
#include "ses_b2.h"
#include "ses_walker2d_shapes.h"

#ifndef W2D_PACK_MANIFOLDS
#define W2D_PACK_MANIFOLDS false      // measured both ways on an MI355X (profiles/walker2d_timing.txt)
#endif

namespace b2l {

constexpr float W2D_STEP_DT = 0.0165f;               // one env step
constexpr int W2D_SUBSTEPS = 4;
constexpr float W2D_DT = W2D_STEP_DT / 4.0f;         // one world step
constexpr float W2D_TORQUE = 40.0f;
constexpr float W2D_MOTOR_SPEED = 1000.0f;           // rad/s; the world caps a body at pi/2 per world step = 381 rad/s
constexpr float W2D_TORSO_Y = 1.25f;
constexpr float W2D_ALIVE_Y = 0.8f, W2D_ALIVE_PITCH = 1.0f;
constexpr float W2D_EDGE = 4.0f;                     // ground edges: [-2048, 2048) in pieces of 4 m
constexpr int W2D_N_EDGES = 1024;
constexpr float W2D_DEG = PI / 180.0f;
constexpr int W2D_NB = 7, W2D_NJ = 6, W2D_NOBS = 22;
constexpr int W2D_FOOT = 3, W2D_FOOT_LEFT = 6;

// anchors (0, 1.05), (0, 0.60), (0, 0.10) in the frames of the bodies at rest: torso centre (0, 1.25), thigh (0, 0.825),
// leg (0, 0.35), foot (0.10, 0.10) -- the foot's capsule runs from the ankle forward to (0.20, 0.10)
#define W2D_LEG_JOINTS(thigh)                                                             \
    {0, thigh, 0.0f, -0.20f, 0.0f, 0.225f, -150.0f * W2D_DEG, 0.0f},                      \
    {thigh, thigh + 1, 0.0f, -0.225f, 0.0f, 0.25f, -150.0f * W2D_DEG, 0.0f},              \
    {thigh + 1, thigh + 2, 0.0f, -0.25f, -0.10f, 0.0f, -45.0f * W2D_DEG, 45.0f * W2D_DEG}
B2_CONST JointDef WALKER2D_JOINT[6] = {W2D_LEG_JOINTS(1), W2D_LEG_JOINTS(4)};
#undef W2D_LEG_JOINTS

struct Walker2dDef {
    static constexpr int NB = W2D_NB, NJ = W2D_NJ, NSLOT = 2, FIRST_SOLVED = 1, VEL_ITERS = 8, POS_ITERS = 3;
    static constexpr bool PACK_MANIFOLDS = W2D_PACK_MANIFOLDS;   // 6 x 2 slots: 12 rows of world_solve's 32-bit mask
    static constexpr bool CONTINUOUS = false;        // nothing is thin or fast enough to tunnel at a 4 ms world step
    static constexpr int VEL_FIXED_POINT_CHECK = -1;
    static constexpr float GRAVITY_Y = -9.8f;
    B2_FN const Poly *poly() { return WALKER2D_POLY; }
    B2_FN const BodyDef *body() { return WALKER2D_BODY; }
    B2_FN const JointDef *joint() { return WALKER2D_JOINT; }
};

// the hopper's ground again (HopperTerrain, ses_hopper_env.h), under this env's name so that neither header needs the other: flat
// at y = 0, collinear edges computed from their index, no memory behind them.  No body's fattened box is longer than 1 m, so it
// overlaps at most two edges (NSLOT 2); index_of never clamps for |x| < 2048.
struct Walker2dTerrain {
    B2_FN_MEMBER int n_edges() const { return W2D_N_EDGES; }
    B2_FN_MEMBER int index_of(float x) const { return (int)B2_FLOOR(x * (1.0f / W2D_EDGE) + (float)(W2D_N_EDGES / 2)); }
    B2_FN_MEMBER void edge(int k, float &x1, float &y1, float &x2, float &y2) const
    {
        x1 = (float)(k - W2D_N_EDGES / 2) * W2D_EDGE; y1 = 0.0f;
        x2 = (float)(k + 1 - W2D_N_EDGES / 2) * W2D_EDGE; y2 = 0.0f;
    }
};

struct Walker2dEnv {
    World<Walker2dDef> w;
    float init_y;                                    // the torso's height after reset
};

// float32[22] in pybullet's layout, its planar constants kept: [0 .. 7] as the hopper's (torso height above its height at reset,
// 0, 1, 0.3 vx, 0, 0.3 vy, 0, pitch), [8 + 2j] joint j's angle scaled to [-1, 1] over its limits, [9 + 2j] 0.1 x its speed
// (j = 0 .. 5), [20] right-foot contact, [21] left-foot contact.  Everything clipped to [-5, 5].
B2_FN void walker2d_obs(const Walker2dEnv &e, float (&obs)[W2D_NOBS])
{
    const World<Walker2dDef> &w = e.w;
    const Body &T = w.body[0];
    obs[0] = T.cy - e.init_y;
    obs[1] = 0.0f;
    obs[2] = 1.0f;
    obs[3] = 0.3f * T.vx;
    obs[4] = 0.0f;
    obs[5] = 0.3f * T.vy;
    obs[6] = 0.0f;
    obs[7] = T.a;
    B2_UNROLL
    for (int j = 0; j < W2D_NJ; ++j) {
        const JointDef &jd = WALKER2D_JOINT[j];
        const float angle = w.body[jd.b].a - w.body[jd.a].a;
        const float speed = w.body[jd.b].w - w.body[jd.a].w;
        const float mid = 0.5f * (jd.lower + jd.upper);
        obs[8 + 2 * j] = 2.0f * (angle - mid) / (jd.upper - jd.lower);
        obs[9 + 2 * j] = 0.1f * speed;
    }
    obs[20] = w.ground_contact[W2D_FOOT] ? 1.0f : 0.0f;
    obs[21] = w.ground_contact[W2D_FOOT_LEFT] ? 1.0f : 0.0f;
    B2_UNROLL
    for (int k = 0; k < W2D_NOBS; ++k) obs[k] = b2clamp(obs[k], -5.0f, 5.0f);
}

// The four reward terms of a step, summed in this order (walker2d_step).  `a`: the clipped action; `o`: the observation AFTER
// the step; x0, x1: the torso's x before and after.
B2_FN void walker2d_reward_terms(const float (&a)[W2D_NJ], const float (&o)[W2D_NOBS], float torso_y, float x0, float x1, float (&term)[4])
{
    const bool alive = torso_y > W2D_ALIVE_Y && b2abs(o[7]) < W2D_ALIVE_PITCH;
    term[0] = alive ? 1.0f : -1.0f;
    term[1] = (x1 - x0) / W2D_STEP_DT;
    float work = 0.0f, sq = 0.0f, at_limit = 0.0f;
    B2_UNROLL
    for (int j = 0; j < W2D_NJ; ++j) {
        work += b2abs(a[j] * o[9 + 2 * j]);
        sq += a[j] * a[j];
        at_limit += b2abs(o[8 + 2 * j]) > 0.99f ? 1.0f : 0.0f;
    }
    term[2] = -2.0f * (work / 6.0f) - 0.1f * (sq / 6.0f);
    term[3] = -0.1f * at_limit;
}

// one env step; returns the reward, sets done (the alive term is negative, or the torso touches the ground).  term_out: the
// four terms, for the host's diagnostics.
B2_FN float walker2d_step(Walker2dEnv &e, const float (&action)[W2D_NJ], bool &done, float *term_out = nullptr)
{
    World<Walker2dDef> &w = e.w;
    const Walker2dTerrain terr{};
    float a[W2D_NJ];
    B2_UNROLL
    for (int j = 0; j < W2D_NJ; ++j) {
        a[j] = b2clamp(action[j], -1.0f, 1.0f);
        const float sgn = a[j] > 0.0f ? 1.0f : (a[j] < 0.0f ? -1.0f : 0.0f);
        w.joint[j].motor_speed = W2D_MOTOR_SPEED * sgn;
        w.joint[j].max_torque = W2D_TORQUE * b2abs(a[j]);
    }
    const float x0 = w.body[0].cx;
    for (int s = 0; s < W2D_SUBSTEPS; ++s) world_step(w, terr, W2D_DT);
    float o[W2D_NOBS], term[4];
    walker2d_obs(e, o);
    walker2d_reward_terms(a, o, w.body[0].cy, x0, w.body[0].cx, term);
    if (term_out) {
        B2_UNROLL
        for (int k = 0; k < 4; ++k) term_out[k] = term[k];
    }
    done = term[0] < 0.0f || w.game_over;
    return ((term[0] + term[1]) + term[2]) + term[3];
}

// reset from one init row of 6 uniforms in [-0.1, 0.1): the joint angles, clipped into their limits.  Zero velocities; the
// chain is built by forward kinematics from the torso at (0, 1.25), then lifted by whatever its lowest vertex would be below
// the ground.
B2_FN void walker2d_reset(Walker2dEnv &e, const float *u)
{
    World<Walker2dDef> &w = e.w;
    w.body[0].cx = 0.0f; w.body[0].cy = W2D_TORSO_Y; w.body[0].a = 0.0f;
    B2_UNROLL
    for (int j = 0; j < W2D_NJ; ++j) {
        const JointDef &jd = WALKER2D_JOINT[j];
        const Body &A = w.body[jd.a];
        Body &B = w.body[jd.b];
        B.a = A.a + b2clamp(u[j], jd.lower, jd.upper);
        float sa, ca, sb, cb;
        B2_SINCOS(A.a, sa, ca);
        B2_SINCOS(B.a, sb, cb);
        const float ax = A.cx + (ca * jd.lax - sa * jd.lay), ay = A.cy + (sa * jd.lax + ca * jd.lay);   // the anchor in the world
        B.cx = ax - (cb * jd.lbx - sb * jd.lby);
        B.cy = ay - (sb * jd.lbx + cb * jd.lby);
    }
    float ymin = FLT_BIG;
    B2_UNROLL
    for (int b = 0; b < W2D_NB; ++b) {
        float s, c;
        B2_SINCOS(w.body[b].a, s, c);
        const Poly &P = WALKER2D_POLY[b];
        B2_UNROLL
        for (int i = 0; i < 4; ++i) ymin = b2min(ymin, (s * P.vx[i] + c * P.vy[i]) + w.body[b].cy);
    }
    const float lift = ymin < 0.0f ? -ymin : 0.0f;
    B2_UNROLL
    for (int b = 0; b < W2D_NB; ++b) {
        Body &B = w.body[b];
        B.cy += lift;
        B.vx = 0.0f; B.vy = 0.0f; B.w = 0.0f;
        xf_of(B, WALKER2D_BODY[b], w.xf[b]);
        w.sleep_time[b] = 0.0f;
        w.ground_contact[b] = false;
        B2_UNROLL
        for (int s = 0; s < Walker2dDef::NSLOT && b >= Walker2dDef::FIRST_SOLVED; ++s) {
            Manifold &m = w.mf[b - Walker2dDef::FIRST_SOLVED][s];
            m.edge = -1; m.count = 0; m.type = 0;
            m.lnx = 0.0f; m.lny = 0.0f; m.lpx = 0.0f; m.lpy = 0.0f;
            B2_UNROLL
            for (int i = 0; i < 2; ++i) { m.px[i] = 0.0f; m.py[i] = 0.0f; m.id[i] = 0u; m.ni[i] = 0.0f; m.ti[i] = 0.0f; }
        }
    }
    B2_UNROLL
    for (int j = 0; j < W2D_NJ; ++j) {
        Joint &J = w.joint[j];
        J.ix = 0.0f; J.iy = 0.0f; J.iz = 0.0f; J.im = 0.0f;
        J.state = LIMIT_INACTIVE;
        J.motor_speed = 0.0f;
        J.max_torque = 0.0f;
    }
    w.game_over = false; w.awake = true;
    w.fx = 0.0f; w.fy = 0.0f;
    e.init_y = w.body[0].cy;
}

}  // namespace b2l
