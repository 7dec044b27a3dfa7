// ses_hopper_env.h -- HopperBulletEnv-v0: the build's own float32 definition of a planar one-legged hopper, modelled on
// pybullet_envs' hopper (reached by the reference through envs/gym_wrapper.py:1-2,9), on the Box2D-style world of ses_b2.h:
// torso, thigh, leg and foot (rectangles standing in for the capsules of pybullet's hopper.xml, ses_hopper_shapes.h) on a chain of
// three revolute joints with limits and torque motors, the foot in friction contact with a flat ground.  pybullet and Bullet are
// third-party and absent: PARITY WITH BULLET IS UNPINNED (env_variant pybullet-restated).  DESIGN.md 7 is the specification.
//
// One text compiled twice, like ses_walker_env.h: for gfx950 by csrc/ses_hopper.hip, for the host by tests/hopper_host.cpp.
//
// Plane: x forward, y up, gravity -9.8.  Angles are counter-clockwise; a joint's angle is (child angle - parent angle), so a
// NEGATIVE thigh or leg angle swings the lower end of the child backwards (the knee bends like a human's) and a positive foot
// angle lifts the toe.  Limits: thigh, leg [-150 deg, 0], foot [-45 deg, 45 deg].
// One env step = 4 world steps of 0.0165 / 4 s (pybullet's frame skip) with 8 velocity and 3 position iterations each (Box2D's
// documented defaults), discrete collision only.  Action: three values, clipped to [-1, 1]; joint j is driven with the torque
// 150 a_j (pybullet: gear 200 x power 0.75) through the joint motor: motor speed sign(a_j) x HP_MOTOR_SPEED -- a speed that no
// joint reaches, so the motor row always sits on its impulse bound -- and maximum torque 150 |a_j|.  pybullet's joint damping
// and armature are not modelled.
#pragma once
#include "ses_b2.h"
#include "ses_hopper_shapes.h"

namespace b2l {

constexpr float HP_STEP_DT = 0.0165f;                // one env step
constexpr int HP_SUBSTEPS = 4;
constexpr float HP_DT = HP_STEP_DT / 4.0f;           // one world step
constexpr float HP_TORQUE = 150.0f;
constexpr float HP_MOTOR_SPEED = 1000.0f;            // rad/s; the world caps a body at pi/2 per world step = 381 rad/s
constexpr float HP_TORSO_Y = 1.25f;
constexpr float HP_ALIVE_Y = 0.8f, HP_ALIVE_PITCH = 1.0f;
constexpr float HP_EDGE = 4.0f;                      // ground edges: [-2048, 2048) in pieces of 4 m
constexpr int HP_N_EDGES = 1024;
constexpr float HP_DEG = PI / 180.0f;

// anchors (0, 1.05), (0, 0.60), (0, 0.10) in the frames of the bodies at rest: torso centre (0, 1.25), thigh (0, 0.825),
// leg (0, 0.35), foot (0.065, 0.10)
B2_CONST JointDef HOPPER_JOINT[3] = {
    {0, 1, 0.0f, -0.20f, 0.0f, 0.225f, -150.0f * HP_DEG, 0.0f},
    {1, 2, 0.0f, -0.225f, 0.0f, 0.25f, -150.0f * HP_DEG, 0.0f},
    {2, 3, 0.0f, -0.25f, -0.065f, 0.0f, -45.0f * HP_DEG, 45.0f * HP_DEG},
};

struct HopperDef {
    static constexpr int NB = 4, NJ = 3, NSLOT = 2, FIRST_SOLVED = 1, VEL_ITERS = 8, POS_ITERS = 3;
    static constexpr bool PACK_MANIFOLDS = false;    // 3 x 2 slots, as the lander's 2 x 2
    static constexpr bool CONTINUOUS = false;        // nothing is thin or fast enough to tunnel at a 4 ms world step
    static constexpr int VEL_FIXED_POINT_CHECK = -1;
    static constexpr float GRAVITY_Y = -9.8f;
    B2_FN const Poly *poly() { return HOPPER_POLY; }
    B2_FN const BodyDef *body() { return HOPPER_BODY; }
    B2_FN const JointDef *joint() { return HOPPER_JOINT; }
};

// flat ground at y = 0: collinear edges computed from their index, no memory behind them.  No body's fattened box is longer
// than 1 m, so it overlaps at most two edges (NSLOT 2); index_of never clamps for |x| < 2048.
struct HopperTerrain {
    B2_FN_MEMBER int n_edges() const { return HP_N_EDGES; }
    B2_FN_MEMBER int index_of(float x) const { return (int)B2_FLOOR(x * (1.0f / HP_EDGE) + (float)(HP_N_EDGES / 2)); }
    B2_FN_MEMBER void edge(int k, float &x1, float &y1, float &x2, float &y2) const
    {
        x1 = (float)(k - HP_N_EDGES / 2) * HP_EDGE; y1 = 0.0f;
        x2 = (float)(k + 1 - HP_N_EDGES / 2) * HP_EDGE; y2 = 0.0f;
    }
};

struct HopperEnv {
    World<HopperDef> w;
    float init_y;                                    // the torso's height after reset
};

// float32[15] in pybullet's layout, its planar constants kept: [0] torso height above its height at reset, [1] 0, [2] 1
// (sin, cos of the angle to a target straight ahead), [3] 0.3 vx, [4] 0, [5] 0.3 vy, [6] 0 (roll), [7] pitch, [8 + 2j] the
// joint's angle scaled to [-1, 1] over its limits, [9 + 2j] 0.1 x its speed, [14] foot contact.  Everything clipped to [-5, 5].
B2_FN void hopper_obs(const HopperEnv &e, float (&obs)[15])
{
    const World<HopperDef> &w = e.w;
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
    for (int j = 0; j < 3; ++j) {
        const JointDef &jd = HOPPER_JOINT[j];
        const float angle = w.body[jd.b].a - w.body[jd.a].a;
        const float speed = w.body[jd.b].w - w.body[jd.a].w;
        const float mid = 0.5f * (jd.lower + jd.upper);
        obs[8 + 2 * j] = 2.0f * (angle - mid) / (jd.upper - jd.lower);
        obs[9 + 2 * j] = 0.1f * speed;
    }
    obs[14] = w.ground_contact[3] ? 1.0f : 0.0f;
    B2_UNROLL
    for (int k = 0; k < 15; ++k) obs[k] = b2clamp(obs[k], -5.0f, 5.0f);
}

// The four reward terms of a step, summed in this order (hopper_step).  `a`: the clipped action; `o`: the observation AFTER
// the step; x0, x1: the torso's x before and after.
B2_FN void hopper_reward_terms(const float (&a)[3], const float (&o)[15], float torso_y, float x0, float x1, float (&term)[4])
{
    const bool alive = torso_y > HP_ALIVE_Y && b2abs(o[7]) < HP_ALIVE_PITCH;
    term[0] = alive ? 1.0f : -1.0f;
    term[1] = (x1 - x0) / HP_STEP_DT;
    float work = 0.0f, sq = 0.0f, at_limit = 0.0f;
    B2_UNROLL
    for (int j = 0; j < 3; ++j) {
        work += b2abs(a[j] * o[9 + 2 * j]);
        sq += a[j] * a[j];
        at_limit += b2abs(o[8 + 2 * j]) > 0.99f ? 1.0f : 0.0f;
    }
    term[2] = -2.0f * (work / 3.0f) - 0.1f * (sq / 3.0f);
    term[3] = -0.1f * at_limit;
}

// one env step; returns the reward, sets done (the alive term is negative, or the torso touches the ground).  term_out: the
// four terms, for the host's diagnostics.
B2_FN float hopper_step(HopperEnv &e, const float (&action)[3], bool &done, float *term_out = nullptr)
{
    World<HopperDef> &w = e.w;
    const HopperTerrain terr{};
    float a[3];
    B2_UNROLL
    for (int j = 0; j < 3; ++j) {
        a[j] = b2clamp(action[j], -1.0f, 1.0f);
        const float sgn = a[j] > 0.0f ? 1.0f : (a[j] < 0.0f ? -1.0f : 0.0f);
        w.joint[j].motor_speed = HP_MOTOR_SPEED * sgn;
        w.joint[j].max_torque = HP_TORQUE * b2abs(a[j]);
    }
    const float x0 = w.body[0].cx;
    for (int s = 0; s < HP_SUBSTEPS; ++s) world_step(w, terr, HP_DT);
    float o[15], term[4];
    hopper_obs(e, o);
    hopper_reward_terms(a, o, w.body[0].cy, x0, w.body[0].cx, term);
    if (term_out) {
        B2_UNROLL
        for (int k = 0; k < 4; ++k) term_out[k] = term[k];
    }
    done = term[0] < 0.0f || w.game_over;
    return ((term[0] + term[1]) + term[2]) + term[3];
}

// reset from one init row of 3 uniforms in [-0.1, 0.1): the joint angles, clipped into their limits.  Zero velocities; the
// chain is built by forward kinematics from the torso at (0, 1.25), then lifted by whatever its lowest vertex would be below
// the ground.
B2_FN void hopper_reset(HopperEnv &e, const float *u)
{
    World<HopperDef> &w = e.w;
    w.body[0].cx = 0.0f; w.body[0].cy = HP_TORSO_Y; w.body[0].a = 0.0f;
    B2_UNROLL
    for (int j = 0; j < 3; ++j) {
        const JointDef &jd = HOPPER_JOINT[j];
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
    for (int b = 0; b < 4; ++b) {
        float s, c;
        B2_SINCOS(w.body[b].a, s, c);
        const Poly &P = HOPPER_POLY[b];
        B2_UNROLL
        for (int i = 0; i < 4; ++i) ymin = b2min(ymin, (s * P.vx[i] + c * P.vy[i]) + w.body[b].cy);
    }
    const float lift = ymin < 0.0f ? -ymin : 0.0f;
    B2_UNROLL
    for (int b = 0; b < 4; ++b) {
        Body &B = w.body[b];
        B.cy += lift;
        B.vx = 0.0f; B.vy = 0.0f; B.w = 0.0f;
        xf_of(B, HOPPER_BODY[b], w.xf[b]);
        w.sleep_time[b] = 0.0f;
        w.ground_contact[b] = false;
        B2_UNROLL
        for (int s = 0; s < HopperDef::NSLOT && b >= HopperDef::FIRST_SOLVED; ++s) {
            Manifold &m = w.mf[b - HopperDef::FIRST_SOLVED][s];
            m.edge = -1; m.count = 0; m.type = 0;
            m.lnx = 0.0f; m.lny = 0.0f; m.lpx = 0.0f; m.lpy = 0.0f;
            B2_UNROLL
            for (int i = 0; i < 2; ++i) { m.px[i] = 0.0f; m.py[i] = 0.0f; m.id[i] = 0u; m.ni[i] = 0.0f; m.ti[i] = 0.0f; }
        }
    }
    B2_UNROLL
    for (int j = 0; j < 3; ++j) {
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
