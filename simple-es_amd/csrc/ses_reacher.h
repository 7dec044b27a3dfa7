// ses_reacher.h -- ReacherBulletEnv-v0 modelled on pybullet_envs, in float64: a planar two-link arm that has to put its
// fingertip on a target drawn anew for every episode.  This is the build's OWN definition: two uniform rods with closed-form
// rigid-body dynamics in a horizontal plane (no gravity term), semi-implicit Euler at dt = 0.0165, a fixed horizon of 150
// steps.  DESIGN.md 7 holds the equations in the order of operations used here and is the specification; tests/reacher_np.py
// restates it in numpy and reproduces every transition bit for bit.  pybullet is not installed, the constants are the build's
// own and parity with Bullet is UNPINNED.
//
// Every operation is a plain correctly rounded IEEE-754 add, sub, mul, div or compare (the build passes -ffp-contract=off),
// __dsqrt_rn for the one distance (as in ses_waterworld.h), and sincos_ieee of ses_classic.h is the only transcendental: sin
// and cos of th + g come from the addition formulas.  The two actions are the policy's float32 tanh outputs widened to double
// and clipped to [-1, 1]; the clipped values drive the joints AND enter the reward's cost terms.  Rewards are float64.
//
// The first member of the family with two actions, with a goal randomised per episode (the target lives in the state) and
// with a reward that is a potential DIFFERENCE: the potential of the state entered is carried in the state blob.
//
// A transition is split into the pieces a fused rollout wants to schedule itself (the ses_pendula.h shape):
//   trig(state)                 two sincos_ieee calls and the addition formulas
//   observe_from(state, trig)
//   advance(state, trig, a)     accelerations from the CURRENT state and its trig, rates first, angles with the new rates, the
//                               elbow limit
//   outcome(state, trig, a)     the reward of the step that ENTERED the state, from its trig; stores the new potential
// so that one trig per step serves the outcome of step t and the observation and dynamics of step t + 1.
#pragma once
#include "ses_classic.h"

namespace ses {

constexpr double RC_DT = 0.0165;
constexpr double RC_L1 = 0.1, RC_L2 = 0.11, RC_M1 = 0.0356, RC_M2 = 0.0393;
constexpr double RC_LC1 = 0.05, RC_LC2 = 0.055;                          // the rods' centres: half their lengths
constexpr double RC_I1 = (RC_M1 * (RC_L1 * RC_L1)) / 12.0, RC_I2 = (RC_M2 * (RC_L2 * RC_L2)) / 12.0;
constexpr double RC_J = 0.002;                                           // armature on both diagonal entries
constexpr double RC_DAMP = 0.01, RC_TORQUE = 0.05;
constexpr double RC_LIMIT = 3.0;                                         // |g| <= 3
constexpr double RC_PI = 3.141592653589793, RC_TARGET = 0.27;
// M11 = RC_M11C + (2 RC_A) cos g, M12 = RC_M12C + RC_A cos g, M22 = RC_M22 (a constant, and so is its reciprocal), h = RC_A sin g
constexpr double RC_A = (RC_M2 * RC_L1) * RC_LC2;
constexpr double RC_2A = 2.0 * RC_A;
constexpr double RC_M12C = RC_I2 + RC_M2 * (RC_LC2 * RC_LC2);
constexpr double RC_M11C = (((RC_I1 + RC_I2) + RC_M1 * (RC_LC1 * RC_LC1)) + RC_M2 * (RC_L1 * RC_L1 + RC_LC2 * RC_LC2)) + RC_J;
constexpr double RC_M22 = RC_M12C + RC_J;
constexpr double RC_R22 = 1.0 / RC_M22;
constexpr int RC_INIT_W = 4;                                             // init row: u0 .. u3 ~ U(-1, 1)

struct ReacherState {
    double th, w1, g, w2, tx, ty, pot;                                   // 56 B
};
struct ReacherTrig {
    double st, ct, sg, cg, sb, cb;                                       // of th, g and th + g
};

__device__ __forceinline__ void reacher_trig(const ReacherState &s, ReacherTrig &t)
{
    sincos_ieee(s.th, t.st, t.ct);
    sincos_ieee(s.g, t.sg, t.cg);
    t.sb = t.st * t.cg + t.ct * t.sg;
    t.cb = t.ct * t.cg - t.st * t.sg;
}

// fingertip - target
__device__ __forceinline__ double reacher_dx(const ReacherState &s, const ReacherTrig &t) { return (RC_L1 * t.ct + RC_L2 * t.cb) - s.tx; }
__device__ __forceinline__ double reacher_dy(const ReacherState &s, const ReacherTrig &t) { return (RC_L1 * t.st + RC_L2 * t.sb) - s.ty; }

// pot = -100 |fingertip - target|
__device__ __forceinline__ double reacher_potential(const ReacherState &s, const ReacherTrig &t)
{
    const double dx = reacher_dx(s, t), dy = reacher_dy(s, t);
    return -100.0 * __dsqrt_rn(dx * dx + dy * dy);
}

__device__ __forceinline__ void reacher_obs_from(const ReacherState &s, const ReacherTrig &t, float (&o)[9])
{
    o[0] = (float)s.tx;
    o[1] = (float)s.ty;
    o[2] = (float)reacher_dx(s, t);
    o[3] = (float)reacher_dy(s, t);
    o[4] = (float)t.ct;
    o[5] = (float)t.st;
    o[6] = (float)s.w1;
    o[7] = (float)s.g;
    o[8] = (float)s.w2;
}

// M(g) q'' = tau - D w - c(g, w), c = (-h (2 w1 w2 + w2^2), h w1^2).  The 2 x 2 solve eliminates with the CONSTANT pivot M22:
// one division per step.
__device__ __forceinline__ void reacher_advance(ReacherState &s, const ReacherTrig &t, double a0, double a1)
{
    const double tau1 = RC_TORQUE * a0, tau2 = RC_TORQUE * a1;           // a0, a1: already clipped
    const double m11 = RC_M11C + RC_2A * t.cg;
    const double m12 = RC_M12C + RC_A * t.cg;
    const double h = RC_A * t.sg;
    const double b1 = (tau1 - RC_DAMP * s.w1) + h * ((2.0 * s.w1) * s.w2 + s.w2 * s.w2);
    const double b2 = (tau2 - RC_DAMP * s.w2) - h * (s.w1 * s.w1);
    const double m = m12 * RC_R22;
    const double e11 = m11 - m * m12, f1 = b1 - m * b2;
    const double acc1 = f1 / e11;
    const double acc2 = (b2 - m12 * acc1) * RC_R22;
    s.w1 = s.w1 + RC_DT * acc1;
    s.w2 = s.w2 + RC_DT * acc2;
    s.th = s.th + RC_DT * s.w1;
    s.g = s.g + RC_DT * s.w2;
    if (s.g > RC_LIMIT) {                                                // the shape of pendula_rail: where the angle was
        s.g = RC_LIMIT;                                                  // clipped, an outward rate becomes 0
        s.w2 = s.w2 > 0.0 ? 0.0 : s.w2;
    }
    if (s.g < -RC_LIMIT) {
        s.g = -RC_LIMIT;
        s.w2 = s.w2 < 0.0 ? 0.0 : s.w2;
    }
}

// the reward of the step that entered s (its new rates, its trig) under the clipped actions a0, a1; s.pot becomes pot_new
__device__ __forceinline__ double reacher_outcome(ReacherState &s, const ReacherTrig &t, double a0, double a1)
{
    const double pot = reacher_potential(s, t);
    double r = pot - s.pot;
    r = r - 0.10 * (__builtin_fabs(a0 * s.w1) + __builtin_fabs(a1 * s.w2));
    r = r - 0.01 * (__builtin_fabs(a0) + __builtin_fabs(a1));
    if (__builtin_fabs(__builtin_fabs(s.g) - 1.0) < 0.01) r = r - 0.1;
    s.pot = pot;
    return r;
}

// A trig env of the contract in ses_classic.h.  step_from clips the actions, advances from the trig of the state it leaves and
// takes the outcome from the trig of the state it enters; never done.
struct ReacherEnv : TrigEnv<ReacherEnv> {
    static constexpr int S = 9, A = 2, INIT_W = RC_INIT_W;
    static constexpr bool TERMINATES = false;
    static constexpr const char *NAME = "Reacher";
    using State = ReacherState;
    using Trig = ReacherTrig;
    using Action = float[A];
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u)
    {
        s = State{RC_PI * (double)u[2], 0.0, RC_LIMIT * (double)u[3], 0.0, RC_TARGET * (double)u[0], RC_TARGET * (double)u[1], 0.0};
        Trig t;
        reacher_trig(s, t);
        s.pot = reacher_potential(s, t);
    }
    __device__ static __forceinline__ void trig(const State &s, Trig &t) { reacher_trig(s, t); }
    __device__ static __forceinline__ void observe_from(const State &s, const Trig &t, float (&o)[S]) { reacher_obs_from(s, t, o); }
    __device__ static __forceinline__ double step_from(State &s, Trig &t, const float (&act)[A], bool &done)
    {
        const double a0 = clip_ieee((double)act[0], -1.0, 1.0), a1 = clip_ieee((double)act[1], -1.0, 1.0);
        reacher_advance(s, t, a0, a1);
        reacher_trig(s, t);
        done = false;
        return reacher_outcome(s, t, a0, a1);
    }
};

}  // namespace ses
