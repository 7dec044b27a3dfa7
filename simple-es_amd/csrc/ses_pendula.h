// ses_pendula.h -- the inverted-pendulum family modelled on pybullet_envs, in float64: InvertedPendulumBulletEnv-v0 (balance),
// InvertedPendulumSwingupBulletEnv-v0 and InvertedDoublePendulumBulletEnv-v0.  These are the build's OWN definitions: rigid
// links on a cart with closed-form equations of motion, semi-implicit Euler at dt = 0.0165.  DESIGN.md 7 holds the equations in
// the order of operations used here and is the specification; tests/pendula_np.py restates it in numpy and reproduces every
// transition bit for bit.  The masses and lengths are recalled from pybullet's MJCF geometry and nothing here verifies them;
// parity with Bullet is UNPINNED (pybullet is not part of the reference tree).
//
// Every operation is a plain correctly rounded IEEE-754 add, sub, mul, div or compare (the build passes -ffp-contract=off) and
// sincos_ieee of ses_classic.h is the only transcendental -- the ses_classic.h rule, which is what makes the restatement exact.
// The action is the policy's float32 tanh output widened to double and clipped to [-1, 1]; rewards are float64.
//
// Each env splits a transition into the pieces a fused rollout wants to schedule itself:
//   trig(state)            the step's sincos_ieee calls (one per angle)
//   observe_from(state, trig)
//   advance(state, trig, a)   accelerations from the CURRENT state and its trig, velocities first, positions with the new
//                             velocities, the rail
//   outcome(state, trig)      reward and done of the NEW state, from its trig
// so that one trig per step serves the outcome of step t and the observation and dynamics of step t + 1.
#pragma once
#include "ses_classic.h"

namespace ses {

constexpr double PB_DT = 0.0165, PB_G = 9.8;
constexpr double PB_CART_M = 10.472;                 // the cart
constexpr double PB_RAIL = 1.0;                      // |x| <= 1
constexpr double PB_FOUR_THIRDS = 4.0 / 3.0;

// x is clipped to the rail; where it was clipped, a velocity that points outward becomes 0
__device__ __forceinline__ void pendula_rail(double &x, double &v)
{
    if (x > PB_RAIL) {
        x = PB_RAIL;
        v = v > 0.0 ? 0.0 : v;
    }
    if (x < -PB_RAIL) {
        x = -PB_RAIL;
        v = v < 0.0 ? 0.0 : v;
    }
}

// ---- the single pendulum: a uniform rod (mass m, half-length l) hinged on the cart; theta = 0 is upright, positive towards +x ----
//   (M + m) x'' + m l (theta'' cos theta - omega^2 sin theta) = F
//   (4/3) m l^2 theta'' + m l x'' cos theta = m g l sin theta
constexpr double IP_POLE_M = 5.0186, IP_L = 0.3;
constexpr double IP_TOTAL_M = PB_CART_M + IP_POLE_M, IP_ML = IP_POLE_M * IP_L;
constexpr double IP_FORCE = 100.0;
constexpr double IP_FALL = 0.2;                      // balance: done when |theta| > 0.2
constexpr double IP_SWINGUP_TH0 = 3.1415;            // swing-up: the reset angle is 3.1415 + u (hanging)
constexpr int IP_INIT_W = 1;                         // init row: u ~ U(-0.1, 0.1)

struct PoleState {
    double x, v, th, w;
};
struct PoleTrig {
    double sn, cs;
};

__device__ __forceinline__ void pole_trig(const PoleState &s, PoleTrig &t) { sincos_ieee(s.th, t.sn, t.cs); }

__device__ __forceinline__ void pole_obs_from(const PoleState &s, const PoleTrig &t, float (&o)[5])
{
    o[0] = (float)s.x;
    o[1] = (float)s.v;
    o[2] = (float)t.cs;
    o[3] = (float)t.sn;
    o[4] = (float)s.w;
}

__device__ __forceinline__ void pole_advance(PoleState &s, const PoleTrig &t, double a)
{
    const double force = IP_FORCE * clip_ieee(a, -1.0, 1.0);
    const double temp = (force + (IP_ML * (s.w * s.w)) * t.sn) / IP_TOTAL_M;
    const double thacc = (PB_G * t.sn - t.cs * temp) / (IP_L * (PB_FOUR_THIRDS - (IP_POLE_M * (t.cs * t.cs)) / IP_TOTAL_M));
    const double xacc = temp - ((IP_ML * thacc) * t.cs) / IP_TOTAL_M;
    s.v = s.v + PB_DT * xacc;
    s.w = s.w + PB_DT * thacc;
    s.x = s.x + PB_DT * s.v;
    s.th = s.th + PB_DT * s.w;
    pendula_rail(s.x, s.v);
}

// ---- the double pendulum: two uniform rods (mass m each, length L = 2 l) on the cart; th2 is the second hinge's RELATIVE angle --
// In the absolute angles alpha = th1, beta = th1 + th2 (their rates wa = w1, wb = w1 + w2) the Lagrangian gives
//   [ D1          D4 cos alpha   D5 cos beta  ] [ x''     ]   [ F + D4 wa^2 sin alpha + D5 wb^2 sin beta ]
//   [ D4 cos alpha  D2           D6 cos th2   ] [ alpha'' ] = [ g D4 sin alpha + D6 wb^2 sin th2         ]
//   [ D5 cos beta   D6 cos th2   D3           ] [ beta''  ]   [ g D5 sin beta  - D6 wa^2 sin th2         ]
// with D1 = M + 2 m, D2 = (4/3) m l^2 + m L^2, D3 = (4/3) m l^2, D4 = m l + m L, D5 = m l, D6 = m L l; th1'' = alpha'',
// th2'' = beta'' - alpha''.  sin / cos of beta come from the addition formulas, not from a third sincos_ieee.
constexpr double DP_POLE_M = 4.1987, DP_LEN = 0.6, DP_L = 0.3;
constexpr double DP_FORCE = 200.0;
constexpr double DP_D1 = (PB_CART_M + DP_POLE_M) + DP_POLE_M;
constexpr double DP_D2 = (PB_FOUR_THIRDS * DP_POLE_M) * (DP_L * DP_L) + DP_POLE_M * (DP_LEN * DP_LEN);
constexpr double DP_D3 = (PB_FOUR_THIRDS * DP_POLE_M) * (DP_L * DP_L);
constexpr double DP_D4 = DP_POLE_M * DP_L + DP_POLE_M * DP_LEN;
constexpr double DP_D5 = DP_POLE_M * DP_L;
constexpr double DP_D6 = (DP_POLE_M * DP_LEN) * DP_L;
constexpr double DP_R1 = 1.0 / DP_D1;                // the first pivot is a constant, and so is its reciprocal
constexpr int DP_INIT_W = 2;                         // init row: th1 = u0, th2 = u1 ~ U(-0.1, 0.1)

struct DoubleState {
    double x, v, th1, w1, th2, w2;
};
struct DoubleTrig {
    double s1, c1, s2, c2, sb, cb;                   // of th1, th2 and beta = th1 + th2
};

__device__ __forceinline__ void double_trig(const DoubleState &s, DoubleTrig &t)
{
    sincos_ieee(s.th1, t.s1, t.c1);
    sincos_ieee(s.th2, t.s2, t.c2);
    t.sb = t.s1 * t.c2 + t.c1 * t.s2;
    t.cb = t.c1 * t.c2 - t.s1 * t.s2;
}

// the centre of the second rod: x2 = x + L sin th1 + l sin beta, y2 = L cos th1 + l cos beta
__device__ __forceinline__ double double_x2(const DoubleState &s, const DoubleTrig &t) { return (s.x + DP_LEN * t.s1) + DP_L * t.sb; }
__device__ __forceinline__ double double_y2(const DoubleTrig &t) { return DP_LEN * t.c1 + DP_L * t.cb; }

__device__ __forceinline__ void double_obs_from(const DoubleState &s, const DoubleTrig &t, float (&o)[9])
{
    o[0] = (float)s.x;
    o[1] = (float)s.v;
    o[2] = (float)double_x2(s, t);
    o[3] = (float)t.c1;
    o[4] = (float)t.s1;
    o[5] = (float)s.w1;
    o[6] = (float)t.c2;
    o[7] = (float)t.s2;
    o[8] = (float)s.w2;
}

// Gaussian elimination without pivoting in the order written (the matrix is symmetric positive definite); one reciprocal per
// pivot -- the first a constant, the third the final division itself -- and the eliminated (3, 2) entry is taken equal to (2, 3)
__device__ __forceinline__ void double_advance(DoubleState &s, const DoubleTrig &t, double a)
{
    const double force = DP_FORCE * clip_ieee(a, -1.0, 1.0);
    const double wa = s.w1, wb = s.w1 + s.w2;
    const double wa2 = wa * wa, wb2 = wb * wb;
    const double a12 = DP_D4 * t.c1, a13 = DP_D5 * t.cb, a23 = DP_D6 * t.c2;
    const double b1 = (force + (DP_D4 * wa2) * t.s1) + (DP_D5 * wb2) * t.sb;
    const double b2 = (PB_G * DP_D4) * t.s1 + (DP_D6 * wb2) * t.s2;
    const double b3 = (PB_G * DP_D5) * t.sb - (DP_D6 * wa2) * t.s2;
    const double m2 = a12 * DP_R1, m3 = a13 * DP_R1;
    const double e22 = DP_D2 - m2 * a12, e23 = a23 - m2 * a13, f2 = b2 - m2 * b1;
    const double e33 = DP_D3 - m3 * a13, f3 = b3 - m3 * b1;
    const double r2 = 1.0 / e22;
    const double m32 = e23 * r2;
    const double g33 = e33 - m32 * e23, h3 = f3 - m32 * f2;
    const double bacc = h3 / g33;
    const double aacc = (f2 - e23 * bacc) * r2;
    const double xacc = ((b1 - a12 * aacc) - a13 * bacc) * DP_R1;
    s.v = s.v + PB_DT * xacc;
    s.w1 = s.w1 + PB_DT * aacc;
    s.w2 = s.w2 + PB_DT * (bacc - aacc);
    s.x = s.x + PB_DT * s.v;
    s.th1 = s.th1 + PB_DT * s.w1;
    s.th2 = s.th2 + PB_DT * s.w2;
    pendula_rail(s.x, s.v);
}

// ---- the adapters the kernels are templated on ----------------------------------------------------------------------------
// Trig envs of the contract in ses_classic.h: step_from is advance from the trig of the state it leaves, the trig of the state
// it enters, and that state's outcome.
template <class EnvP>
struct PendulaEnv : TrigEnv<EnvP> {
    template <class St, class Tg>
    __device__ static __forceinline__ double step_from(St &s, Tg &t, const float (&act)[1], bool &done)
    {
        EnvP::advance(s, t, (double)act[0]);
        EnvP::trig(s, t);
        return EnvP::outcome(s, t, done);
    }
};

struct InvertedPendulumEnv : PendulaEnv<InvertedPendulumEnv> {
    static constexpr int S = 5, A = 1, INIT_W = IP_INIT_W;
    static constexpr bool TERMINATES = true;
    static constexpr const char *NAME = "InvertedPendulum";
    using State = PoleState;
    using Trig = PoleTrig;
    using Action = float[A];
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u) { s = State{0.0, 0.0, (double)u[0], 0.0}; }
    __device__ static __forceinline__ void trig(const State &s, Trig &t) { pole_trig(s, t); }
    __device__ static __forceinline__ void observe_from(const State &s, const Trig &t, float (&o)[S]) { pole_obs_from(s, t, o); }
    __device__ static __forceinline__ void advance(State &s, const Trig &t, double a) { pole_advance(s, t, a); }
    __device__ static __forceinline__ double outcome(const State &s, const Trig &, bool &done)
    {
        done = s.th > IP_FALL || s.th < -IP_FALL;
        return 1.0;
    }
};

struct PendulumSwingupEnv : PendulaEnv<PendulumSwingupEnv> {
    static constexpr int S = 5, A = 1, INIT_W = IP_INIT_W;
    static constexpr bool TERMINATES = false;
    static constexpr const char *NAME = "InvertedPendulumSwingup";
    using State = PoleState;
    using Trig = PoleTrig;
    using Action = float[A];
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u)
    {
        s = State{0.0, 0.0, IP_SWINGUP_TH0 + (double)u[0], 0.0};
    }
    __device__ static __forceinline__ void trig(const State &s, Trig &t) { pole_trig(s, t); }
    __device__ static __forceinline__ void observe_from(const State &s, const Trig &t, float (&o)[S]) { pole_obs_from(s, t, o); }
    __device__ static __forceinline__ void advance(State &s, const Trig &t, double a) { pole_advance(s, t, a); }
    __device__ static __forceinline__ double outcome(const State &, const Trig &t, bool &done)
    {
        done = false;
        return t.cs;
    }
};

struct DoublePendulumEnv : PendulaEnv<DoublePendulumEnv> {
    static constexpr int S = 9, A = 1, INIT_W = DP_INIT_W;
    static constexpr bool TERMINATES = true;
    static constexpr const char *NAME = "InvertedDoublePendulum";
    using State = DoubleState;
    using Trig = DoubleTrig;
    using Action = float[A];
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u)
    {
        s = State{0.0, 0.0, (double)u[0], 0.0, (double)u[1], 0.0};
    }
    __device__ static __forceinline__ void trig(const State &s, Trig &t) { double_trig(s, t); }
    __device__ static __forceinline__ void observe_from(const State &s, const Trig &t, float (&o)[S]) { double_obs_from(s, t, o); }
    __device__ static __forceinline__ void advance(State &s, const Trig &t, double a) { double_advance(s, t, a); }
    __device__ static __forceinline__ double outcome(const State &s, const Trig &t, bool &done)
    {
        const double x2 = double_x2(s, t);
        const double h = double_y2(t) + 0.3;
        const double d = h - 2.0;
        done = h <= 1.0;
        return (10.0 - 0.01 * (x2 * x2)) - d * d;
    }
};

}  // namespace ses
