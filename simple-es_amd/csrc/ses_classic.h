// ses_classic.h -- gym 0.21's classic-control envs in float64: Acrobot-v1 and MountainCar-v0 (discrete actions), Pendulum-v1
// and MountainCarContinuous-v0 (continuous actions; DESIGN.md 7 holds their equations, which are the specification).  All
// four are restated in gym's own order of operations (Python's left-to-right evaluation) so that tests/classic_control_np.py
// and tests/classic_control_cont_np.py -- independent numpy float64 restatements -- reproduce every transition bit for bit.
//
// The state lives in float64 between steps as in gym; observations are cast to float32 as gym's _get_ob does.  Every
// operation is a plain correctly rounded IEEE-754 add, sub, mul, div or compare: the build passes -ffp-contract=off, f64
// division is correctly rounded on gfx950, and the sin / cos below use no fma -- numpy cannot restate an fma exactly,
// which is why ses_math.h's sincos64_ (fma-based, for the float64 CartPole) is not used here.
//
// A discrete env takes an action index and its reward is exact in float.  A continuous env takes the policy's float32 tanh
// output widened to double, and its reward is a float64 that depends on it (gym returns a Python float, the reference's
// RolloutWorker adds it up in float64).
//
// Parity with gym itself is UNPINNED: gym is not part of the reference tree, and these envs are checked against the
// restatement of its published source in tests/, not against gym.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ses {

// ---- the adapter contract of the float64 envs (this header, ses_pendula.h, ses_reacher.h; the kernels of ses_f64_envs.hip) ----
// Every adapter has
//   S, A, INIT_W      widths of the observation, of the policy's output and of an init row
//   NAME              what error texts call the env
//   State             the float64 state, which is the step-wise blob
//   Action            what marks the kind: int -- an index into gym's Discrete(3), the policy's first argmax, the reward a float
//                     (exact) -- or float[A] -- the policy's tanh outputs, which the env clips; the reward the env's double
//   TERMINATES        false: step never sets done, a rollout carries no alive flag, no ballot and no frozen state
//   HAS_TRIG          whether the adapter is a trig env (below); one that is not derives from NoTrigEnv
//   reset(s, u)       from an init row
//   observe(s, o)     float32, as gym's _get_ob casts
//   step(s, action, done) -> reward
// A TRIG ENV splits a transition so that a fused rollout evaluates the sincos_ieee calls of a state once, when the state is
// entered: they give the outcome of the step that entered it and, one iteration later, the observation and the dynamics of the
// step that leaves it -- the bits are the same, which is what makes it legal.  It has in addition
//   Trig, trig(s, t)              the sincos_ieee of every angle of s (and what the addition formulas make of them)
//   observe_from(s, t, o)         t the trig of s
//   step_from(s, t, act, done)    on entry t is the trig of s, on exit the trig of the new s; returns the reward
//   TRIG_ON_EXIT                  true unless the adapter says otherwise.  An env whose outcome reads no trig of the state entered
//                                 may set it false: step_from then leaves t alone and the rollout evaluates trig(s, t) at the top
//                                 of the next step instead -- once per step either way, in the other instruction order
// and derives from TrigEnv, which writes observe and step with these pieces: an observation costs one trig, a step the trig of
// the state it leaves and -- where the outcome reads it -- of the one it enters.
struct NoTrigEnv {
    static constexpr bool HAS_TRIG = false;
    struct Trig {};                                  // (what the rollout declares and, without the one-trig form, never uses)
};

template <class Env>
struct TrigEnv {
    static constexpr bool HAS_TRIG = true, TRIG_ON_EXIT = true;
    template <class St, int N>
    __device__ static __forceinline__ void observe(const St &s, float (&o)[N])
    {
        typename Env::Trig t;
        Env::trig(s, t);
        Env::observe_from(s, t, o);
    }
    template <class St, int N>
    __device__ static __forceinline__ double step(St &s, const float (&act)[N], bool &done)
    {
        typename Env::Trig t;
        Env::trig(s, t);
        return Env::step_from(s, t, act, done);
    }
};

// sin and cos of one double.  Reduction by pi/2 in three Cody-Waite parts: C1 and C2 carry 33 significant bits each, so
// k * C1 and k * C2 are exact for |k| < 2^20 (|x| up to ~1.6e6), and k * C3 (C3 the remaining 53 bits of pi/2) is rounded
// once, an error below 2^-102 at |x| <= 1e3.  Then the Cephes sin.c polynomials on |r| <= pi/4, in Cephes' own order:
//   sin r = r + r * (z * P(z)),  cos r = (1 - z / 2) + (z * z) * Q(z),  z = r * r,
// and the quadrant k mod 4 picks and signs the pair.  Within 2 ulp of a correctly rounded sin / cos on [-1e3, 1e3]
// (tests/test_classic_control_host.py).  The envs' arguments stay below ~16 in magnitude.
__device__ __forceinline__ void sincos_ieee(double x, double &s_out, double &c_out)
{
    const double k = __builtin_rint(x * 0x1.45f306dc9c883p-1);       // x * (2 / pi), to nearest even
    double r = x - k * 0x1.921fb544p+0;
    r = r - k * 0x1.0b4611a6p-34;
    r = r - k * 0x1.3198a2e037073p-69;
    const double z = r * r;
    double ps = 1.58962301576546568060E-10;
    ps = ps * z + -2.50507477628578072866E-8;
    ps = ps * z + 2.75573136213857245213E-6;
    ps = ps * z + -1.98412698295895385996E-4;
    ps = ps * z + 8.33333333332211858878E-3;
    ps = ps * z + -1.66666666666666307295E-1;
    const double s = r + r * (z * ps);
    double pc = -1.13585365213876817300E-11;
    pc = pc * z + 2.08757008419747316778E-9;
    pc = pc * z + -2.75573141792967388112E-7;
    pc = pc * z + 2.48015872888517045348E-5;
    pc = pc * z + -1.38888888888730564116E-3;
    pc = pc * z + 4.16666666666665929218E-2;
    const double c = (1.0 - 0.5 * z) + (z * z) * pc;
    const double kc = k < -1.0e9 ? -1.0e9 : (k > 1.0e9 ? 1.0e9 : k);   // (NaN: q = 0, the NaN propagates through r)
    const int32_t q = (int32_t)kc;
    const double sv = (q & 1) ? c : s;
    const double cv = (q & 1) ? s : c;
    s_out = (q & 2) ? -sv : sv;
    c_out = ((q + 1) & 2) ? -cv : cv;
}

__device__ __forceinline__ double cos_ieee(double x)
{
    double s, c;
    sincos_ieee(x, s, c);
    return c;
}

// ---- Acrobot-v1 (gym/envs/classic_control/acrobot.py, "book" dynamics, no torque noise) --------------------------------
constexpr double AC_DT = 0.2;
constexpr double AC_M1 = 1.0, AC_M2 = 1.0, AC_L1 = 1.0, AC_LC1 = 0.5, AC_LC2 = 0.5, AC_I1 = 1.0, AC_I2 = 1.0, AC_G = 9.8;
constexpr double AC_PI = 3.141592653589793;
constexpr double AC_MAX_VEL_1 = 4.0 * AC_PI, AC_MAX_VEL_2 = 9.0 * AC_PI;
constexpr int AC_INIT_W = 4;                 // init row: theta1, theta2, dtheta1, dtheta2 ~ U(-0.1, 0.1)
constexpr int AC_WRAP_MAX = 4096;            // bound on gym's wrap loop: |theta| < ~2.5e4 wraps exactly; an inf cannot hang a lane

struct AcrobotState {
    double th1, th2, w1, w2;
};

// _dsdt: the time derivative of (theta1, theta2, dtheta1, dtheta2) under torque a
__device__ __forceinline__ void acrobot_dsdt(double th1, double th2, double w1, double w2, double a, double (&d)[4])
{
    double s2, c2;
    sincos_ieee(th2, s2, c2);
    const double d1 = AC_M1 * (AC_LC1 * AC_LC1) + AC_M2 * ((AC_L1 * AC_L1 + AC_LC2 * AC_LC2) + ((2.0 * AC_L1) * AC_LC2) * c2) + AC_I1 + AC_I2;
    const double d2 = AC_M2 * (AC_LC2 * AC_LC2 + (AC_L1 * AC_LC2) * c2) + AC_I2;
    const double phi2 = ((AC_M2 * AC_LC2) * AC_G) * cos_ieee((th1 + th2) - AC_PI / 2.0);
    const double phi1 = ((((-AC_M2) * AC_L1) * AC_LC2) * (w2 * w2)) * s2 - (((((2.0 * AC_M2) * AC_L1) * AC_LC2) * w2) * w1) * s2 +
                        ((AC_M1 * AC_LC1 + AC_M2 * AC_L1) * AC_G) * cos_ieee(th1 - AC_PI / 2.0) + phi2;
    const double dd2 = (((a + (d2 / d1) * phi1) - (((AC_M2 * AC_L1) * AC_LC2) * (w1 * w1)) * s2) - phi2) /
                       ((AC_M2 * (AC_LC2 * AC_LC2) + AC_I2) - (d2 * d2) / d1);
    const double dd1 = -(d1 * dd2 + phi1) / d1;
    d[0] = w1;
    d[1] = w2;
    d[2] = dd1;
    d[3] = dd2;
}

__device__ __forceinline__ double acrobot_wrap(double x)
{
    const double diff = AC_PI - (-AC_PI);
    for (int i = 0; i < AC_WRAP_MAX && x > AC_PI; ++i) x = x - diff;
    for (int i = 0; i < AC_WRAP_MAX && x < -AC_PI; ++i) x = x + diff;
    return x;
}

__device__ __forceinline__ double acrobot_bound(double x, double m) { return x < -m ? -m : (x > m ? m : x); }   // min(max(x, -m), m)

__device__ __forceinline__ bool acrobot_terminal(const AcrobotState &s)
{
    return -cos_ieee(s.th1) - cos_ieee(s.th2 + s.th1) > 1.0;
}

// one env.step(a), a in {0, 1, 2}: rk4 over [0, dt] on (state, torque), wrap, bound; returns done (reward: -1, 0 when done)
__device__ __forceinline__ bool acrobot_step(AcrobotState &s, int a)
{
    const double tau = a == 0 ? -1.0 : (a == 2 ? 1.0 : 0.0);
    const double dt = AC_DT - 0.0, dt2 = dt / 2.0;
    const double y0[4] = {s.th1, s.th2, s.w1, s.w2};
    double k1[4], k2[4], k3[4], k4[4], y[4];
    acrobot_dsdt(y0[0], y0[1], y0[2], y0[3], tau, k1);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = y0[i] + dt2 * k1[i];
    acrobot_dsdt(y[0], y[1], y[2], y[3], tau, k2);        // the torque component: tau + dt2 * 0 = tau
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = y0[i] + dt2 * k2[i];
    acrobot_dsdt(y[0], y[1], y[2], y[3], tau, k3);
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = y0[i] + dt * k3[i];
    acrobot_dsdt(y[0], y[1], y[2], y[3], tau, k4);
    const double h = dt / 6.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) y[i] = y0[i] + h * (((k1[i] + 2.0 * k2[i]) + 2.0 * k3[i]) + k4[i]);
    s.th1 = acrobot_wrap(y[0]);
    s.th2 = acrobot_wrap(y[1]);
    s.w1 = acrobot_bound(y[2], AC_MAX_VEL_1);
    s.w2 = acrobot_bound(y[3], AC_MAX_VEL_2);
    return acrobot_terminal(s);
}

__device__ __forceinline__ void acrobot_obs(const AcrobotState &s, float (&o)[6])
{
    double s1, c1, s2, c2;
    sincos_ieee(s.th1, s1, c1);
    sincos_ieee(s.th2, s2, c2);
    o[0] = (float)c1; o[1] = (float)s1; o[2] = (float)c2; o[3] = (float)s2;
    o[4] = (float)s.w1; o[5] = (float)s.w2;
}

__device__ __forceinline__ AcrobotState acrobot_reset(const float *__restrict__ u)
{
    return AcrobotState{(double)u[0], (double)u[1], (double)u[2], (double)u[3]};
}

// ---- MountainCar-v0 (gym/envs/classic_control/mountain_car.py) ----------------------------------------------------------
constexpr double MC_FORCE = 0.001, MC_GRAVITY = 0.0025, MC_MAX_SPEED = 0.07;
constexpr double MC_MIN_POS = -1.2, MC_MAX_POS = 0.6, MC_GOAL_POS = 0.5, MC_GOAL_VEL = 0.0;
constexpr int MC_INIT_W = 1;                 // init row: position ~ U(-0.6, -0.4); velocity 0

struct MountainCarState {
    double p, v;
};

__device__ __forceinline__ bool mountaincar_step(MountainCarState &s, int a)
{
    double v = s.v + ((double)(a - 1) * MC_FORCE + cos_ieee(3.0 * s.p) * (-MC_GRAVITY));
    v = v < -MC_MAX_SPEED ? -MC_MAX_SPEED : (v > MC_MAX_SPEED ? MC_MAX_SPEED : v);
    double p = s.p + v;
    p = p < MC_MIN_POS ? MC_MIN_POS : (p > MC_MAX_POS ? MC_MAX_POS : p);
    if (p == MC_MIN_POS && v < 0.0) v = 0.0;
    s.p = p;
    s.v = v;
    return p >= MC_GOAL_POS && v >= MC_GOAL_VEL;
}

__device__ __forceinline__ void mountaincar_obs(const MountainCarState &s, float (&o)[2])
{
    o[0] = (float)s.p;
    o[1] = (float)s.v;
}

__device__ __forceinline__ MountainCarState mountaincar_reset(const float *__restrict__ u)
{
    return MountainCarState{(double)u[0], 0.0};
}

__device__ __forceinline__ double clip_ieee(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }   // min(max(x, lo), hi)

// ---- Pendulum-v1 ------------------------------------------------------------------------------------------------------------
constexpr double PD_PI = 3.141592653589793, PD_TWO_PI = 2.0 * PD_PI;
constexpr double PD_MAX_SPEED = 8.0, PD_MAX_TORQUE = 2.0, PD_DT = 0.05;
constexpr double PD_GRAV = 15.0, PD_INERTIA = 3.0;   // 3 g / (2 l) and 3 / (m l^2) at g = 10, m = l = 1
constexpr int PD_INIT_W = 2;                         // init row: u0, u1 ~ U(-1, 1): th = u0 * pi, w = u1

struct PendulumState {
    double th, w;
};

// Python's x % (2 pi) (numpy's np.remainder): C fmod, then the sign adjustment -- a result in [0, 2 pi).  fmod is exact, so any
// exact evaluation has its bits.  Below 16 periods (|th| < ~97; a rollout stays below 84) it is four shift-and-subtract steps:
// each subtracts 2^j periods from a value in [2^j, 2^(j+1)) periods, exact by Sterbenz' lemma, as is the power-of-two multiple
// of the period.  Anything larger (a state blob a caller wrote) goes through fmod itself.
__device__ __forceinline__ double pendulum_mod_two_pi(double x)
{
    double a = __builtin_fabs(x);
    if (a < 16.0 * PD_TWO_PI) {
        a = a >= 8.0 * PD_TWO_PI ? a - 8.0 * PD_TWO_PI : a;
        a = a >= 4.0 * PD_TWO_PI ? a - 4.0 * PD_TWO_PI : a;
        a = a >= 2.0 * PD_TWO_PI ? a - 2.0 * PD_TWO_PI : a;
        a = a >= PD_TWO_PI ? a - PD_TWO_PI : a;
    } else {
        a = fmod(a, PD_TWO_PI);                      // (inf, NaN -> NaN, as Python's)
    }
    const double r = x < 0.0 ? -a : a;               // fmod(x, m) carries x's sign
    return r < 0.0 ? r + PD_TWO_PI : (r == 0.0 ? 0.0 : r);
}

// one env.step(a) given sin(th) of the CURRENT angle -- the observation of this state needed the same sincos_ieee(th), and a
// fused rollout passes it on instead of evaluating it again; returns the float64 reward.  The env never terminates.
__device__ __forceinline__ double pendulum_step_sin(PendulumState &s, double sin_th, double a)
{
    const double u = clip_ieee(a, -PD_MAX_TORQUE, PD_MAX_TORQUE);
    const double an = pendulum_mod_two_pi(s.th + PD_PI) - PD_PI;
    const double cost = (an * an + 0.1 * (s.w * s.w)) + 0.001 * (u * u);
    double w = s.w + ((PD_GRAV * sin_th) + (PD_INERTIA * u)) * PD_DT;
    w = clip_ieee(w, -PD_MAX_SPEED, PD_MAX_SPEED);
    s.th = s.th + w * PD_DT;
    s.w = w;
    return -cost;
}

__device__ __forceinline__ void pendulum_obs_from(double sin_th, double cos_th, const PendulumState &s, float (&o)[3])
{
    o[0] = (float)cos_th;
    o[1] = (float)sin_th;
    o[2] = (float)s.w;
}

__device__ __forceinline__ PendulumState pendulum_reset(const float *__restrict__ u)
{
    return PendulumState{(double)u[0] * PD_PI, (double)u[1]};
}

// ---- MountainCarContinuous-v0 -----------------------------------------------------------------------------------------------
constexpr double MCC_POWER = 0.0015, MCC_GRAVITY = 0.0025, MCC_MAX_SPEED = 0.07;
constexpr double MCC_MIN_POS = -1.2, MCC_MAX_POS = 0.6, MCC_GOAL_POS = 0.45, MCC_GOAL_VEL = 0.0;
constexpr int MCC_INIT_W = 1;                        // init row: position ~ U(-0.6, -0.4); velocity 0

// one env.step(a): returns the float64 reward, which charges the UNclipped action; the state is kept float32-representable
// (gym 0.21 keeps this env's state as a float32 array; float64 arithmetic on it is the build's definition)
__device__ __forceinline__ double mountaincar_cont_step(MountainCarState &s, double a, bool &done)
{
    const double f = clip_ieee(a, -1.0, 1.0);
    double v = s.v + (f * MCC_POWER - MCC_GRAVITY * cos_ieee(3.0 * s.p));
    v = clip_ieee(v, -MCC_MAX_SPEED, MCC_MAX_SPEED);
    double p = s.p + v;
    p = clip_ieee(p, MCC_MIN_POS, MCC_MAX_POS);
    if (p == MCC_MIN_POS && v < 0.0) v = 0.0;
    done = p >= MCC_GOAL_POS && v >= MCC_GOAL_VEL;
    const double reward = (done ? 100.0 : 0.0) - (a * a) * 0.1;
    s.p = (double)(float)p;
    s.v = (double)(float)v;
    return reward;
}


// ---- the adapters the kernels are templated on (the contract at the top of this header) -----------------------------------
struct AcrobotEnv : NoTrigEnv {
    static constexpr int S = 6, A = 3, INIT_W = AC_INIT_W;
    static constexpr bool TERMINATES = true;
    static constexpr const char *NAME = "Acrobot";
    using State = AcrobotState;
    using Action = int;
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u) { s = acrobot_reset(u); }
    __device__ static __forceinline__ void observe(const State &s, float (&o)[S]) { acrobot_obs(s, o); }
    __device__ static __forceinline__ float step(State &s, int a, bool &done)
    {
        done = acrobot_step(s, a);
        return done ? 0.0f : -1.0f;
    }
};

struct MountainCarEnv : NoTrigEnv {
    static constexpr int S = 2, A = 3, INIT_W = MC_INIT_W;
    static constexpr bool TERMINATES = true;
    static constexpr const char *NAME = "MountainCar";
    using State = MountainCarState;
    using Action = int;
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u) { s = mountaincar_reset(u); }
    __device__ static __forceinline__ void observe(const State &s, float (&o)[S]) { mountaincar_obs(s, o); }
    __device__ static __forceinline__ float step(State &s, int a, bool &done)
    {
        done = mountaincar_step(s, a);
        return -1.0f;
    }
};

// The env never terminates.  One step needs sin th for the dynamics and (cos th, sin th) for the observation of the SAME
// angle: the trig of a state is one sincos_ieee.  The reward reads no trig of the state entered, so TRIG_ON_EXIT is false: the
// one-trig loop evaluates the sincos at the top of the step that uses it, which is the instruction order of the kernel once
// written out by hand for this env; carried over from the end of the step before, the same sincos measured 2 ... 3 % slower
// (profiles/f64_envs_refactor_timing.txt).  The step is one float64 dependence chain -- sincos (~25 f64 ops deep), the policy,
// the torque, th' -- and the cost term (the exact mod, three squares) hangs off its side: latency, not issue, is what a small
// population pays.
struct PendulumEnv : TrigEnv<PendulumEnv> {
    static constexpr int S = 3, A = 1, INIT_W = PD_INIT_W;
    static constexpr bool TERMINATES = false, TRIG_ON_EXIT = false;
    static constexpr const char *NAME = "Pendulum";
    using State = PendulumState;
    struct Trig {
        double sn, cs;
    };
    using Action = float[A];
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u) { s = pendulum_reset(u); }
    __device__ static __forceinline__ void trig(const State &s, Trig &t) { sincos_ieee(s.th, t.sn, t.cs); }
    __device__ static __forceinline__ void observe_from(const State &s, const Trig &t, float (&o)[S]) { pendulum_obs_from(t.sn, t.cs, s, o); }
    __device__ static __forceinline__ double step_from(State &s, Trig &t, const float (&act)[A], bool &done)
    {
        done = false;
        return pendulum_step_sin(s, t.sn, (double)act[0]);
    }
};

struct MountainCarContEnv : NoTrigEnv {
    static constexpr int S = 2, A = 1, INIT_W = MCC_INIT_W;
    static constexpr bool TERMINATES = true;
    static constexpr const char *NAME = "MountainCarContinuous";
    using State = MountainCarState;
    using Action = float[A];
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u) { s = mountaincar_reset(u); }
    __device__ static __forceinline__ void observe(const State &s, float (&o)[S]) { mountaincar_obs(s, o); }
    __device__ static __forceinline__ double step(State &s, const float (&act)[A], bool &done)
    {
        return mountaincar_cont_step(s, (double)act[0], done);
    }
};

}  // namespace ses
