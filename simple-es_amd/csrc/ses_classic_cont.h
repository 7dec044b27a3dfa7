// ses_classic_cont.h -- gym 0.21's continuous-action classic-control envs Pendulum-v1 and MountainCarContinuous-v0 in
// float64, restated (DESIGN.md 7 holds the equations; they are the specification) in Python's left-to-right order of
// operations so that tests/classic_control_cont_np.py -- an independent numpy float64 restatement -- reproduces every
// transition bit for bit.
//
// As in ses_classic.h every operation is one correctly rounded IEEE-754 add, sub, mul or compare (-ffp-contract=off), and
// sin / cos are that header's fma-free sincos_ieee.  What is new against the discrete envs: the action is the policy's float32
// tanh output widened to double, and the reward is a float64 that depends on it (gym returns a Python float, the
// reference's RolloutWorker adds it up in float64).  Parity with gym itself is UNPINNED.
#pragma once
#include "ses_classic.h"

namespace ses {

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

// ---- the adapters the kernels are templated on ----------------------------------------------------------------------------
// The interface of ses_classic.h's adapters with a float action VECTOR (the policy's tanh outputs) and a double reward.
struct PendulumEnv {
    static constexpr int S = 3, A = 1, INIT_W = PD_INIT_W;
    using State = PendulumState;
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u) { s = pendulum_reset(u); }
    __device__ static __forceinline__ void observe(const State &s, float (&o)[S])
    {
        double sn, cs;
        sincos_ieee(s.th, sn, cs);
        pendulum_obs_from(sn, cs, s, o);
    }
    __device__ static __forceinline__ double step(State &s, const float (&act)[A], bool &done)
    {
        double sn, cs;
        sincos_ieee(s.th, sn, cs);
        done = false;
        return pendulum_step_sin(s, sn, (double)act[0]);
    }
};

struct MountainCarContEnv {
    static constexpr int S = 2, A = 1, INIT_W = MCC_INIT_W;
    using State = MountainCarState;
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u) { s = mountaincar_reset(u); }
    __device__ static __forceinline__ void observe(const State &s, float (&o)[S]) { mountaincar_obs(s, o); }
    __device__ static __forceinline__ double step(State &s, const float (&act)[A], bool &done)
    {
        return mountaincar_cont_step(s, (double)act[0], done);
    }
};

}  // namespace ses
