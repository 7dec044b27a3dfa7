// ses_classic.hip -- gym's discrete classic-control envs Acrobot-v1 and MountainCar-v0 (csrc/ses_classic.h: float64, gym's
// order of operations) on the device, through every path the other envs have:
//   k_envs_reset_classic / k_envs_step_classic : env.reset() / env.step(a) for n independent envs (ses_env_reset /
//                                                ses_env_step_generic), one lane per env, the blob is the float64 state
//   k_rollout_classic_mlp                      : RolloutWorker (loop.py:108-125) with an MLP policy, one kernel per shard
//   k_rollout_gru_lockstep<AcrobotLs / ...>    : the same with a GRU policy, the lockstep kernel of ses_gru_lockstep.h
//   k_policy_forward_mlp / _gru<6 or 2, 3>     : ses_policy_forward for these shapes (GymEnvModel.forward, playback)
// Episodic mode only.  A unit of its own: the kernels of the other units keep their machine code byte for byte.
#include "ses_classic.h"
#include "ses_gru_lockstep.h"
#include "ses_internal.h"
#include "ses_policy.h"
#include "ses_policy_forward.h"

namespace ses {

// ---- step-wise envs -----------------------------------------------------------------------------------------------------
template <class EnvC>
__global__ __launch_bounds__(64) void k_envs_reset_classic(const float *__restrict__ init, int n, typename EnvC::State *__restrict__ state,
                                                           float *__restrict__ obs)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    typename EnvC::State st;
    EnvC::reset(st, init + (size_t)i * EnvC::INIT_W);
    state[i] = st;
    float o[EnvC::S];
    EnvC::observe(st, o);
#pragma unroll
    for (int k = 0; k < EnvC::S; ++k) obs[(size_t)i * EnvC::S + k] = o[k];
}

template <class EnvC>
__global__ __launch_bounds__(64) void k_envs_step_classic(typename EnvC::State *__restrict__ state, const int32_t *__restrict__ action,
                                                          int n, float *__restrict__ obs, float *__restrict__ reward,
                                                          int32_t *__restrict__ done)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    typename EnvC::State st = state[i];
    const int a = action[i];
    bool d;
    const float r = EnvC::step(st, a < 0 ? 0 : (a > 2 ? 2 : a), d);   // (gym's action spaces are {0, 1, 2}: clamped into it)
    state[i] = st;
    float o[EnvC::S];
    EnvC::observe(st, o);
#pragma unroll
    for (int k = 0; k < EnvC::S; ++k) obs[(size_t)i * EnvC::S + k] = o[k];
    reward[i] = r;
    done[i] = d ? 1 : 0;
}

// ---- fused MLP rollout ----------------------------------------------------------------------------------------------------
// LPE adjacent lanes share one env (env = row * E + episode) as in k_rollout_box2d_mlp without the terrain: every lane of
// the group runs the env's physics (identical bits), the MLP is split over the group -- MlpSlice with the offspring's slice
// in registers for 4 ... 32 lanes per env, streamed from the (L2-resident) row for 1 and 2.  A finished env is frozen, the
// wave leaves as soon as none of its envs is alive.  One env step is a chain of ~15 sin / cos and 16 f64 divisions behind
// four sequential RK4 stages (Acrobot): at the populations ES uses the chip holds far fewer envs than lanes, so the step's
// dependence chain, not issue, is what a rollout costs -- the lanes per env only decide how many waves (and SIMDs) share
// the population and how short the policy's part of the chain is (classic_lanes_per_env).
template <class EnvC, int LPE>
__global__ __launch_bounds__(64) void k_rollout_classic_mlp(const float *__restrict__ theta, const float *__restrict__ init,
                                                            int init_per_offspring, int n_rows, int E, int P, int max_step,
                                                            double *__restrict__ ep_return, int32_t *__restrict__ ep_steps)
{
    constexpr int S = EnvC::S, A = EnvC::A;
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    stage_tanh_table(tanh_tab);
    const long long n_env = (long long)n_rows * E;
    long long env = ((long long)blockIdx.x * 64 + threadIdx.x) / LPE;
    const int sub = (int)(threadIdx.x % LPE);
    const bool valid = env < n_env;
    env = valid ? env : n_env - 1;                                  // lane groups past the last env shadow it
    const int row = (int)(env / E), ep = (int)(env - (long long)row * E);
    const float *th = theta + (size_t)row * P;
    typename EnvC::State st;
    EnvC::reset(st, init + ((size_t)(init_per_offspring ? row : 0) * E + ep) * EnvC::INIT_W);
    MlpSlice<S, A, (LPE >= 4 ? LPE : 4)> net;
    if constexpr (LPE >= 4) net.load(th, sub);
    double ret = 0.0;
    int steps = 0;
    bool done = false;
    for (int t = 0; t < max_step; ++t) {
        if (__ballot(!done) == 0ull) break;
        float obs[S], logits[A];
        EnvC::observe(st, obs);
        if constexpr (LPE >= 4) net.forward(tanh_tab, obs, logits);
        else mlp_forward_streamed<S, A, LPE>(th, sub, tanh_tab, obs, logits);
        const int action = argmax_first<A>(logits);
        if (!done) {
            ret += (double)EnvC::step(st, action, done);
            steps += 1;
        }
    }
    if (valid && sub == 0) {
        ep_return[env] = ret;
        if (ep_steps) ep_steps[env] = steps;
    }
}

// ---- GRU adapters of the lockstep kernel (the CartPoleLs interface, ses_rollout.hip) -------------------------------------
template <class EnvC>
struct ClassicLs {
    static constexpr int S = EnvC::S, A = EnvC::A, INIT_W = EnvC::INIT_W;
    struct State {
        typename EnvC::State st;
    };
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u, int) { EnvC::reset(s.st, u); }
    __device__ static __forceinline__ void observe(const State &s, float (&obs)[S]) { EnvC::observe(s.st, obs); }
    __device__ static __forceinline__ float step(State &s, const float (&logits)[A], const TanhEntry *, bool freeze, bool &done)
    {
        typename EnvC::State ns = s.st;
        const float r = EnvC::step(ns, argmax_first<A>(logits), done);
        if (!freeze) s.st = ns;                                     // a finished env is frozen
        return r;
    }
};
using AcrobotLs = ClassicLs<AcrobotEnv>;
using MountainCarLs = ClassicLs<MountainCarEnv>;

// ---- host side -----------------------------------------------------------------------------------------------------------
static bool is_acrobot(const ses_handle *h) { return h->cfg.env_id == SES_ENV_ACROBOT; }

int classic_env_state_bytes(const ses_handle *h)
{
    return is_acrobot(h) ? (int)sizeof(AcrobotState) : (int)sizeof(MountainCarState);
}

int classic_env_obs_width(const ses_handle *h) { return is_acrobot(h) ? AcrobotEnv::S : MountainCarEnv::S; }

int classic_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs)
{
    const dim3 grid(ceil_div(n, 64)), block(64);
    if (is_acrobot(h))
        hipLaunchKernelGGL(k_envs_reset_classic<AcrobotEnv>, grid, block, 0, h->stream, init, n, (AcrobotState *)state, obs);
    else
        hipLaunchKernelGGL(k_envs_reset_classic<MountainCarEnv>, grid, block, 0, h->stream, init, n, (MountainCarState *)state, obs);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int classic_env_step(ses_handle *h, void *state, const int32_t *action, int n, float *obs, float *reward, int32_t *done)
{
    const dim3 grid(ceil_div(n, 64)), block(64);
    if (is_acrobot(h))
        hipLaunchKernelGGL(k_envs_step_classic<AcrobotEnv>, grid, block, 0, h->stream, (AcrobotState *)state, action, n, obs, reward,
                           done);
    else
        hipLaunchKernelGGL(k_envs_step_classic<MountainCarEnv>, grid, block, 0, h->stream, (MountainCarState *)state, action, n, obs,
                           reward, done);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

// Lanes per env of the MLP rollout (cfg.lanes_per_env overrides): the largest split up to 16 that keeps the population within
// a wave budget -- 1024 waves for Acrobot, 2048 for MountainCar.  Every lane of an env's group repeats the env's physics, so
// more lanes per env buy a shorter policy step and fewer envs per wave (an earlier exit) only while the chip has issue slots
// to spare for the copies.  Measured (profiles/classic_control_timing.txt, tools/time_classic.py; 5 episodes, random
// first-generation policies): Acrobot 97 offspring 1.32 ms at 16 or 32 lanes per env against 1.53 at 8; 4096 offspring
// 2.30 ms at 2 against 2.44 / 2.55 / 3.54 at 1 / 4 / 8 -- its 16 f64 divisions and ~15 sin / cos per step make the copies
// cost issue there; MountainCar 240 offspring 0.083 ms at 16 (0.089 / 0.091 at 8 / 32); 4096 offspring 0.151 ms at 4
// (0.170 / 0.273 at 8 / 2).
int classic_lanes_per_env(const ses_handle *h, long long episodes)
{
    if (h->cfg.lanes_per_env) return h->cfg.lanes_per_env;
    const long long budget = is_acrobot(h) ? 1024 : 2048;
    int lpe = 16;
    while (lpe > 1 && (episodes * lpe + 63) / 64 > budget) lpe >>= 1;
    return lpe;
}

// (first-use order of the kernel instances, see ses_internal.h: the GRU kernels Acrobot, MountainCar; then the MLP kernels
// Acrobot 1 ... 32 lanes per env, MountainCar 1 ... 32)
template <class EnvC>
static int launch_classic_mlp(const ses_handle *h, const RolloutArgs &a)
{
    const int lpe = classic_lanes_per_env(h, a.episodes());
    const dim3 grid(ceil_div(a.episodes() * lpe, 64)), block(64);
    const bool known = with_lanes<1, 2, 4, 8, 16, 32>(lpe, [&](auto lanes) {
        hipLaunchKernelGGL((k_rollout_classic_mlp<EnvC, lanes()>), grid, block, 0, h->stream, a.theta, a.init, a.per, a.n_rows, a.E,
                           a.P, a.max_step, a.epr, a.ep_steps);
    });
    if (!known)
        return set_error(SES_ERR_INVALID_ARG, "ses_rollout: %s has no MLP rollout at %d lanes per env (1, 2, 4, 8, 16, 32)",
                         h->cfg.env_id == SES_ENV_ACROBOT ? "Acrobot" : "MountainCar", lpe);
    return SES_OK;
}

int classic_rollout(const ses_handle *h, const RolloutArgs &a, int mode)
{
    SES_REQUIRE(mode == SES_MODE_EPISODIC, "ses_rollout: %s has no fixed-length mode", is_acrobot(h) ? "Acrobot" : "MountainCar");
    if (h->cfg.gru) {
        const dim3 grid(ceil_div(a.n_rows, 4)), block(256);
        if (is_acrobot(h)) launch_rollout_kernel(h, k_rollout_gru_lockstep<AcrobotLs, false, 4>, grid, block, a);
        else launch_rollout_kernel(h, k_rollout_gru_lockstep<MountainCarLs, false, 4>, grid, block, a);
    } else {
        const int rc = is_acrobot(h) ? launch_classic_mlp<AcrobotEnv>(h, a) : launch_classic_mlp<MountainCarEnv>(h, a);
        if (rc != SES_OK) return rc;
    }
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int classic_policy_forward(ses_handle *h, const float *theta, const float *obs, float *hidden, int n, float *logits, float *act,
                           int32_t *action)
{
    const int S = h->cfg.num_state == 6 ? 6 : 2;                // (first-use order: the GRU instances, then the MLP ones)
    if (h->cfg.gru)
        with_policy_shape<PolicyShape<6, 3>, PolicyShape<2, 3>>(S, 3, [&](auto sh) {
            hipLaunchKernelGGL((k_policy_forward_gru<sh.S, sh.A>), dim3(ceil_div(n, 4)), dim3(256), 0, h->stream, theta, obs, hidden, n,
                               h->P, logits, act, action);
        });
    else
        with_policy_shape<PolicyShape<6, 3>, PolicyShape<2, 3>>(S, 3, [&](auto sh) {
            hipLaunchKernelGGL((k_policy_forward_mlp<sh.S, sh.A>), dim3(ceil_div((long long)n * 4, 64)), dim3(64), 0, h->stream, theta,
                               obs, n, h->P, logits, act, action);
        });
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

}  // namespace ses
