// ses_walker2d.hip -- Walker2DBulletEnv-v0: the build's own float32 definition of a planar two-legged walker modelled on
// pybullet_envs' (ses_walker2d_env.h) on the Box2D-style world of ses_b2.h: seven bodies, six torque-driven revolute
// joints with limits, both feet in friction contact with flat ground, 4 world steps of 8 + 3 iterations per env step.
//   k_w2d_mlp<LPE>            : fused rollout, MLP policy, LPE lanes per env (the shape of k_hop_mlp)
//   k_w2d_gru_ls              : fused rollout, GRU policy, the shared lockstep body of ses_gru_lockstep.h
//   k_w2d_env_reset / _step   : the step-wise env, one lane per env, state blob = Walker2dState (ses_env_state_bytes says its size)
//   k_policy_forward_mlp / _gru<22, 6> : ses_policy_forward for this env's shape (playback)
//
// A unit of its own for the reason ses_lander_discrete.hip gives: a kernel added to an existing unit moves that unit's machine
// code.  The env step, w2d_step, is compiled once in this unit as a real function, like hp_step: a world step is as long as a
// small kernel, and compiled once it has its own register allocation and one copy of its code serves every kernel.  The env
// struct is 1316 bytes, nearly twice the hopper's: what of it lives in registers and what in scratch is accounted for in
// DESIGN.md 7 (Walker2D, registers), and WALKER2D_MLP_WAVES_PER_SIMD is the measured choice that follows from it.
// The wave shape of the MLP rollout is the Box2D plan's (ses_rollout_plan.h: box2d_lanes_per_env, box2d_envs_per_wave).
#include "ses_lander.h"          // the B2_* macros of the device build
#include "ses_walker2d_env.h"
#include "ses_env_table.h"
#include "ses_gru_lockstep.h"
#include "ses_internal.h"
#include "ses_policy.h"
#include "ses_policy_forward.h"

namespace ses {

// the env in a rollout's private memory and in the step-wise env's state blob alike: the env struct alone, the ground has no memory
struct Walker2dState {
    b2l::Walker2dEnv env;
};

__device__ __forceinline__ void w2d_obs(const Walker2dState &s, float (&obs)[22]) { b2l::walker2d_obs(s.env, obs); }

// one env step; returns the reward, sets done.  State in the caller's private memory, no wave votes inside: the call may sit
// under any divergence (finished envs do not call).
__device__ __attribute__((noinline)) float w2d_step(Walker2dState &s, const float (&act)[6], bool &done)
{
    b2l::Walker2dEnv e = s.env;
    bool d;
    const float r = b2l::walker2d_step(e, act, d);
    s.env = e;
    done = d;
    return r;
}

__device__ __forceinline__ void w2d_reset(Walker2dState &s, const float *__restrict__ u) { b2l::walker2d_reset(s.env, u); }

// the adapter of the lockstep GRU body (as LanderLs in ses_rollout.hip)
struct Walker2dLs {
    static constexpr int S = 22, A = 6, INIT_W = 6;
    struct State {
        Walker2dState st;
    };
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u, int) { w2d_reset(s.st, u); }
    __device__ static __forceinline__ void observe(const State &s, float (&obs)[S]) { w2d_obs(s.st, obs); }
    __device__ static __forceinline__ float step(State &s, const float (&logits)[A], const TanhEntry *tab, bool freeze, bool &done)
    {
        float act[A];
#pragma unroll
        for (int k = 0; k < A; ++k) act[k] = tanh_(tab, logits[k]);
        float r = 0.0f;
        done = true;
        if (!freeze) r = w2d_step(s.st, act, done);      // a finished env is frozen
        return r;
    }
};

// MLP at LPE lanes per env, single-wave workgroups (k_hop_mlp's shape): LPE <= 8: 32 / LPE hidden units per lane; above:
// the forward on every 16-lane row of the env's lanes.  envs_per_wave <= 64 / LPE different envs in the wave; the lane groups past
// the last one shadow it (same env, same path).  The lane's weight slice is re-read from the (L2-resident) row every step, so
// nothing of the policy has to stay in registers across the world steps.
template <int LPE>
__global__ __launch_bounds__(64, WALKER2D_MLP_WAVES_PER_SIMD) void k_w2d_mlp(const float *__restrict__ theta, const float *__restrict__ init,
                                                                           int init_per_offspring, int n_rows, int E, int P, int max_step,
                                                                           uint32_t obs_mask, int envs_per_wave,
                                                                           double *__restrict__ ep_return, int32_t *__restrict__ ep_steps)
{
    constexpr int S = 22, A = 6;
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    stage_tanh_table(tanh_tab);
    const int n_env = n_rows * E;
    const int group = (int)threadIdx.x / LPE;
    const int slot = group < envs_per_wave ? group : envs_per_wave - 1;
    int env = (int)blockIdx.x * envs_per_wave + slot;
    const int sub = (int)(threadIdx.x % LPE);
    const bool valid = env < n_env && group < envs_per_wave;
    env = env < n_env ? env : n_env - 1;
    const int row = env / E, ep = env - row * E;
    Walker2dState st;
    w2d_reset(st, init + ((size_t)(init_per_offspring ? row : 0) * E + ep) * 6);
    double ret = 0.0;
    int steps = 0;
    bool done = false;
    for (int t = 0; t < max_step; ++t) {
        if (__ballot(!done) == 0ull) break;
        float obs[S], logits[A];
        w2d_obs(st, obs);
#pragma unroll
        for (int k = 0; k < S; ++k) obs[k] = ((obs_mask >> k) & 1u) ? 0.0f : obs[k];
        if constexpr (LPE > 8) {
            MlpSlice<S, A, 16> net;
            net.load(theta + (size_t)row * P, (int)(threadIdx.x & 15));
            net.forward(tanh_tab, obs, logits);
        } else if constexpr (LPE >= 4) {
            MlpSlice<S, A, LPE> net;
            net.load(theta + (size_t)row * P, sub);
            net.forward(tanh_tab, obs, logits);
        } else {
            mlp_forward_streamed<S, A, LPE>(theta + (size_t)row * P, sub, tanh_tab, obs, logits);
        }
        float act[A];
#pragma unroll
        for (int k = 0; k < A; ++k) act[k] = tanh_(tanh_tab, logits[k]);
        if (!done) {                                               // a finished env is frozen
            ret += (double)w2d_step(st, act, done);
            steps += 1;
        }
    }
    if (valid && sub == 0) {
        ep_return[env] = ret;
        if (ep_steps) ep_steps[env] = steps;
    }
}

// GRU lockstep, one offspring per single-wave workgroup (k_rollout_gru_lockstep<.., false, 1>'s shape): a wave lives as long as
// the longest of its episodes and frees its SIMD slot for the next offspring when they are over
__global__ __launch_bounds__(64, WALKER2D_MLP_WAVES_PER_SIMD) void k_w2d_gru_ls(const float *__restrict__ theta, const float *__restrict__ init,
                                                                              int init_per_offspring, int n_rows, int E, int P, int max_step,
                                                                              uint32_t obs_mask, double *__restrict__ ep_return,
                                                                              int32_t *__restrict__ ep_steps)
{
    using EnvT = Walker2dLs;
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ __attribute__((aligned(16))) GruLockstepLds<EnvT::S, EnvT::A> lds;
    stage_tanh_table(tanh_tab);
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x < (unsigned)n_rows ? (int)blockIdx.x : n_rows - 1;
    const bool valid = blockIdx.x < (unsigned)n_rows;
    GruLockstep<EnvT::S, EnvT::A> net;
    net.load(theta + (size_t)row * P, lane, lds);
    wave_lds_sync();
    for (int e0 = 0; e0 < E; e0 += GL_EB) {
        const int nb = E - e0 < GL_EB ? E - e0 : GL_EB;
        const float *rows = init + ((size_t)(init_per_offspring ? row : 0) * E + e0) * EnvT::INIT_W;
        double *ro = ep_return ? ep_return + (size_t)row * E + e0 : nullptr;
        int32_t *so = ep_steps ? ep_steps + (size_t)row * E + e0 : nullptr;
#define SES_W2D_CASE(NP_, ODD_)                                                                                       \
    gru_lockstep_batch<EnvT, false, NP_, ODD_>(tanh_tab, lds, net, lane, nb, rows, max_step, obs_mask, ro, so, valid)
        switch (nb) {
            case 1: SES_W2D_CASE(1, true); break;
            case 2: SES_W2D_CASE(1, false); break;
            case 3: SES_W2D_CASE(2, true); break;
            case 4: SES_W2D_CASE(2, false); break;
            case 5: SES_W2D_CASE(3, true); break;
            case 6: SES_W2D_CASE(3, false); break;
            case 7: SES_W2D_CASE(4, true); break;
            default: SES_W2D_CASE(4, false); break;
        }
#undef SES_W2D_CASE
    }
}

// ---- the step-wise env: one lane per env -------------------------------------------------------------------------------------
__global__ __launch_bounds__(64, WALKER2D_MLP_WAVES_PER_SIMD) void k_w2d_env_reset(const float *__restrict__ init, int n,
                                                                                 Walker2dState *__restrict__ state, float *__restrict__ obs)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    Walker2dState s;
    w2d_reset(s, init + (size_t)i * 6);
    state[i].env = s.env;
    float o[22];
    w2d_obs(s, o);
    for (int k = 0; k < 22; ++k) obs[(size_t)i * 22 + k] = o[k];
}

__global__ __launch_bounds__(64, WALKER2D_MLP_WAVES_PER_SIMD) void k_w2d_env_step(Walker2dState *__restrict__ state, const float *__restrict__ action,
                                                                                int n, float *__restrict__ obs, float *__restrict__ reward,
                                                                                int32_t *__restrict__ done)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    Walker2dState s;
    s.env = state[i].env;
    float a[6];
    for (int k = 0; k < 6; ++k) a[k] = action[(size_t)i * 6 + k];
    bool d;
    const float r = w2d_step(s, a, d);
    state[i].env = s.env;
    float o[22];
    w2d_obs(s, o);
    for (int k = 0; k < 22; ++k) obs[(size_t)i * 22 + k] = o[k];
    reward[i] = r;
    done[i] = d ? 1 : 0;
}

// ---- host: the table row's entry functions (ses_env_table.h) -----------------------------------------------------------------
int walker2d_env_state_bytes(const ses_config *) { return (int)sizeof(Walker2dState); }

int walker2d_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs)
{
    hipLaunchKernelGGL(k_w2d_env_reset, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, init, n, (Walker2dState *)state, obs);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int walker2d_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done)
{
    hipLaunchKernelGGL(k_w2d_env_step, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, (Walker2dState *)state, (const float *)action, n, obs,
                       reward, done);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int walker2d_rollout(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode)
{
    SES_REQUIRE(mode == SES_MODE_EPISODIC, "ses_rollout: Walker2DBulletEnv-v0 has no fixed-length mode");
    if (h->cfg.gru) {
        launch_rollout_kernel(h, k_w2d_gru_ls, dim3(a.n_rows), dim3(64), a);
        return SES_OK;
    }
    const int lpe = plan.box2d_lpe, epw = plan.box2d_epw;
    SES_REQUIRE(epw >= 1 && lpe >= 1 && epw * lpe <= 64, "ses_rollout: Walker2DBulletEnv-v0 wave shape %d envs x %d lanes", epw, lpe);
    const dim3 grid(ceil_div(a.episodes(), epw));
    const auto launch = [&](auto lanes) { launch_rollout_kernel(h, k_w2d_mlp<lanes()>, grid, dim3(64), a, epw); };
    if (!with_lanes<64, 32, 16, 8, 4, 2, 1>(lpe, launch)) with_lanes<1>(1, launch);      // any other value: one lane per env
    return SES_OK;
}

// ses_policy_forward for (num_state, num_action) = (22, 6), MLP or GRU; the caller has checked the shape
int walker2d_policy_forward(ses_handle *h, const float *theta, const float *obs, float *hidden, int n, float *logits, float *act,
                          int32_t *action)
{
    if (h->cfg.gru)
        hipLaunchKernelGGL((k_policy_forward_gru<22, 6>), dim3(ceil_div(n, 4)), dim3(256), 0, h->stream, theta, obs, hidden, n, h->P, logits,
                           act, action);
    else
        hipLaunchKernelGGL((k_policy_forward_mlp<22, 6>), dim3(ceil_div((long long)n * 4, 64)), dim3(64), 0, h->stream, theta, obs, n, h->P,
                           logits, act, action);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

}  // namespace ses
