// ses_classic_cont.hip -- gym's continuous-action classic-control envs Pendulum-v1 and MountainCarContinuous-v0
// (csrc/ses_classic_cont.h: float64, Python's order of operations) on the device, through every path the other envs have:
//   k_envs_reset_classic_cont / k_envs_step_classic_cont : env.reset() / env.step(a) for n independent envs (ses_env_reset /
//                                                ses_env_step_generic), one lane per env, the blob is the float64 state,
//                                                the action float32[n, 1], the reward the float64 reward rounded to float
//   k_rollout_classic_cont_mlp                 : RolloutWorker (loop.py:108-125) with an MLP policy and the tanh head, any env
//   k_rollout_pendulum_mlp                     : the same for Pendulum alone: one sincos per step, no alive / freeze logic
//   k_rollout_gru_lockstep<PendulumLs / ...>   : the same with a GRU policy, the lockstep kernel of ses_gru_lockstep.h
//   k_policy_forward_mlp / _gru<3 or 2, 1>     : ses_policy_forward for these shapes (GymEnvModel.forward, playback)
// Episodic mode only.  A unit of its own: the kernels of the other units keep their machine code byte for byte.
#include "ses_classic_cont.h"
#include "ses_gru_lockstep.h"
#include "ses_internal.h"
#include "ses_policy.h"
#include "ses_policy_forward.h"

namespace ses {

// ---- step-wise envs -----------------------------------------------------------------------------------------------------
template <class EnvC>
__global__ __launch_bounds__(64) void k_envs_reset_classic_cont(const float *__restrict__ init, int n,
                                                                typename EnvC::State *__restrict__ state, float *__restrict__ obs)
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
__global__ __launch_bounds__(64) void k_envs_step_classic_cont(typename EnvC::State *__restrict__ state, const float *__restrict__ action,
                                                               int n, float *__restrict__ obs, float *__restrict__ reward,
                                                               int32_t *__restrict__ done)
{
    constexpr int A = EnvC::A;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    typename EnvC::State st = state[i];
    float act[A];
#pragma unroll
    for (int k = 0; k < A; ++k) act[k] = action[(size_t)i * A + k];     // (any float: the env clips it, never rejects it)
    bool d;
    const double r = EnvC::step(st, act, d);
    state[i] = st;
    float o[EnvC::S];
    EnvC::observe(st, o);
#pragma unroll
    for (int k = 0; k < EnvC::S; ++k) obs[(size_t)i * EnvC::S + k] = o[k];
    reward[i] = (float)r;
    done[i] = d ? 1 : 0;
}

// ---- fused MLP rollouts ---------------------------------------------------------------------------------------------------
// k_rollout_classic_mlp (ses_classic.hip) with the tanh head in place of the argmax and the adapter's float64 reward added
// as it is: LPE adjacent lanes share one env, every lane of the group runs the env's physics (identical bits), the MLP is
// split over the group (slice in registers for 4 ... 32 lanes per env, streamed from the row for 1 and 2).
template <class EnvC, int LPE>
__global__ __launch_bounds__(64) void k_rollout_classic_cont_mlp(const float *__restrict__ theta, const float *__restrict__ init,
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
        float obs[S], logits[A], act[A];
        EnvC::observe(st, obs);
        if constexpr (LPE >= 4) net.forward(tanh_tab, obs, logits);
        else mlp_forward_streamed<S, A, LPE>(th, sub, tanh_tab, obs, logits);
#pragma unroll
        for (int k = 0; k < A; ++k) act[k] = tanh_(tanh_tab, logits[k]);
        if (!done) {
            ret += EnvC::step(st, act, done);
            steps += 1;
        }
    }
    if (valid && sub == 0) {
        ep_return[env] = ret;
        if (ep_steps) ep_steps[env] = steps;
    }
}

// Pendulum never terminates: every episode is max_step steps and the whole population runs in lockstep, so the loop carries
// no alive flag, no ballot and no frozen state.  One step needs sin th for the dynamics and (cos th, sin th) for the
// observation of the SAME angle: sincos_ieee runs once per step and serves both (the bits are the same, which is what makes
// it legal).  The step is one float64 dependence chain -- sincos (~25 f64 ops deep), the policy, the torque, th' -- and the
// cost term (the exact mod, three squares) hangs off its side: latency, not issue, is what a small population pays.
template <int LPE>
__global__ __launch_bounds__(64) void k_rollout_pendulum_mlp(const float *__restrict__ theta, const float *__restrict__ init,
                                                             int init_per_offspring, int n_rows, int E, int P, int max_step,
                                                             double *__restrict__ ep_return, int32_t *__restrict__ ep_steps)
{
    constexpr int S = PendulumEnv::S, A = PendulumEnv::A;
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    stage_tanh_table(tanh_tab);
    const long long n_env = (long long)n_rows * E;
    long long env = ((long long)blockIdx.x * 64 + threadIdx.x) / LPE;
    const int sub = (int)(threadIdx.x % LPE);
    const bool valid = env < n_env;
    env = valid ? env : n_env - 1;                                  // lane groups past the last env shadow it
    const int row = (int)(env / E), ep = (int)(env - (long long)row * E);
    const float *th = theta + (size_t)row * P;
    PendulumState st = pendulum_reset(init + ((size_t)(init_per_offspring ? row : 0) * E + ep) * PD_INIT_W);
    MlpSlice<S, A, (LPE >= 4 ? LPE : 4)> net;
    if constexpr (LPE >= 4) net.load(th, sub);
    double ret = 0.0;
    for (int t = 0; t < max_step; ++t) {
        double sn, cs;
        sincos_ieee(st.th, sn, cs);
        float obs[S], logits[A];
        pendulum_obs_from(sn, cs, st, obs);
        if constexpr (LPE >= 4) net.forward(tanh_tab, obs, logits);
        else mlp_forward_streamed<S, A, LPE>(th, sub, tanh_tab, obs, logits);
        ret += pendulum_step_sin(st, sn, (double)tanh_(tanh_tab, logits[0]));
    }
    if (valid && sub == 0) {
        ep_return[env] = ret;
        if (ep_steps) ep_steps[env] = max_step;
    }
}

// ---- GRU adapters of the lockstep kernel (the CartPoleLs interface, ses_rollout.hip; the reward is the adapter's double) ----
template <class EnvC>
struct ClassicContLs {
    static constexpr int S = EnvC::S, A = EnvC::A, INIT_W = EnvC::INIT_W;
    struct State {
        typename EnvC::State st;
    };
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u, int) { EnvC::reset(s.st, u); }
    __device__ static __forceinline__ void observe(const State &s, float (&obs)[S]) { EnvC::observe(s.st, obs); }
    __device__ static __forceinline__ double step(State &s, const float (&logits)[A], const TanhEntry *tab, bool freeze, bool &done)
    {
        float act[A];
#pragma unroll
        for (int k = 0; k < A; ++k) act[k] = tanh_(tab, logits[k]);
        typename EnvC::State ns = s.st;
        const double r = EnvC::step(ns, act, done);
        if (!freeze) s.st = ns;                                     // a finished env is frozen
        return r;
    }
};
using PendulumLs = ClassicContLs<PendulumEnv>;
using MountainCarContLs = ClassicContLs<MountainCarContEnv>;

// ---- host side -----------------------------------------------------------------------------------------------------------
static bool is_pendulum(const ses_handle *h) { return h->cfg.env_id == SES_ENV_PENDULUM; }
static const char *cont_name(const ses_handle *h) { return is_pendulum(h) ? "Pendulum" : "MountainCarContinuous"; }

int classic_cont_env_state_bytes(const ses_handle *h)
{
    return is_pendulum(h) ? (int)sizeof(PendulumState) : (int)sizeof(MountainCarState);
}

int classic_cont_env_obs_width(const ses_handle *h) { return is_pendulum(h) ? PendulumEnv::S : MountainCarContEnv::S; }

int classic_cont_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs)
{
    const dim3 grid(ceil_div(n, 64)), block(64);
    if (is_pendulum(h))
        hipLaunchKernelGGL(k_envs_reset_classic_cont<PendulumEnv>, grid, block, 0, h->stream, init, n, (PendulumState *)state, obs);
    else
        hipLaunchKernelGGL(k_envs_reset_classic_cont<MountainCarContEnv>, grid, block, 0, h->stream, init, n, (MountainCarState *)state,
                           obs);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int classic_cont_env_step(ses_handle *h, void *state, const float *action, int n, float *obs, float *reward, int32_t *done)
{
    const dim3 grid(ceil_div(n, 64)), block(64);
    if (is_pendulum(h))
        hipLaunchKernelGGL(k_envs_step_classic_cont<PendulumEnv>, grid, block, 0, h->stream, (PendulumState *)state, action, n, obs,
                           reward, done);
    else
        hipLaunchKernelGGL(k_envs_step_classic_cont<MountainCarContEnv>, grid, block, 0, h->stream, (MountainCarState *)state, action, n,
                           obs, reward, done);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

// Lanes per env of the MLP rollout (cfg.lanes_per_env overrides), the best measured setting at both population sizes
// (profiles/classic_control_cont_timing.txt, tools/time_classic_cont.py; 5 episodes to the TimeLimit, random first-generation
// policies).  Pendulum: the largest split up to 8 that keeps the population within 2048 waves -- 240 offspring 0.104 ms at 8
// (0.122 / 0.111 / 0.107 at 4 / 16 / 32), 4096 offspring 0.178 ms at 4 (0.201 / 0.206 at 2 / 8).  MountainCarContinuous: 32
// lanes while the population fits 256 waves (one per CU: the copies of the physics cost nobody an issue slot, the policy's
// part of the chain is shortest) -- 97 offspring 0.382 ms (0.393 / 0.439 at 16 / 8) -- else MountainCar's rule, the largest
// split up to 16 within 2048 waves: 4096 offspring 0.757 ms at 4 (0.83 / 1.54 at 8 / 2).
int classic_cont_lanes_per_env(const ses_handle *h, long long episodes)
{
    if (h->cfg.lanes_per_env) return h->cfg.lanes_per_env;
    const long long budget = 2048;
    if (!is_pendulum(h) && (episodes * 32 + 63) / 64 <= 256) return 32;
    int lpe = is_pendulum(h) ? 8 : 16;
    while (lpe > 1 && (episodes * lpe + 63) / 64 > budget) lpe >>= 1;
    return lpe;
}

// (first-use order of the kernel instances, see ses_internal.h: the GRU kernels Pendulum, MountainCarContinuous; then the MLP
// kernels: Pendulum's own 1 ... 32 lanes per env, the generic one for Pendulum 1 ... 32, for MountainCarContinuous 1 ... 32)
static int launch_pendulum_mlp(const ses_handle *h, const RolloutArgs &a)
{
    const int lpe = classic_cont_lanes_per_env(h, a.episodes());
    const dim3 grid(ceil_div(a.episodes() * lpe, 64)), block(64);
    const bool known = with_lanes<1, 2, 4, 8, 16, 32>(lpe, [&](auto lanes) {
        hipLaunchKernelGGL((k_rollout_pendulum_mlp<lanes()>), grid, block, 0, h->stream, a.theta, a.init, a.per, a.n_rows, a.E, a.P,
                           a.max_step, a.epr, a.ep_steps);
    });
    if (!known) return set_error(SES_ERR_INVALID_ARG, "ses_rollout: Pendulum has no MLP rollout at %d lanes per env (1, 2, 4, 8, 16, 32)", lpe);
    return SES_OK;
}

template <class EnvC>
static int launch_classic_cont_mlp(const ses_handle *h, const RolloutArgs &a)
{
    const int lpe = classic_cont_lanes_per_env(h, a.episodes());
    const dim3 grid(ceil_div(a.episodes() * lpe, 64)), block(64);
    const bool known = with_lanes<1, 2, 4, 8, 16, 32>(lpe, [&](auto lanes) {
        hipLaunchKernelGGL((k_rollout_classic_cont_mlp<EnvC, lanes()>), grid, block, 0, h->stream, a.theta, a.init, a.per, a.n_rows,
                           a.E, a.P, a.max_step, a.epr, a.ep_steps);
    });
    if (!known)
        return set_error(SES_ERR_INVALID_ARG, "ses_rollout: %s has no MLP rollout at %d lanes per env (1, 2, 4, 8, 16, 32)", cont_name(h), lpe);
    return SES_OK;
}

int classic_cont_rollout(const ses_handle *h, const RolloutArgs &a, int mode)
{
    SES_REQUIRE(mode == SES_MODE_EPISODIC, "ses_rollout: %s has no fixed-length mode", cont_name(h));
    if (h->cfg.gru) {
        const dim3 grid(ceil_div(a.n_rows, 4)), block(256);
        if (is_pendulum(h)) launch_rollout_kernel(h, k_rollout_gru_lockstep<PendulumLs, false, 4>, grid, block, a);
        else launch_rollout_kernel(h, k_rollout_gru_lockstep<MountainCarContLs, false, 4>, grid, block, a);
    } else {
        int rc;
        if (!is_pendulum(h)) rc = launch_classic_cont_mlp<MountainCarContEnv>(h, a);
        else if (h->tune_pendulum_generic) rc = launch_classic_cont_mlp<PendulumEnv>(h, a);     // the observe / step split, for A/B runs
        else rc = launch_pendulum_mlp(h, a);
        if (rc != SES_OK) return rc;
    }
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int classic_cont_policy_forward(ses_handle *h, const float *theta, const float *obs, float *hidden, int n, float *logits, float *act,
                                int32_t *action)
{
    const int S = h->cfg.num_state == 3 ? 3 : 2;                // (first-use order: the GRU instances, then the MLP ones)
    if (h->cfg.gru)
        with_policy_shape<PolicyShape<3, 1>, PolicyShape<2, 1>>(S, 1, [&](auto sh) {
            hipLaunchKernelGGL((k_policy_forward_gru<sh.S, sh.A>), dim3(ceil_div(n, 4)), dim3(256), 0, h->stream, theta, obs, hidden, n,
                               h->P, logits, act, action);
        });
    else
        with_policy_shape<PolicyShape<3, 1>, PolicyShape<2, 1>>(S, 1, [&](auto sh) {
            hipLaunchKernelGGL((k_policy_forward_mlp<sh.S, sh.A>), dim3(ceil_div((long long)n * 4, 64)), dim3(64), 0, h->stream, theta,
                               obs, n, h->P, logits, act, action);
        });
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

}  // namespace ses
