// ses_classic.hip -- gym's classic-control envs Acrobot-v1, MountainCar-v0, Pendulum-v1 and MountainCarContinuous-v0
// (csrc/ses_classic.h: float64, gym's order of operations) on the device, through every path the other envs have:
//   k_envs_reset_classic / k_envs_step_classic : env.reset() / env.step(a) for n independent envs (ses_env_reset /
//                                                ses_env_step_generic), one lane per env, the blob is the float64 state;
//                                                the action int32[n] or float32[n, A], the reward rounded to float
//   k_rollout_classic_mlp                      : RolloutWorker (loop.py:108-125) with an MLP policy, one kernel per shard
//   k_rollout_pendulum_mlp                     : the same for Pendulum alone: one sincos per step, no alive / freeze logic
//   k_rollout_gru_lockstep<ClassicLs<...>>     : the same with a GRU policy, the lockstep kernel of ses_gru_lockstep.h
//   k_policy_forward_mlp / _gru                : ses_policy_forward for these envs' shapes (GymEnvModel.forward, playback)
// Every kernel is one template over the env adapters of ses_classic.h; EnvC::Action (int, or float[A]) picks the policy head
// and the step-wise action layout at compile time.  Episodic mode only.  A unit of its own: the kernels of the other units
// keep their machine code byte for byte.
#include "ses_classic.h"
#include "ses_gru_lockstep.h"
#include "ses_internal.h"
#include "ses_policy.h"
#include "ses_policy_forward.h"

namespace ses {

template <class EnvC>
constexpr bool is_discrete = std::is_same_v<typename EnvC::Action, int>;

// the policy head: the first argmax of the A outputs (discrete), or tanh_ of each (continuous)
template <class EnvC>
__device__ __forceinline__ void classic_head(const TanhEntry *tab, const float (&logits)[EnvC::A], typename EnvC::Action &action)
{
    if constexpr (is_discrete<EnvC>) {
        action = argmax_first<EnvC::A>(logits);
    } else {
#pragma unroll
        for (int k = 0; k < EnvC::A; ++k) action[k] = tanh_(tab, logits[k]);
    }
}

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
__global__ __launch_bounds__(64) void k_envs_step_classic(typename EnvC::State *__restrict__ state,
                                                          const std::remove_extent_t<typename EnvC::Action> *__restrict__ action, int n,
                                                          float *__restrict__ obs, float *__restrict__ reward, int32_t *__restrict__ done)
{
    constexpr int A = EnvC::A;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    typename EnvC::State st = state[i];
    typename EnvC::Action act;
    if constexpr (is_discrete<EnvC>) {
        const int a = action[i];
        act = a < 0 ? 0 : (a > 2 ? 2 : a);                                  // (gym's action spaces are {0, 1, 2}: clamped into it)
    } else {
#pragma unroll
        for (int k = 0; k < A; ++k) act[k] = action[(size_t)i * A + k];     // (any float: the env clips it, never rejects it)
    }
    bool d;
    const auto r = EnvC::step(st, act, d);
    state[i] = st;
    float o[EnvC::S];
    EnvC::observe(st, o);
#pragma unroll
    for (int k = 0; k < EnvC::S; ++k) obs[(size_t)i * EnvC::S + k] = o[k];
    reward[i] = (float)r;
    done[i] = d ? 1 : 0;
}

// ---- fused MLP rollouts ---------------------------------------------------------------------------------------------------
// LPE adjacent lanes share one env (env = row * E + episode) as in k_rollout_box2d_mlp without the terrain: every lane of
// the group runs the env's physics (identical bits), the MLP is split over the group -- MlpSlice with the offspring's slice
// in registers for 4 ... 32 lanes per env, streamed from the (L2-resident) row for 1 and 2.  A finished env is frozen, the
// wave leaves as soon as none of its envs is alive.  One env step is a chain of ~15 sin / cos and 16 f64 divisions behind
// four sequential RK4 stages (Acrobot): at the populations ES uses the chip holds far fewer envs than lanes, so the step's
// dependence chain, not issue, is what a rollout costs -- the lanes per env only decide how many waves (and SIMDs) share
// the population and how short the policy's part of the chain is (classic_lanes_per_env).  The return adds the adapter's
// reward in float64: exact for the discrete envs' float rewards, the env's own float64 for the continuous ones.
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
        typename EnvC::Action action;
        classic_head<EnvC>(tanh_tab, logits, action);
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

// ---- GRU adapter of the lockstep kernel (the CartPoleLs interface, ses_rollout.hip; the reward is the adapter's own type) ----
template <class EnvC>
struct ClassicLs {
    static constexpr int S = EnvC::S, A = EnvC::A, INIT_W = EnvC::INIT_W;
    struct State {
        typename EnvC::State st;
    };
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u, int) { EnvC::reset(s.st, u); }
    __device__ static __forceinline__ void observe(const State &s, float (&obs)[S]) { EnvC::observe(s.st, obs); }
    __device__ static __forceinline__ auto step(State &s, const float (&logits)[A], const TanhEntry *tab, bool freeze, bool &done)
    {
        typename EnvC::Action action;
        classic_head<EnvC>(tab, logits, action);
        typename EnvC::State ns = s.st;
        const auto r = EnvC::step(ns, action, done);
        if (!freeze) s.st = ns;                                     // a finished env is frozen
        return r;
    }
};

// ---- host side -----------------------------------------------------------------------------------------------------------
// env_id -> adapter: returns f(EnvC{}) for the adapter of a classic-control env_id (is_classic_env; visited in the order
// listed).  f is a generic lambda that names the kernel instances with decltype of its argument.
template <class F>
static int with_classic_env(int env_id, F &&f)
{
    switch (env_id) {
        case SES_ENV_ACROBOT: return f(AcrobotEnv{});
        case SES_ENV_MOUNTAINCAR: return f(MountainCarEnv{});
        case SES_ENV_PENDULUM: return f(PendulumEnv{});
        default: return f(MountainCarContEnv{});
    }
}

// (first-use order of the kernel instances, see ses_internal.h: the reset kernels Acrobot, MountainCar, Pendulum,
// MountainCarContinuous; the step kernels likewise; then per env in that order its GRU kernel and its MLP kernels 1 ... 32
// lanes per env -- for Pendulum the generic kernel and its own alternate, lane count by lane count; last the
// policy-forward instances, GRU (6,3) (2,3) (3,1) (2,1), then MLP likewise)
int classic_env_state_bytes(const ses_handle *h)
{
    return with_classic_env(h->cfg.env_id, [](auto env) { return (int)sizeof(typename decltype(env)::State); });
}

int classic_env_obs_width(const ses_handle *h)
{
    return with_classic_env(h->cfg.env_id, [](auto env) { return decltype(env)::S; });
}

int classic_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs)
{
    return with_classic_env(h->cfg.env_id, [&](auto env) -> int {
        using EnvC = decltype(env);
        hipLaunchKernelGGL(k_envs_reset_classic<EnvC>, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, init, n,
                           (typename EnvC::State *)state, obs);
        SES_HIP_TRY(hipGetLastError());
        return SES_OK;
    });
}

// action: int32[n] for the discrete envs, float32[n, A] for the continuous ones
int classic_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done)
{
    return with_classic_env(h->cfg.env_id, [&](auto env) -> int {
        using EnvC = decltype(env);
        hipLaunchKernelGGL(k_envs_step_classic<EnvC>, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, (typename EnvC::State *)state,
                           (const std::remove_extent_t<typename EnvC::Action> *)action, n, obs, reward, done);
        SES_HIP_TRY(hipGetLastError());
        return SES_OK;
    });
}

// Lanes per env of the MLP rollout (cfg.lanes_per_env overrides): the largest split up to a cap that keeps the population
// within a wave budget -- up to 16 within 1024 waves for Acrobot, up to 16 within 2048 for MountainCar, up to 8 within 2048
// for Pendulum; MountainCarContinuous 32 while the population fits 256 waves, else MountainCar's rule.  Every lane of an
// env's group repeats the env's physics, so more lanes per env buy a shorter policy step and fewer envs per wave (an earlier
// exit) only while the chip has issue slots to spare for the copies.
// Measured, discrete envs (profiles/classic_control_timing.txt, tools/time_classic.py; 5 episodes, random first-generation
// policies): Acrobot 97 offspring 1.32 ms at 16 or 32 lanes per env against 1.53 at 8; 4096 offspring 2.30 ms at 2 against
// 2.44 / 2.55 / 3.54 at 1 / 4 / 8 -- its 16 f64 divisions and ~15 sin / cos per step make the copies cost issue there;
// MountainCar 240 offspring 0.083 ms at 16 (0.089 / 0.091 at 8 / 32); 4096 offspring 0.151 ms at 4 (0.170 / 0.273 at 8 / 2).
// Measured, continuous envs, the best setting at both population sizes (profiles/classic_control_cont_timing.txt, the same
// tool; 5 episodes to the TimeLimit, random first-generation policies): Pendulum 240 offspring 0.104 ms at 8 (0.122 / 0.111 /
// 0.107 at 4 / 16 / 32), 4096 offspring 0.178 ms at 4 (0.201 / 0.206 at 2 / 8).  MountainCarContinuous at 32 lanes has one
// wave per CU (the copies of the physics cost nobody an issue slot, the policy's part of the chain is shortest) -- 97
// offspring 0.382 ms (0.393 / 0.439 at 16 / 8); 4096 offspring 0.757 ms at 4 (0.83 / 1.54 at 8 / 2).
int classic_lanes_per_env(const ses_handle *h, long long episodes)
{
    if (h->cfg.lanes_per_env) return h->cfg.lanes_per_env;
    const int env_id = h->cfg.env_id;
    if (env_id == SES_ENV_MOUNTAINCAR_CONT && (episodes * 32 + 63) / 64 <= 256) return 32;
    const long long budget = env_id == SES_ENV_ACROBOT ? 1024 : 2048;
    int lpe = env_id == SES_ENV_PENDULUM ? 8 : 16;
    while (lpe > 1 && (episodes * lpe + 63) / 64 > budget) lpe >>= 1;
    return lpe;
}

int classic_rollout(const ses_handle *h, const RolloutArgs &a, int mode)
{
    return with_classic_env(h->cfg.env_id, [&](auto env) -> int {
        using EnvC = decltype(env);
        SES_REQUIRE(mode == SES_MODE_EPISODIC, "ses_rollout: %s has no fixed-length mode", EnvC::NAME);
        if (h->cfg.gru) {
            launch_rollout_kernel(h, k_rollout_gru_lockstep<ClassicLs<EnvC>, false, 4>, dim3(ceil_div(a.n_rows, 4)), dim3(256), a);
        } else {
            const int lpe = classic_lanes_per_env(h, a.episodes());
            const bool known = with_lanes<1, 2, 4, 8, 16, 32>(lpe, [&](auto lanes) {
                auto kernel = k_rollout_classic_mlp<EnvC, lanes()>;
                if constexpr (std::is_same_v<EnvC, PendulumEnv>) {
                    if (!h->tune_pendulum_generic) kernel = k_rollout_pendulum_mlp<lanes()>;   // (1: the observe / step split, for A/B runs)
                }
                hipLaunchKernelGGL(kernel, dim3(ceil_div(a.episodes() * lpe, 64)), dim3(64), 0, h->stream, a.theta, a.init, a.per,
                                   a.n_rows, a.E, a.P, a.max_step, a.epr, a.ep_steps);
            });
            if (!known)
                return set_error(SES_ERR_INVALID_ARG, "ses_rollout: %s has no MLP rollout at %d lanes per env (1, 2, 4, 8, 16, 32)",
                                 EnvC::NAME, lpe);
        }
        SES_HIP_TRY(hipGetLastError());
        return SES_OK;
    });
}

// ses_policy_forward for the shapes of the four envs; the caller has checked that (num_state, num_action) is one of them
int classic_policy_forward(ses_handle *h, const float *theta, const float *obs, float *hidden, int n, float *logits, float *act,
                           int32_t *action)
{
    const int S = h->cfg.num_state, A = h->cfg.num_action;
    if (h->cfg.gru)
        with_policy_shape<PolicyShape<6, 3>, PolicyShape<2, 3>, PolicyShape<3, 1>, PolicyShape<2, 1>>(S, A, [&](auto sh) {
            hipLaunchKernelGGL((k_policy_forward_gru<sh.S, sh.A>), dim3(ceil_div(n, 4)), dim3(256), 0, h->stream, theta, obs, hidden, n,
                               h->P, logits, act, action);
        });
    else
        with_policy_shape<PolicyShape<6, 3>, PolicyShape<2, 3>, PolicyShape<3, 1>, PolicyShape<2, 1>>(S, A, [&](auto sh) {
            hipLaunchKernelGGL((k_policy_forward_mlp<sh.S, sh.A>), dim3(ceil_div((long long)n * 4, 64)), dim3(64), 0, h->stream, theta,
                               obs, n, h->P, logits, act, action);
        });
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

}  // namespace ses
