// ses_pendula.hip -- the inverted-pendulum family modelled on pybullet_envs (csrc/ses_pendula.h: float64, the build's own
// definitions) on the device, through every path the classic-control envs have:
//   k_envs_reset_pendula / k_envs_step_pendula : env.reset() / env.step(a) for n independent envs (ses_env_reset /
//                                                ses_env_step_generic), one lane per env, the blob is the float64 state;
//                                                the action float32[n, 1], the reward rounded to float
//   k_rollout_pendula_mlp                      : RolloutWorker (loop.py:108-125) with an MLP policy, one kernel per shard: one
//                                                trig per step (ONE_TRIG), or the generic observe / step form (its A/B partner)
//   k_rollout_gru_lockstep<PendulaLs<...>>     : the same with a GRU policy, the lockstep kernel of ses_gru_lockstep.h
//   k_policy_forward_mlp / _gru                : ses_policy_forward at (5, 1) and (9, 1) (GymEnvModel.forward, playback)
// Every kernel is one template over the three env adapters.  Episodic mode only.  A unit of its own: the kernels of the other
// units keep their machine code byte for byte.
#include "ses_pendula.h"
#include "ses_gru_lockstep.h"
#include "ses_internal.h"
#include "ses_policy.h"
#include "ses_policy_forward.h"

namespace ses {

// ---- step-wise envs -----------------------------------------------------------------------------------------------------
template <class EnvP>
__global__ __launch_bounds__(64) void k_envs_reset_pendula(const float *__restrict__ init, int n, typename EnvP::State *__restrict__ state,
                                                           float *__restrict__ obs)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    typename EnvP::State st;
    EnvP::reset(st, init + (size_t)i * EnvP::INIT_W);
    state[i] = st;
    float o[EnvP::S];
    EnvP::observe(st, o);
#pragma unroll
    for (int k = 0; k < EnvP::S; ++k) obs[(size_t)i * EnvP::S + k] = o[k];
}

template <class EnvP>
__global__ __launch_bounds__(64) void k_envs_step_pendula(typename EnvP::State *__restrict__ state, const float *__restrict__ action, int n,
                                                          float *__restrict__ obs, float *__restrict__ reward, int32_t *__restrict__ done)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    typename EnvP::State st = state[i];
    const float act[1] = {action[i]};                                       // (any float: the env clips it, never rejects it)
    bool d;
    const double r = EnvP::step(st, act, d);
    state[i] = st;
    float o[EnvP::S];
    EnvP::observe(st, o);
#pragma unroll
    for (int k = 0; k < EnvP::S; ++k) obs[(size_t)i * EnvP::S + k] = o[k];
    reward[i] = (float)r;
    done[i] = d ? 1 : 0;
}

// ---- fused MLP rollouts ---------------------------------------------------------------------------------------------------
// LPE adjacent lanes share one env (env = row * E + episode) as in k_rollout_classic_mlp: every lane of the group runs the
// env's physics (identical bits), the MLP is split over the group -- MlpSlice with the offspring's slice in registers for
// 4 ... 32 lanes per env, streamed from the (L2-resident) row for 1 and 2.
// ONE_TRIG: the trig of a state (one sincos_ieee per angle) is evaluated once, when the state is entered.  It gives the
// outcome of the step that entered it (swing-up's reward cos theta, the double pendulum's x2 / y2 reward and done) and, one
// iteration later, the observation and the accelerations of the step that leaves it -- the bits are the same, which is what
// makes it legal.  The generic form (ONE_TRIG false) is EnvP::observe then EnvP::step: one trig for the observation, one for
// the accelerations, one for the outcome.
// A terminating env (balance, double) is frozen once done and the wave leaves when none of its envs is alive; swing-up never
// terminates, so its loop carries no alive flag, no ballot and no frozen state.
template <class EnvP, int LPE, bool ONE_TRIG = true>
__global__ __launch_bounds__(64) void k_rollout_pendula_mlp(const float *__restrict__ theta, const float *__restrict__ init,
                                                            int init_per_offspring, int n_rows, int E, int P, int max_step,
                                                            double *__restrict__ ep_return, int32_t *__restrict__ ep_steps)
{
    constexpr int S = EnvP::S, A = EnvP::A;
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    stage_tanh_table(tanh_tab);
    const long long n_env = (long long)n_rows * E;
    long long env = ((long long)blockIdx.x * 64 + threadIdx.x) / LPE;
    const int sub = (int)(threadIdx.x % LPE);
    const bool valid = env < n_env;
    env = valid ? env : n_env - 1;                                  // lane groups past the last env shadow it
    const int row = (int)(env / E), ep = (int)(env - (long long)row * E);
    const float *th = theta + (size_t)row * P;
    typename EnvP::State st;
    EnvP::reset(st, init + ((size_t)(init_per_offspring ? row : 0) * E + ep) * EnvP::INIT_W);
    MlpSlice<S, A, (LPE >= 4 ? LPE : 4)> net;
    if constexpr (LPE >= 4) net.load(th, sub);
    typename EnvP::Trig tg;
    if constexpr (ONE_TRIG) EnvP::trig(st, tg);
    double ret = 0.0;
    int steps = 0;
    bool done = false;
    for (int t = 0; t < max_step; ++t) {
        if constexpr (EnvP::TERMINATES) {
            if (__ballot(!done) == 0ull) break;
        }
        float obs[S], logits[A];
        if constexpr (ONE_TRIG) EnvP::observe_from(st, tg, obs);
        else EnvP::observe(st, obs);
        if constexpr (LPE >= 4) net.forward(tanh_tab, obs, logits);
        else mlp_forward_streamed<S, A, LPE>(th, sub, tanh_tab, obs, logits);
        const float act[A] = {tanh_(tanh_tab, logits[0])};
        if (!EnvP::TERMINATES || !done) {
            if constexpr (ONE_TRIG) {
                EnvP::advance(st, tg, (double)act[0]);
                EnvP::trig(st, tg);
                ret += EnvP::outcome(st, tg, done);
            } else {
                ret += EnvP::step(st, act, done);
            }
            steps += 1;
        }
    }
    if (valid && sub == 0) {
        ep_return[env] = ret;
        if (ep_steps) ep_steps[env] = EnvP::TERMINATES ? steps : max_step;
    }
}

// ---- GRU adapter of the lockstep kernel (the ClassicLs shape of ses_classic.hip) ------------------------------------------------
template <class EnvP>
struct PendulaLs {
    static constexpr int S = EnvP::S, A = EnvP::A, INIT_W = EnvP::INIT_W;
    struct State {
        typename EnvP::State st;
    };
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u, int) { EnvP::reset(s.st, u); }
    __device__ static __forceinline__ void observe(const State &s, float (&obs)[S]) { EnvP::observe(s.st, obs); }
    __device__ static __forceinline__ double step(State &s, const float (&logits)[A], const TanhEntry *tab, bool freeze, bool &done)
    {
        const float act[A] = {tanh_(tab, logits[0])};
        typename EnvP::State ns = s.st;
        const double r = EnvP::step(ns, act, done);
        if (!freeze) s.st = ns;                                     // a finished env is frozen
        return r;
    }
};

// ---- host side -----------------------------------------------------------------------------------------------------------
// env_id -> adapter: returns f(EnvP{}) for the adapter of an env_id of the family (is_pendula_env; visited in the order listed)
template <class F>
static int with_pendula_env(int env_id, F &&f)
{
    switch (env_id) {
        case SES_ENV_INVERTED_PENDULUM: return f(InvertedPendulumEnv{});
        case SES_ENV_PENDULUM_SWINGUP: return f(PendulumSwingupEnv{});
        default: return f(DoublePendulumEnv{});
    }
}

int pendula_env_state_bytes(const ses_handle *h)
{
    return with_pendula_env(h->cfg.env_id, [](auto env) { return (int)sizeof(typename decltype(env)::State); });
}

int pendula_env_obs_width(const ses_handle *h)
{
    return with_pendula_env(h->cfg.env_id, [](auto env) { return decltype(env)::S; });
}

int pendula_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs)
{
    return with_pendula_env(h->cfg.env_id, [&](auto env) -> int {
        using EnvP = decltype(env);
        hipLaunchKernelGGL(k_envs_reset_pendula<EnvP>, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, init, n,
                           (typename EnvP::State *)state, obs);
        SES_HIP_TRY(hipGetLastError());
        return SES_OK;
    });
}

// action: float32[n, 1]
int pendula_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done)
{
    return with_pendula_env(h->cfg.env_id, [&](auto env) -> int {
        using EnvP = decltype(env);
        hipLaunchKernelGGL(k_envs_step_pendula<EnvP>, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, (typename EnvP::State *)state,
                           (const float *)action, n, obs, reward, done);
        SES_HIP_TRY(hipGetLastError());
        return SES_OK;
    });
}

// Lanes per env of the MLP rollout (cfg.lanes_per_env overrides): the largest split up to 32 that keeps the population within
// 2048 waves.  Every lane of an env's group repeats the env's physics, so more lanes per env buy a shorter policy step only
// while the chip has issue slots to spare for the copies.
// Measured (profiles/pendula_timing.txt, tools/time_pendula.py; 5 episodes, random first-generation policies, the default form,
// all candidates alternating in one process): swing-up, every episode 1000 steps, 240 offspring 0.457 ms at 32 (0.519 / 0.540 /
// 0.591 at 16 / 8 / 4), 4096 offspring 1.00 ms at 4 (1.02 / 1.20 / 1.73 / 3.18 at 2 / 8 / 16 / 32); the double pendulum, ~21
// steps per episode, 240 offspring 0.063 / 0.064 ms at 16 / 32 (0.070 at 8), 4096 offspring 0.142 ms at 4 (0.153 / 0.181 at 8 /
// 16).  Balance under random policies lasts ~15 steps per episode, so its waves leave early and its first generation would take
// 16 lanes at 4096 offspring (0.590 ms against 0.717 at 4; 240 offspring: 0.145 ms at 32, 0.148 at 16); a population that has
// learnt to balance runs every episode to the cap on the swing-up's transition code, and the rule is set for that: one rule for the
// three envs.  Pendulum-v1 in the same run: 0.099 ms at 240 offspring (8 lanes), 0.171 ms at 4096 (4 lanes), 200 steps.
int pendula_lanes_per_env(const ses_handle *h, long long episodes)
{
    if (h->cfg.lanes_per_env) return h->cfg.lanes_per_env;
    int lpe = 32;
    while (lpe > 1 && (episodes * lpe + 63) / 64 > 2048) lpe >>= 1;
    return lpe;
}

// Which form of the MLP rollout runs (tune_pendula_generic overrides).  The one-trig form is the default where it was faster
// than the generic form by more than the spread between repeats of the same form (profiles/pendula_timing.txt): swing-up by
// 14 ... 20 % at 4 to 32 lanes (0.457 against 0.533 ms at 240 offspring, 1.00 against 1.17 at 4096; spread below 1 %), the
// double pendulum by 20 ... 25 % (0.063 against 0.082, 0.142 against 0.185; spread 2 ... 5 %).  Balance's outcome reads no trig
// and the compiler merges the generic form's two evaluations of one angle: the forms are within 3 % of each other, one-trig
// ahead at 240 offspring (0.141 against 0.145 ms at 32 lanes), the generic form ahead at 4096 (0.590 against 0.594 at 16, 0.630
// against 0.638 at 8, inside a spread of 2 %) -- not a win beyond the spread, so balance runs the generic form.
template <class EnvP>
static bool pendula_generic_form(const ses_handle *h)
{
    if (h->tune_pendula_generic >= 0) return h->tune_pendula_generic != 0;
    return std::is_same_v<EnvP, InvertedPendulumEnv>;
}

int pendula_rollout(const ses_handle *h, const RolloutArgs &a, int mode)
{
    return with_pendula_env(h->cfg.env_id, [&](auto env) -> int {
        using EnvP = decltype(env);
        SES_REQUIRE(mode == SES_MODE_EPISODIC, "ses_rollout: %s has no fixed-length mode", EnvP::NAME);
        if (h->cfg.gru) {
            launch_rollout_kernel(h, k_rollout_gru_lockstep<PendulaLs<EnvP>, false, 4>, dim3(ceil_div(a.n_rows, 4)), dim3(256), a);
        } else {
            const int lpe = pendula_lanes_per_env(h, a.episodes());
            const bool known = with_lanes<1, 2, 4, 8, 16, 32>(lpe, [&](auto lanes) {
                auto kernel = k_rollout_pendula_mlp<EnvP, lanes(), true>;
                if (pendula_generic_form<EnvP>(h)) kernel = k_rollout_pendula_mlp<EnvP, lanes(), false>;   // (observe / step)
                hipLaunchKernelGGL(kernel, dim3(ceil_div(a.episodes() * lpe, 64)), dim3(64), 0, h->stream, a.theta, a.init, a.per,
                                   a.n_rows, a.E, a.P, a.max_step, a.epr, a.ep_steps);
            });
            if (!known)
                return set_error(SES_ERR_INVALID_ARG, "ses_rollout: %s has no MLP rollout at %d lanes per env (1, 2, 4, 8, 16, 32)",
                                 EnvP::NAME, lpe);
        }
        SES_HIP_TRY(hipGetLastError());
        return SES_OK;
    });
}

// ses_policy_forward at (5, 1) and (9, 1); the caller has checked that (num_state, num_action) is one of them
int pendula_policy_forward(ses_handle *h, const float *theta, const float *obs, float *hidden, int n, float *logits, float *act,
                           int32_t *action)
{
    const int S = h->cfg.num_state, A = h->cfg.num_action;
    if (h->cfg.gru)
        with_policy_shape<PolicyShape<5, 1>, PolicyShape<9, 1>>(S, A, [&](auto sh) {
            hipLaunchKernelGGL((k_policy_forward_gru<sh.S, sh.A>), dim3(ceil_div(n, 4)), dim3(256), 0, h->stream, theta, obs, hidden, n,
                               h->P, logits, act, action);
        });
    else
        with_policy_shape<PolicyShape<5, 1>, PolicyShape<9, 1>>(S, A, [&](auto sh) {
            hipLaunchKernelGGL((k_policy_forward_mlp<sh.S, sh.A>), dim3(ceil_div((long long)n * 4, 64)), dim3(64), 0, h->stream, theta,
                               obs, n, h->P, logits, act, action);
        });
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

}  // namespace ses
