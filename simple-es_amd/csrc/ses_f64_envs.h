// ses_f64_envs.h -- what the units that run the eight float64 control envs share (ses_f64_envs.hip, ses_obs_norm.hip): the
// adapters, the policy head, env_id -> adapter, and the two launch rules of the MLP rollout.
#pragma once
#include "ses_pendula.h"
#include "ses_reacher.h"
#include "ses_env_table.h"
#include "ses_policy.h"

namespace ses {

template <class Env>
constexpr bool is_discrete = std::is_same_v<typename Env::Action, int>;

// the policy head: the first argmax of the A outputs (discrete), or tanh_ of each (continuous)
template <class Env>
__device__ __forceinline__ void classic_head(const TanhEntry *tab, const float (&logits)[Env::A], typename Env::Action &action)
{
    if constexpr (is_discrete<Env>) {
        action = argmax_first<Env::A>(logits);
    } else {
#pragma unroll
        for (int k = 0; k < Env::A; ++k) action[k] = tanh_(tab, logits[k]);
    }
}

// env_id -> adapter: returns f(Env{}) for the adapter of a float64 env_id (is_f64_env; visited in the order listed).  f is a
// generic lambda that names the kernel instances with decltype of its argument.
template <class F>
inline int with_f64_env(int env_id, F &&f)
{
    switch (env_id) {
        case SES_ENV_ACROBOT: return f(AcrobotEnv{});
        case SES_ENV_MOUNTAINCAR: return f(MountainCarEnv{});
        case SES_ENV_PENDULUM: return f(PendulumEnv{});
        case SES_ENV_MOUNTAINCAR_CONT: return f(MountainCarContEnv{});
        case SES_ENV_INVERTED_PENDULUM: return f(InvertedPendulumEnv{});
        case SES_ENV_PENDULUM_SWINGUP: return f(PendulumSwingupEnv{});
        case SES_ENV_DOUBLE_PENDULUM: return f(DoublePendulumEnv{});
        default: return f(ReacherEnv{});
    }
}

// lanes per env and step form of the MLP rollout for this handle and population (ses_f64_envs.hip holds the rules and what was measured)
int f64_lanes_per_env(const ses_handle *h, long long episodes);
bool f64_generic_form(const ses_handle *h);
int f64_rollout_norm(const ses_handle *h, const RolloutArgs &a);   // ses_obs_norm.hip

}  // namespace ses
