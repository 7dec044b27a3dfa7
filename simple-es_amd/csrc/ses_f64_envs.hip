// ses_f64_envs.hip -- the eight float64 control envs on the device, through every path the other envs have: gym's classic
// control (csrc/ses_classic.h: Acrobot-v1, MountainCar-v0, Pendulum-v1, MountainCarContinuous-v0; gym's order of operations),
// the inverted-pendulum family modelled on pybullet_envs (csrc/ses_pendula.h: balance, swing-up, double) and ReacherBulletEnv-v0
// (csrc/ses_reacher.h) -- the last four the build's own definitions, DESIGN.md 7.
//   k_envs_reset_f64 / k_envs_step_f64     : env.reset() / env.step(a) for n independent envs (ses_env_reset /
//                                            ses_env_step_generic), one lane per env, the blob is the float64 state; the
//                                            action int32[n] or float32[n, A], the reward rounded to float
//   k_rollout_f64_mlp                      : RolloutWorker (loop.py:108-125) with an MLP policy, one kernel per shard: one trig
//                                            per step (ONE_TRIG, trig envs only), or the generic observe / step form
//   k_rollout_gru_lockstep<F64Ls<...>>     : the same with a GRU policy, the lockstep kernel of ses_gru_lockstep.h
//   k_policy_forward_mlp / _gru            : ses_policy_forward for these envs' shapes (GymEnvModel.forward, playback)
// Every kernel is one template over the env adapters (the contract at the top of ses_classic.h); Env::Action (int, or
// float[A]) picks the policy head and the step-wise action layout at compile time.  Episodic mode only.
// The normalising form of the MLP rollout (ses_obs_norm_bind) is a kernel of ses_obs_norm.hip, a code object of its own.
#include "ses_f64_envs.h"
#include "ses_gru_lockstep.h"
#include "ses_internal.h"
#include "ses_policy.h"
#include "ses_policy_forward.h"

namespace ses {

// ---- step-wise envs -----------------------------------------------------------------------------------------------------
template <class Env>
__global__ __launch_bounds__(64) void k_envs_reset_f64(const float *__restrict__ init, int n, typename Env::State *__restrict__ state,
                                                       float *__restrict__ obs)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    typename Env::State st;
    Env::reset(st, init + (size_t)i * Env::INIT_W);
    state[i] = st;
    float o[Env::S];
    Env::observe(st, o);
#pragma unroll
    for (int k = 0; k < Env::S; ++k) obs[(size_t)i * Env::S + k] = o[k];
}

template <class Env>
__global__ __launch_bounds__(64) void k_envs_step_f64(typename Env::State *__restrict__ state,
                                                      const std::remove_extent_t<typename Env::Action> *__restrict__ action, int n,
                                                      float *__restrict__ obs, float *__restrict__ reward, int32_t *__restrict__ done)
{
    constexpr int A = Env::A;
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    typename Env::State st = state[i];
    typename Env::Action act;
    if constexpr (is_discrete<Env>) {
        const int a = action[i];
        act = a < 0 ? 0 : (a > 2 ? 2 : a);                                  // (gym's action spaces are {0, 1, 2}: clamped into it)
    } else {
#pragma unroll
        for (int k = 0; k < A; ++k) act[k] = action[(size_t)i * A + k];     // (any float: the env clips it, never rejects it)
    }
    bool d;
    const auto r = Env::step(st, act, d);
    state[i] = st;
    float o[Env::S];
    Env::observe(st, o);
#pragma unroll
    for (int k = 0; k < Env::S; ++k) obs[(size_t)i * Env::S + k] = o[k];
    reward[i] = (float)r;
    done[i] = d ? 1 : 0;
}

// ---- fused MLP rollouts ---------------------------------------------------------------------------------------------------
// LPE adjacent lanes share one env (env = row * E + episode) as in k_rollout_box2d_mlp without the terrain: every lane of
// the group runs the env's physics (identical bits), the MLP is split over the group -- MlpSlice with the offspring's slice
// in registers for 4 ... 32 lanes per env, streamed from the (L2-resident) row for 1 and 2.  A finished env is frozen, the
// wave leaves as soon as none of its envs is alive; an env that never terminates (Pendulum-v1, swing-up, the Reacher) runs
// every episode to max_step and the whole population in lockstep, so its loop carries no alive flag, no ballot and no frozen
// state.  One env step is a chain of ~15 sin / cos and 16 f64 divisions behind four sequential RK4 stages (Acrobot): at the
// populations ES uses the chip holds far fewer envs than lanes, so the step's dependence chain, not issue, is what a rollout
// costs -- the lanes per env only decide how many waves (and SIMDs) share the population and how short the policy's part of
// the chain is (f64_lanes_per_env).  The return adds the adapter's reward in float64: exact for the discrete envs' float
// rewards, the env's own float64 for the continuous ones.
// ONE_TRIG (trig envs): the trig of a state (one sincos_ieee per angle, the addition formulas) is evaluated once, when the
// state is entered.  It gives the outcome of the step that entered it (swing-up's reward cos theta, the double pendulum's
// x2 / y2 reward and done, the Reacher's pot_new from the fingertip) and, one iteration later, the observation and the
// accelerations of the step that leaves it -- the bits are the same, which is what makes it legal.  The generic form
// (ONE_TRIG false) is Env::observe then Env::step: one trig for the observation, one for the accelerations, one for the
// outcome.  An env with TRIG_ON_EXIT false (Pendulum-v1) has its one trig at the top of the step instead.
template <class Env, int LPE, bool ONE_TRIG>
__global__ __launch_bounds__(64) void k_rollout_f64_mlp(const float *__restrict__ theta, const float *__restrict__ init,
                                                        int init_per_offspring, int n_rows, int E, int P, int max_step,
                                                        double *__restrict__ ep_return, int32_t *__restrict__ ep_steps)
{
    constexpr int S = Env::S, A = Env::A;
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    stage_tanh_table(tanh_tab);
    const long long n_env = (long long)n_rows * E;
    long long env = ((long long)blockIdx.x * 64 + threadIdx.x) / LPE;
    const int sub = (int)(threadIdx.x % LPE);
    const bool valid = env < n_env;
    env = valid ? env : n_env - 1;                                  // lane groups past the last env shadow it
    const int row = (int)(env / E), ep = (int)(env - (long long)row * E);
    const float *th = theta + (size_t)row * P;
    typename Env::State st;
    Env::reset(st, init + ((size_t)(init_per_offspring ? row : 0) * E + ep) * Env::INIT_W);
    MlpSlice<S, A, (LPE >= 4 ? LPE : 4)> net;
    if constexpr (LPE >= 4) net.load(th, sub);
    typename Env::Trig tg;                                          // (empty for an env without the trig form)
    if constexpr (ONE_TRIG) {
        if constexpr (Env::TRIG_ON_EXIT) Env::trig(st, tg);
    }
    double ret = 0.0;
    int steps = 0;
    bool done = false;
    for (int t = 0; t < max_step; ++t) {
        if constexpr (Env::TERMINATES) {
            if (__ballot(!done) == 0ull) break;
        }
        float obs[S], logits[A];
        if constexpr (ONE_TRIG) {
            if constexpr (!Env::TRIG_ON_EXIT) Env::trig(st, tg);
            Env::observe_from(st, tg, obs);
        } else {
            Env::observe(st, obs);
        }
        if constexpr (LPE >= 4) net.forward(tanh_tab, obs, logits);
        else mlp_forward_streamed<S, A, LPE>(th, sub, tanh_tab, obs, logits);
        typename Env::Action action;
        classic_head<Env>(tanh_tab, logits, action);
        if (!Env::TERMINATES || !done) {
            if constexpr (ONE_TRIG) ret += Env::step_from(st, tg, action, done);
            else ret += (double)Env::step(st, action, done);
            steps += 1;
        }
    }
    if (valid && sub == 0) {
        ep_return[env] = ret;
        if (ep_steps) ep_steps[env] = Env::TERMINATES ? steps : max_step;
    }
}

// ---- GRU adapter of the lockstep kernel (the CartPoleLs interface, ses_rollout.hip; the reward is the adapter's own type) ----
template <class Env>
struct F64Ls {
    static constexpr int S = Env::S, A = Env::A, INIT_W = Env::INIT_W;
    struct State {
        typename Env::State st;
    };
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u, int) { Env::reset(s.st, u); }
    __device__ static __forceinline__ void observe(const State &s, float (&obs)[S]) { Env::observe(s.st, obs); }
    __device__ static __forceinline__ auto step(State &s, const float (&logits)[A], const TanhEntry *tab, bool freeze, bool &done)
    {
        typename Env::Action action;
        classic_head<Env>(tab, logits, action);
        typename Env::State ns = s.st;
        const auto r = Env::step(ns, action, done);
        if (!freeze) s.st = ns;                                     // a finished env (or one past max_step) is frozen
        return r;
    }
};

// ---- host side -----------------------------------------------------------------------------------------------------------
int f64_env_state_bytes(const ses_config *cfg)
{
    return with_f64_env(cfg->env_id, [](auto env) { return (int)sizeof(typename decltype(env)::State); });
}

int f64_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs)
{
    return with_f64_env(h->cfg.env_id, [&](auto env) -> int {
        using Env = decltype(env);
        hipLaunchKernelGGL(k_envs_reset_f64<Env>, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, init, n, (typename Env::State *)state,
                           obs);
        SES_HIP_TRY(hipGetLastError());
        return SES_OK;
    });
}

// action: int32[n] for the discrete envs, float32[n, A] for the continuous ones
int f64_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done)
{
    return with_f64_env(h->cfg.env_id, [&](auto env) -> int {
        using Env = decltype(env);
        hipLaunchKernelGGL(k_envs_step_f64<Env>, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, (typename Env::State *)state,
                           (const std::remove_extent_t<typename Env::Action> *)action, n, obs, reward, done);
        SES_HIP_TRY(hipGetLastError());
        return SES_OK;
    });
}

// Lanes per env of the MLP rollout (cfg.lanes_per_env overrides): the largest split up to a cap that keeps the population
// within a wave budget.  Every lane of an env's group repeats the env's float64 physics, so more lanes per env buy a shorter
// policy step and fewer envs per wave (an earlier exit) only while the chip has issue slots to spare for the copies.
//
// The classic-control envs: up to 16 within 1024 waves for Acrobot, up to 16 within 2048 for MountainCar, up to 8 within 2048
// for Pendulum; MountainCarContinuous 32 while the population fits 256 waves, else MountainCar's rule.
// Measured, discrete envs (profiles/classic_control_timing.txt, tools/time_classic.py; 5 episodes, random first-generation
// policies): Acrobot 97 offspring 1.32 ms at 16 or 32 lanes per env against 1.53 at 8; 4096 offspring 2.30 ms at 2 against
// 2.44 / 2.55 / 3.54 at 1 / 4 / 8 -- its 16 f64 divisions and ~15 sin / cos per step make the copies cost issue there;
// MountainCar 240 offspring 0.083 ms at 16 (0.089 / 0.091 at 8 / 32); 4096 offspring 0.151 ms at 4 (0.170 / 0.273 at 8 / 2).
// Measured, continuous envs, the best setting at both population sizes (profiles/classic_control_cont_timing.txt, the same
// tool; 5 episodes to the TimeLimit, random first-generation policies): Pendulum 240 offspring 0.104 ms at 8 (0.122 / 0.111 /
// 0.107 at 4 / 16 / 32), 4096 offspring 0.178 ms at 4 (0.201 / 0.206 at 2 / 8).  MountainCarContinuous at 32 lanes has one
// wave per CU (the copies of the physics cost nobody an issue slot, the policy's part of the chain is shortest) -- 97
// offspring 0.382 ms (0.393 / 0.439 at 16 / 8); 4096 offspring 0.757 ms at 4 (0.83 / 1.54 at 8 / 2).
//
// The inverted-pendulum family: the largest split up to 32 that keeps the population within 2048 waves.
// Measured (profiles/pendula_timing.txt, tools/time_pendula.py; 5 episodes, random first-generation policies, the default form,
// all candidates alternating in one process): swing-up, every episode 1000 steps, 240 offspring 0.457 ms at 32 (0.519 / 0.540 /
// 0.591 at 16 / 8 / 4), 4096 offspring 1.00 ms at 4 (1.02 / 1.20 / 1.73 / 3.18 at 2 / 8 / 16 / 32); the double pendulum, ~21
// steps per episode, 240 offspring 0.063 / 0.064 ms at 16 / 32 (0.070 at 8), 4096 offspring 0.142 ms at 4 (0.153 / 0.181 at 8 /
// 16).  Balance under random policies lasts ~15 steps per episode, so its waves leave early and its first generation would take
// 16 lanes at 4096 offspring (0.590 ms against 0.717 at 4; 240 offspring: 0.145 ms at 32, 0.148 at 16); a population that has
// learnt to balance runs every episode to the cap on the swing-up's transition code, and the rule is set for that: one rule for the
// three envs.  Pendulum-v1 in the same run: 0.099 ms at 240 offspring (8 lanes), 0.171 ms at 4096 (4 lanes), 200 steps.
//
// The Reacher: the largest split up to 16 that keeps the population within 1024 waves -- one wave per SIMD of the 256 CUs.  The
// rule started as the inverted-pendulum family's (up to 32 lanes, 2048 waves), which chose 32 and 4 lanes at the two
// populations below; the measurement replaced it.
// Measured (profiles/reacher_timing.txt, tools/time_reacher.py; 5 episodes x 150 steps, random first-generation policies, the
// one-trig form, all candidates alternating in one process, ms per rollout at 1 / 2 / 4 / 8 / 16 / 32 lanes): 240 offspring
// 0.407 / 0.190 / 0.143 / 0.111 / 0.110 / 0.113 -- 8, 16 and 32 lie within 3 % of each other, the spread of a setting's own
// repeats being up to 2 %, so 16 is a tie-break, not a win; 4096 offspring 0.457 / 0.209 / 0.236 / 0.279 / 0.420 / 0.758 -- 2
// lanes (streamed weights, 640 waves) beat 4 by 11 %, spread 2 %.  GRU: 0.412 and 1.15 ms.  The yardsticks in the same run:
// Pendulum-v1 (200 steps) 0.098 / 0.400 ms (MLP / GRU) at 240 offspring and 0.161 / 1.09 ms at 4096; the double pendulum (~21
// steps per episode) 0.064 / 0.183 and 0.139 / 0.438 ms.  Per env step of the 240 x 5 population that is 0.73 us of kernel
// time for the Reacher against 0.49 us for Pendulum-v1: two sincos, a square root and a division per step against one sincos.
int f64_lanes_per_env(const ses_handle *h, long long episodes)
{
    if (h->cfg.lanes_per_env) return h->cfg.lanes_per_env;
    const auto waves = [&](int lpe) { return (episodes * lpe + 63) / 64; };
    int lpe = 16, budget = 2048;                                    // MountainCar, MountainCarContinuous past 256 waves
    switch (h->cfg.env_id) {
        case SES_ENV_ACROBOT: budget = 1024; break;
        case SES_ENV_PENDULUM: lpe = 8; break;
        case SES_ENV_MOUNTAINCAR_CONT:
            if (waves(32) <= 256) return 32;
            break;
        case SES_ENV_INVERTED_PENDULUM:
        case SES_ENV_PENDULUM_SWINGUP:
        case SES_ENV_DOUBLE_PENDULUM: lpe = 32; break;
        case SES_ENV_REACHER: budget = 1024; break;
    }
    while (lpe > 1 && waves(lpe) > budget) lpe >>= 1;
    return lpe;
}

// Which form of a trig env's MLP rollout runs: true is the generic observe / step form, false the one-trig form.  The tuning
// names "pendulum_generic_step" (0 / 1), "pendula_generic_step" and "reacher_generic_step" (-1: the default / 0 / 1) override.
//
// Pendulum-v1: the one-trig form -- sincos_ieee runs once per step and serves the dynamics and the observation.
//
// The inverted-pendulum family: the one-trig form is the default where it was faster than the generic form by more than the
// spread between repeats of the same form (profiles/pendula_timing.txt): swing-up by 14 ... 20 % at 4 to 32 lanes (0.457
// against 0.533 ms at 240 offspring, 1.00 against 1.17 at 4096; spread below 1 %), the double pendulum by 20 ... 25 % (0.063
// against 0.082, 0.142 against 0.185; spread 2 ... 5 %).  Balance's outcome reads no trig and the compiler merges the generic
// form's two evaluations of one angle: the forms are within 3 % of each other, one-trig ahead at 240 offspring (0.141 against
// 0.145 ms at 32 lanes), the generic form ahead at 4096 (0.590 against 0.594 at 16, 0.630 against 0.638 at 8, inside a spread
// of 2 %) -- not a win beyond the spread, so balance runs the generic form.
//
// The Reacher: the one-trig form.  It was faster than the generic form at every lane count by far more than the spread
// (profiles/reacher_timing.txt): 0.110 against 0.159 ms at 240 offspring and 16 lanes, 0.209 against 0.245 ms at 4096
// offspring and 2 lanes; between 8 % (1 lane) and 31 % (16 lanes) overall.
bool f64_generic_form(const ses_handle *h)
{
    switch (h->cfg.env_id) {
        case SES_ENV_PENDULUM: return h->tune.pendulum_generic != 0;
        case SES_ENV_INVERTED_PENDULUM: return h->tune.pendula_generic != 0;    // (-1: balance runs the generic form)
        case SES_ENV_PENDULUM_SWINGUP:
        case SES_ENV_DOUBLE_PENDULUM: return h->tune.pendula_generic > 0;
        default: return h->tune.reacher_generic > 0;
    }
}

int f64_rollout(ses_handle *h, const RolloutArgs &a, const RolloutPlan &, int mode)
{
    return with_f64_env(h->cfg.env_id, [&](auto env) -> int {
        using Env = decltype(env);
        SES_REQUIRE(mode == SES_MODE_EPISODIC, "ses_rollout: %s has no fixed-length mode", Env::NAME);
        if (h->cfg.gru) {
            launch_rollout_kernel(h, k_rollout_gru_lockstep<F64Ls<Env>, false, 4>, dim3(ceil_div(a.n_rows, 4)), dim3(256), a);
        } else if (a.norm_affine) {
            return f64_rollout_norm(h, a);                           // a normaliser is bound to the handle: ses_obs_norm.hip
        } else {
            const int lpe = f64_lanes_per_env(h, a.episodes());
            const bool known = with_lanes<1, 2, 4, 8, 16, 32>(lpe, [&](auto lanes) {
                auto kernel = k_rollout_f64_mlp<Env, lanes(), false>;
                if constexpr (Env::HAS_TRIG) {
                    if (!f64_generic_form(h)) kernel = k_rollout_f64_mlp<Env, lanes(), true>;
                }
                hipLaunchKernelGGL(kernel, dim3(ceil_div(a.episodes() * lpe, 64)), dim3(64), 0, h->stream, a.theta, a.init, a.per,
                                   a.n_rows, a.E, a.P, a.max_step, a.epr, a.ep_steps);
            });
            if (!known)
                return set_error(SES_ERR_INVALID_ARG, "ses_rollout: %s has no MLP rollout at %d lanes per env (1, 2, 4, 8, 16, 32)",
                                 Env::NAME, lpe);
        }
        SES_HIP_TRY(hipGetLastError());
        return SES_OK;
    });
}

// ses_policy_forward for the shapes of the eight envs; the caller has checked that (num_state, num_action) is one of them
// (is_f64_policy_shape)
int f64_policy_forward(ses_handle *h, const float *theta, const float *obs, float *hidden, int n, float *logits, float *act,
                       int32_t *action)
{
    const auto with_shape = [&](auto &&f) {
        with_policy_shape<PolicyShape<6, 3>, PolicyShape<2, 3>, PolicyShape<3, 1>, PolicyShape<2, 1>, PolicyShape<5, 1>, PolicyShape<9, 1>,
                          PolicyShape<9, 2>>(h->cfg.num_state, h->cfg.num_action, f);
    };
    if (h->cfg.gru)
        with_shape([&](auto sh) {
            hipLaunchKernelGGL((k_policy_forward_gru<sh.S, sh.A>), dim3(ceil_div(n, 4)), dim3(256), 0, h->stream, theta, obs, hidden, n,
                               h->P, logits, act, action);
        });
    else
        with_shape([&](auto sh) {
            hipLaunchKernelGGL((k_policy_forward_mlp<sh.S, sh.A>), dim3(ceil_div((long long)n * 4, 64)), dim3(64), 0, h->stream, theta,
                               obs, n, h->P, logits, act, action);
        });
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

}  // namespace ses
