// ses_reacher.hip -- ReacherBulletEnv-v0 modelled on pybullet_envs (csrc/ses_reacher.h: float64, the build's own definition;
// DESIGN.md 7) on the device, through every path the inverted-pendulum family has:
//   k_envs_reset_reacher / k_envs_step_reacher : env.reset() / env.step(a) for n independent envs (ses_env_reset /
//                                                ses_env_step_generic), one lane per env, the blob is the float64 state (56 B);
//                                                the action float32[n, 2], the reward rounded to float
//   k_rollout_reacher_mlp                      : RolloutWorker (loop.py:108-125) with an MLP policy, one kernel per shard: one
//                                                trig per step (ONE_TRIG), or the generic observe / step form (its A/B partner)
//   k_rollout_gru_lockstep<ReacherLs>          : the same with a GRU policy, the lockstep kernel of ses_gru_lockstep.h
//   k_policy_forward_mlp / _gru                : ses_policy_forward at (9, 2) (GymEnvModel.forward, playback)
// The first unit of the family whose policies have TWO tanh outputs.  Episodic mode only.  A unit of its own: the kernels of
// the other units keep their machine code byte for byte.
#include "ses_reacher.h"
#include "ses_gru_lockstep.h"
#include "ses_internal.h"
#include "ses_policy.h"
#include "ses_policy_forward.h"

namespace ses {

// ---- step-wise env ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_envs_reset_reacher(const float *__restrict__ init, int n, ReacherState *__restrict__ state,
                                                           float *__restrict__ obs)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    ReacherState st;
    ReacherEnv::reset(st, init + (size_t)i * ReacherEnv::INIT_W);
    state[i] = st;
    float o[ReacherEnv::S];
    ReacherEnv::observe(st, o);
#pragma unroll
    for (int k = 0; k < ReacherEnv::S; ++k) obs[(size_t)i * ReacherEnv::S + k] = o[k];
}

__global__ __launch_bounds__(64) void k_envs_step_reacher(ReacherState *__restrict__ state, const float *__restrict__ action, int n,
                                                          float *__restrict__ obs, float *__restrict__ reward, int32_t *__restrict__ done)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    ReacherState st = state[i];
    const float act[2] = {action[(size_t)i * 2], action[(size_t)i * 2 + 1]};   // (any floats: the env clips them, never rejects them)
    bool d;
    const double r = ReacherEnv::step(st, act, d);
    state[i] = st;
    float o[ReacherEnv::S];
    ReacherEnv::observe(st, o);
#pragma unroll
    for (int k = 0; k < ReacherEnv::S; ++k) obs[(size_t)i * ReacherEnv::S + k] = o[k];
    reward[i] = (float)r;
    done[i] = d ? 1 : 0;
}

// ---- fused MLP rollout ----------------------------------------------------------------------------------------------------
// LPE adjacent lanes share one env (env = row * E + episode) as in k_rollout_pendula_mlp: every lane of the group runs the
// env's physics (identical bits), the MLP is split over the group -- MlpSlice<9, 2, LPE> with the offspring's slice in
// registers for 4 ... 32 lanes per env, streamed from the (L2-resident) row for 1 and 2.
// ONE_TRIG: the trig of a state (two sincos_ieee and the addition formulas) is evaluated once, when the state is entered.  It
// gives the outcome of the step that entered it (pot_new, from the fingertip) and, one iteration later, the observation (the
// same fingertip) and the mass matrix of the step that leaves it -- the bits are the same, which is what makes it legal.  The
// generic form (ONE_TRIG false) is ReacherEnv::observe then ReacherEnv::step: one trig for the observation, one for the
// dynamics, one for the outcome.
// The env never terminates: the loop carries no alive flag, no ballot and no frozen state; every episode is max_step steps.
template <int LPE, bool ONE_TRIG = true>
__global__ __launch_bounds__(64) void k_rollout_reacher_mlp(const float *__restrict__ theta, const float *__restrict__ init,
                                                            int init_per_offspring, int n_rows, int E, int P, int max_step,
                                                            double *__restrict__ ep_return, int32_t *__restrict__ ep_steps)
{
    constexpr int S = ReacherEnv::S, A = ReacherEnv::A;
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    stage_tanh_table(tanh_tab);
    const long long n_env = (long long)n_rows * E;
    long long env = ((long long)blockIdx.x * 64 + threadIdx.x) / LPE;
    const int sub = (int)(threadIdx.x % LPE);
    const bool valid = env < n_env;
    env = valid ? env : n_env - 1;                                  // lane groups past the last env shadow it
    const int row = (int)(env / E), ep = (int)(env - (long long)row * E);
    const float *th = theta + (size_t)row * P;
    ReacherState st;
    ReacherEnv::reset(st, init + ((size_t)(init_per_offspring ? row : 0) * E + ep) * ReacherEnv::INIT_W);
    MlpSlice<S, A, (LPE >= 4 ? LPE : 4)> net;
    if constexpr (LPE >= 4) net.load(th, sub);
    ReacherTrig tg;
    if constexpr (ONE_TRIG) ReacherEnv::trig(st, tg);
    double ret = 0.0;
    for (int t = 0; t < max_step; ++t) {
        float obs[S], logits[A];
        if constexpr (ONE_TRIG) ReacherEnv::observe_from(st, tg, obs);
        else ReacherEnv::observe(st, obs);
        if constexpr (LPE >= 4) net.forward(tanh_tab, obs, logits);
        else mlp_forward_streamed<S, A, LPE>(th, sub, tanh_tab, obs, logits);
        const float act[A] = {tanh_(tanh_tab, logits[0]), tanh_(tanh_tab, logits[1])};
        if constexpr (ONE_TRIG) {
            double a[A];
            ReacherEnv::clip_action(act, a);
            reacher_advance(st, tg, a[0], a[1]);
            ReacherEnv::trig(st, tg);
            ret += reacher_outcome(st, tg, a[0], a[1]);
        } else {
            bool done;
            ret += ReacherEnv::step(st, act, done);
        }
    }
    if (valid && sub == 0) {
        ep_return[env] = ret;
        if (ep_steps) ep_steps[env] = max_step;
    }
}

// ---- GRU adapter of the lockstep kernel (the PendulaLs shape; both tanh outputs go to the env) ------------------------------
struct ReacherLs {
    static constexpr int S = ReacherEnv::S, A = ReacherEnv::A, INIT_W = ReacherEnv::INIT_W;
    struct State {
        ReacherState st;
    };
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u, int) { ReacherEnv::reset(s.st, u); }
    __device__ static __forceinline__ void observe(const State &s, float (&obs)[S]) { ReacherEnv::observe(s.st, obs); }
    __device__ static __forceinline__ double step(State &s, const float (&logits)[A], const TanhEntry *tab, bool freeze, bool &done)
    {
        const float act[A] = {tanh_(tab, logits[0]), tanh_(tab, logits[1])};
        ReacherState ns = s.st;
        const double r = ReacherEnv::step(ns, act, done);
        if (!freeze) s.st = ns;                                     // (an env past max_step is frozen; the env itself never ends)
        return r;
    }
};

// ---- host side -----------------------------------------------------------------------------------------------------------
int reacher_env_state_bytes() { return (int)sizeof(ReacherState); }

int reacher_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs)
{
    hipLaunchKernelGGL(k_envs_reset_reacher, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, init, n, (ReacherState *)state, obs);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

// action: float32[n, 2]
int reacher_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done)
{
    hipLaunchKernelGGL(k_envs_step_reacher, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, (ReacherState *)state, (const float *)action, n,
                       obs, reward, done);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

// Lanes per env of the MLP rollout (cfg.lanes_per_env overrides): the largest split up to 16 that keeps the population within
// 1024 waves -- one wave per SIMD of the 256 CUs.  Every lane of an env's group repeats the env's float64 physics, so more
// lanes per env buy a shorter policy step only while the chip has issue slots to spare for the copies.  The rule started as
// the inverted-pendulum family's (up to 32 lanes, 2048 waves), which chose 32 and 4 lanes at the two populations below; the
// measurement replaced it.
// Measured (profiles/reacher_timing.txt, tools/time_reacher.py; 5 episodes x 150 steps, random first-generation policies, the
// one-trig form, all candidates alternating in one process, ms per rollout at 1 / 2 / 4 / 8 / 16 / 32 lanes): 240 offspring
// 0.407 / 0.190 / 0.143 / 0.111 / 0.110 / 0.113 -- 8, 16 and 32 lie within 3 % of each other, the spread of a setting's own
// repeats being up to 2 %, so 16 is a tie-break, not a win; 4096 offspring 0.457 / 0.209 / 0.236 / 0.279 / 0.420 / 0.758 -- 2
// lanes (streamed weights, 640 waves) beat 4 by 11 %, spread 2 %.  GRU: 0.412 and 1.15 ms.  The yardsticks in the same run:
// Pendulum-v1 (200 steps) 0.098 / 0.400 ms (MLP / GRU) at 240 offspring and 0.161 / 1.09 ms at 4096; the double pendulum (~21
// steps per episode) 0.064 / 0.183 and 0.139 / 0.438 ms.  Per env step of the 240 x 5 population that is 0.73 us of kernel
// time for the Reacher against 0.49 us for Pendulum-v1: two sincos, a square root and a division per step against one sincos.
int reacher_lanes_per_env(const ses_handle *h, long long episodes)
{
    if (h->cfg.lanes_per_env) return h->cfg.lanes_per_env;
    int lpe = 16;
    while (lpe > 1 && (episodes * lpe + 63) / 64 > 1024) lpe >>= 1;
    return lpe;
}

// Which form of the MLP rollout runs ("reacher_generic_step" overrides): the one-trig form.  It was faster than the generic
// form at every lane count by far more than the spread (profiles/reacher_timing.txt): 0.110 against 0.159 ms at 240 offspring
// and 16 lanes, 0.209 against 0.245 ms at 4096 offspring and 2 lanes; between 8 % (1 lane) and 31 % (16 lanes) overall.
static bool reacher_generic_form(const ses_handle *h) { return h->tune_reacher_generic > 0; }

int reacher_rollout(const ses_handle *h, const RolloutArgs &a, int mode)
{
    SES_REQUIRE(mode == SES_MODE_EPISODIC, "ses_rollout: %s has no fixed-length mode", ReacherEnv::NAME);
    if (h->cfg.gru) {
        launch_rollout_kernel(h, k_rollout_gru_lockstep<ReacherLs, false, 4>, dim3(ceil_div(a.n_rows, 4)), dim3(256), a);
    } else {
        const int lpe = reacher_lanes_per_env(h, a.episodes());
        const bool known = with_lanes<1, 2, 4, 8, 16, 32>(lpe, [&](auto lanes) {
            auto kernel = k_rollout_reacher_mlp<lanes(), true>;
            if (reacher_generic_form(h)) kernel = k_rollout_reacher_mlp<lanes(), false>;   // (observe / step)
            hipLaunchKernelGGL(kernel, dim3(ceil_div(a.episodes() * lpe, 64)), dim3(64), 0, h->stream, a.theta, a.init, a.per,
                               a.n_rows, a.E, a.P, a.max_step, a.epr, a.ep_steps);
        });
        if (!known)
            return set_error(SES_ERR_INVALID_ARG, "ses_rollout: %s has no MLP rollout at %d lanes per env (1, 2, 4, 8, 16, 32)",
                             ReacherEnv::NAME, lpe);
    }
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

// ses_policy_forward at (9, 2); the caller has checked the shape
int reacher_policy_forward(ses_handle *h, const float *theta, const float *obs, float *hidden, int n, float *logits, float *act,
                           int32_t *action)
{
    if (h->cfg.gru)
        hipLaunchKernelGGL((k_policy_forward_gru<9, 2>), dim3(ceil_div(n, 4)), dim3(256), 0, h->stream, theta, obs, hidden, n, h->P, logits,
                           act, action);
    else
        hipLaunchKernelGGL((k_policy_forward_mlp<9, 2>), dim3(ceil_div((long long)n * 4, 64)), dim3(64), 0, h->stream, theta, obs, n, h->P,
                           logits, act, action);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

}  // namespace ses
