// ses_envs.hip -- step-wise device entry for EVERY env of the library: one lane = one env, state in an opaque
// caller-owned blob (ses_env_state_bytes per env).  This is `env.reset()` / `env.step(action)` of the reference's
// wrappers (envs/gym_wrapper.py:23-45, envs/pettingzoo_wrapper.py:22-58) for n independent envs at once: the kernels
// call the SAME device functions the fused rollouts call (cartpole_step_general, ll_step, bw_step, spread_step), so an
// env can be stepped, inspected and compared with the oracle's env objects one transition at a time, and the
// reference's playback loop (test.py:53-63) runs against the wrappers for every supported env.
//
// Blob layout (opaque to the caller, fixed per handle): CartPole {x, xd, th, thd}; simple_spread SpreadState<NA> + the
// cycle counter; LunarLander (LanderBlob, ses_lander.h) / BipedalWalker the env struct of the Box2D-style world followed by the episode's terrain
// heights (the fused rollouts keep those in LDS; here they live in the blob and the env reads them through the same
// pointer); the float64 control envs, waterworld and pursuit: their own units (ses_f64_envs.hip, ses_waterworld.hip, ses_pursuit.hip).  Truncation at env.max_step is the wrapper's job (gym_wrapper.py:37-39), as in the reference.
#include "ses_cartpole.h"
#include "ses_env_table.h"
#include "ses_lander.h"
#include "ses_policy.h"
#include "ses_spread.h"
#include "ses_walker.h"
#include "ses_env_blobs.h"   // CartPoleBlob, SpreadBlob<NA>, WalkerBlob (shared with ses_render.hip)

namespace ses {

constexpr int SPREAD_MAX_CYCLES = 25;        // pettingzoo mpe default max_cycles: every agent is done after 25 cycles

__device__ __forceinline__ void store_obs_masked(float *__restrict__ dst, const float *obs, int S, uint32_t obs_mask)
{
    for (int k = 0; k < S; ++k) dst[k] = ((obs_mask >> k) & 1u) ? 0.0f : obs[k];
}

// ---- CartPole --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_envs_reset_cartpole(const float *__restrict__ init, int n, CartPoleBlob *__restrict__ state,
                                                            float *__restrict__ obs, uint32_t obs_mask)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float *u = init + (size_t)i * 4;
    const CartPoleState st{u[0], u[1], u[2], u[3]};
    state[i].st = st;
    const float o[4] = {st.x, st.xd, st.th, st.thd};
    store_obs_masked(obs + (size_t)i * 4, o, 4, obs_mask);
}

__global__ __launch_bounds__(64) void k_envs_step_cartpole(CartPoleBlob *__restrict__ state, const int32_t *__restrict__ action, int n,
                                                           float *__restrict__ obs, float *__restrict__ reward,
                                                           int32_t *__restrict__ done, uint32_t obs_mask)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    CartPoleState st = state[i].st;
    const bool term = cartpole_step_general(st, action[i]);
    state[i].st = st;
    const float o[4] = {st.x, st.xd, st.th, st.thd};
    store_obs_masked(obs + (size_t)i * 4, o, 4, obs_mask);
    reward[i] = 1.0f;
    done[i] = term ? 1 : 0;
}

// ---- simple_spread -----------------------------------------------------------------------------------------------
template <int NA>
__device__ __forceinline__ void spread_store_obs(const SpreadState<NA> &st, float *__restrict__ dst)
{
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        float o[6 * NA];
        spread_obs<NA>(st, a, o);
#pragma unroll
        for (int k = 0; k < 6 * NA; ++k) dst[a * 6 * NA + k] = o[k];
    }
}

template <int NA>
__global__ __launch_bounds__(64) void k_envs_reset_spread(const float *__restrict__ init, int n, SpreadBlob<NA> *__restrict__ state,
                                                          float *__restrict__ obs)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float *s0 = init + (size_t)i * (4 * NA);
    SpreadState<NA> st;
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        st.ax[a] = s0[2 * a]; st.ay[a] = s0[2 * a + 1];
        st.vx[a] = 0.0f; st.vy[a] = 0.0f;
        st.lx[a] = s0[2 * NA + 2 * a]; st.ly[a] = s0[2 * NA + 2 * a + 1];
    }
    state[i].st = st;
    state[i].cycle = 0;
    spread_store_obs<NA>(st, obs + (size_t)i * NA * 6 * NA);
}

template <int NA>
__global__ __launch_bounds__(64) void k_envs_step_spread(SpreadBlob<NA> *__restrict__ state, const int32_t *__restrict__ action, int n,
                                                         float *__restrict__ obs, float *__restrict__ reward,
                                                         int32_t *__restrict__ done)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    SpreadState<NA> st = state[i].st;
    int act[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) act[a] = action[(size_t)i * NA + a];
    const float r = spread_step<NA>(st, act);
    const int cycle = state[i].cycle + 1;
    state[i].st = st;
    state[i].cycle = cycle;
    spread_store_obs<NA>(st, obs + (size_t)i * NA * 6 * NA);
    reward[i] = r;
    done[i] = cycle >= SPREAD_MAX_CYCLES ? 1 : 0;
}

// ---- the Box2D-style envs ------------------------------------------------------------------------------------------
// One lane per env: a wave steps 64 different worlds at once (ll_step / bw_step contain no wave-level operation).
__global__ __launch_bounds__(64, 2) void k_envs_reset_lander(const float *__restrict__ init, int n, LanderBlob *__restrict__ state,
                                                             float *__restrict__ obs, uint32_t obs_mask)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    LanderBlob &b = state[i];
    LanderState s;
    ll_reset(s, init + (size_t)i * 16, b.ty);                  // the terrain row is the blob's own (ll_reset ends with the no-op step)
    b.env = s.env;
    float o[8];
    ll_obs(s, o);
    store_obs_masked(obs + (size_t)i * 8, o, 8, obs_mask);
}

__global__ __launch_bounds__(64, 2) void k_envs_step_lander(LanderBlob *__restrict__ state, const float *__restrict__ action, int A, int n,
                                                            float *__restrict__ obs, float *__restrict__ reward,
                                                            int32_t *__restrict__ done, uint32_t obs_mask)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    LanderBlob &b = state[i];
    LanderState s;
    s.env = b.env;
    s.ty = b.ty;
    bool d;
    const float r = ll_step(s, action[(size_t)i * A], action[(size_t)i * A + 1], d);   // the env uses outputs 0 and 1
    b.env = s.env;
    float o[8];
    ll_obs(s, o);
    store_obs_masked(obs + (size_t)i * 8, o, 8, obs_mask);
    reward[i] = r;
    done[i] = d ? 1 : 0;
}

__global__ __launch_bounds__(64, 1) void k_envs_reset_walker(const float *__restrict__ init, int n, WalkerBlob *__restrict__ state,
                                                             float *__restrict__ obs)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    WalkerBlob &b = state[i];
    WalkerState s;
    bw_reset(s, init + (size_t)i * 4, b.ty);
    b.env = s.env;
    float o[24];
    bw_obs(s, o);
    store_obs_masked(obs + (size_t)i * 24, o, 24, 0u);
}

__global__ __launch_bounds__(64, 1) void k_envs_step_walker(WalkerBlob *__restrict__ state, const float *__restrict__ action, int n,
                                                            float *__restrict__ obs, float *__restrict__ reward,
                                                            int32_t *__restrict__ done)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    WalkerBlob &b = state[i];
    WalkerState s;
    s.env = b.env;
    s.ty = b.ty;
    const float *a = action + (size_t)i * 4;
    bool d;
    const float r = bw_step(s, a[0], a[1], a[2], a[3], d);
    b.env = s.env;
    float o[24];
    bw_obs(s, o);
    store_obs_masked(obs + (size_t)i * 24, o, 24, 0u);
    reward[i] = r;
    done[i] = d ? 1 : 0;
}

// ---- the entry functions of this unit's four envs (EnvDesc: ses_env_table.h) ------------------------------------------------------
template <class K, class... X>
static int launch_per_env(const ses_handle *h, K kernel, int n, X... args)          // one lane per env, 64 to a workgroup
{
    hipLaunchKernelGGL(kernel, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, args...);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

static int cartpole_state_bytes(const ses_config *) { return (int)sizeof(CartPoleBlob); }
static int spread_state_bytes(const ses_config *cfg) { return cfg->n_agents == 2 ? (int)sizeof(SpreadBlob<2>) : (int)sizeof(SpreadBlob<3>); }
static int lander_state_bytes(const ses_config *) { return (int)sizeof(LanderBlob); }
static int walker_state_bytes(const ses_config *) { return (int)sizeof(WalkerBlob); }

static int cartpole_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs)
{
    return launch_per_env(h, k_envs_reset_cartpole, n, init, n, (CartPoleBlob *)state, obs, h->obs_mask);
}
static int spread_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs)
{
    if (h->cfg.n_agents == 2) return launch_per_env(h, k_envs_reset_spread<2>, n, init, n, (SpreadBlob<2> *)state, obs);
    return launch_per_env(h, k_envs_reset_spread<3>, n, init, n, (SpreadBlob<3> *)state, obs);
}
static int lander_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs)
{
    return launch_per_env(h, k_envs_reset_lander, n, init, n, (LanderBlob *)state, obs, h->obs_mask);
}
static int walker_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs)
{
    return launch_per_env(h, k_envs_reset_walker, n, init, n, (WalkerBlob *)state, obs);
}

static int cartpole_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done)
{
    return launch_per_env(h, k_envs_step_cartpole, n, (CartPoleBlob *)state, (const int32_t *)action, n, obs, reward, done, h->obs_mask);
}
static int spread_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done)
{
    if (h->cfg.n_agents == 2)
        return launch_per_env(h, k_envs_step_spread<2>, n, (SpreadBlob<2> *)state, (const int32_t *)action, n, obs, reward, done);
    return launch_per_env(h, k_envs_step_spread<3>, n, (SpreadBlob<3> *)state, (const int32_t *)action, n, obs, reward, done);
}
static int lander_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done)
{
    if (h->cfg.discrete_action)                                       // LunarLander-v2: int32[n] actions (ses_lander_discrete.hip)
        return lander_discrete_env_step(h, state, (const int32_t *)action, n, obs, reward, done);
    return launch_per_env(h, k_envs_step_lander, n, (LanderBlob *)state, (const float *)action, h->cfg.num_action, n, obs, reward, done,
                          h->obs_mask);
}
static int walker_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done)
{
    return launch_per_env(h, k_envs_step_walker, n, (WalkerBlob *)state, (const float *)action, n, obs, reward, done);
}

// ---- THE ENV TABLE: one row per env_id.  A new env is its own unit, one row here and one record in ses/envs.py. -----------------
// Columns as EnvDesc declares them:
//   id, name | S, S per agent, A, discrete | n_agents lo, hi | gru, pomdp, physics64 accepted, pomdp mask | eval_ep_num cap |
//   init row: width, width per agent, lo, hi | ep_steps, float64 env | state bytes, reset, step, rollout
// pomdp masks: CartPole obs[1], obs[3] (gym_wrapper.py:73-77); LunarLander obs[2, 3, 5] (gym_wrapper.py:61-66).  Init rows: CartPole x, xd,
// th, thd; simple_spread agent and landmark positions; LunarLander force, terrain heights, noise key (ses_lander.h); BipedalWalker force
// uniform, two terrain-key words, pad (ses_walker.h); the float64 envs as include/ses.h says per env; waterworld positions, headings,
// respawn key (ses_waterworld.h); pursuit pursuer cells, evader cells, evader-move key (ses_pursuit.h); the hopper its three joint angles
// (ses_hopper_env.h); Walker2D its six (ses_walker2d_env.h); BipedalWalkerHardcore-v3 BipedalWalker's row (ses_walker_hardcore_env.h).
#define SES_F64_ROW(id, name, S, A, discrete, init_w, lo, hi)                                                                      \
    {id, name, S, 0, A, discrete, 0, 0, true, false, false, 0u, 0, init_w, 0, lo, hi, true, true,                                  \
     f64_env_state_bytes, f64_env_reset, f64_env_step, f64_rollout}
// (a host function's static: the device half of the unit never sees host function pointers)
const EnvDesc *env_table_row(int i)
{
    static const EnvDesc table[] = {
    {SES_ENV_CARTPOLE, "CartPole", 4, 0, 2, 1, 0, 0, true, true, true, 0xAu, 0, 4, 0, -0.05, 0.05, true, false,
     cartpole_state_bytes, cartpole_env_reset, cartpole_env_step, rollout_cartpole},
    {SES_ENV_LUNARLANDER, "LunarLander", 8, 0, 4, EITHER, 0, 0, true, true, false, 0x2Cu, 0, 16, 0, 0.0, 1.0, true, false,
     lander_state_bytes, lander_env_reset, lander_env_step, rollout_lander},
    {SES_ENV_SIMPLE_SPREAD, "simple_spread", 0, 6, 5, 1, 2, 3, true, false, false, 0u, 0, 0, 4, -1.0, 1.0, false, false,
     spread_state_bytes, spread_env_reset, spread_env_step, rollout_spread},
    {SES_ENV_BIPEDALWALKER, "BipedalWalker", 24, 0, 4, 0, 0, 0, false, false, false, 0u, 0, 4, 0, 0.0, 1.0, true, false,
     walker_state_bytes, walker_env_reset, walker_env_step, rollout_walker},
    SES_F64_ROW(SES_ENV_ACROBOT, "Acrobot-v1", 6, 3, 1, 4, -0.1, 0.1),
    SES_F64_ROW(SES_ENV_MOUNTAINCAR, "MountainCar-v0", 2, 3, 1, 1, -0.6, -0.4),
    SES_F64_ROW(SES_ENV_PENDULUM, "Pendulum-v1", 3, 1, 0, 2, -1.0, 1.0),
    SES_F64_ROW(SES_ENV_MOUNTAINCAR_CONT, "MountainCarContinuous-v0", 2, 1, 0, 1, -0.6, -0.4),
    {SES_ENV_WATERWORLD, "waterworld", 242, 0, 2, 0, 5, 5, false, false, false, 0u, 16, 72, 0, 0.0, 1.0, true, false,
     waterworld_env_state_bytes, waterworld_env_reset, waterworld_env_step, waterworld_rollout},
    SES_F64_ROW(SES_ENV_INVERTED_PENDULUM, "InvertedPendulumBulletEnv-v0", 5, 1, 0, 1, -0.1, 0.1),
    SES_F64_ROW(SES_ENV_PENDULUM_SWINGUP, "InvertedPendulumSwingupBulletEnv-v0", 5, 1, 0, 1, -0.1, 0.1),
    SES_F64_ROW(SES_ENV_DOUBLE_PENDULUM, "InvertedDoublePendulumBulletEnv-v0", 9, 1, 0, 2, -0.1, 0.1),
    {SES_ENV_PURSUIT, "pursuit", 147, 0, 5, 1, 8, 8, false, false, false, 0u, 16, 40, 0, 0.0, 1.0, true, false,
     pursuit_env_state_bytes, pursuit_env_reset, pursuit_env_step, pursuit_rollout},
    SES_F64_ROW(SES_ENV_REACHER, "ReacherBulletEnv-v0", 9, 2, 0, 4, -1.0, 1.0),
    {SES_ENV_HOPPER, "HopperBulletEnv-v0", 15, 0, 3, 0, 0, 0, true, false, false, 0u, 0, 3, 0, -0.1, 0.1, true, false,
     hopper_env_state_bytes, hopper_env_reset, hopper_env_step, hopper_rollout},
    {SES_ENV_WALKER2D, "Walker2DBulletEnv-v0", 22, 0, 6, 0, 0, 0, true, false, false, 0u, 0, 6, 0, -0.1, 0.1, true, false,
     walker2d_env_state_bytes, walker2d_env_reset, walker2d_env_step, walker2d_rollout},
    {SES_ENV_BIPEDALWALKER_HARDCORE, "BipedalWalkerHardcore-v3", 24, 0, 4, 0, 0, 0, true, false, false, 0u, 0, 4, 0, 0.0, 1.0, true, false,
     walker_hardcore_env_state_bytes, walker_hardcore_env_reset, walker_hardcore_env_step, walker_hardcore_rollout},
    };
    return i >= 0 && i < (int)(sizeof table / sizeof table[0]) ? &table[i] : nullptr;
}
#undef SES_F64_ROW

const EnvDesc *env_desc(int env_id)
{
    for (int i = 0; const EnvDesc *d = env_table_row(i); ++i)
        if (d->env_id == env_id) return d;
    return nullptr;
}

const EnvDesc *env_desc(const ses_handle *h) { return env_desc(h->cfg.env_id); }

int env_check_config(const char *who, const ses_config *cfg, const EnvDesc **row)
{
    *row = nullptr;
    if (cfg->env_id == SES_ENV_NONE) return SES_OK;
    const EnvDesc *d = env_desc(cfg->env_id);
    SES_REQUIRE(d, "%s: unknown env_id %d", who, cfg->env_id);
    int rc = SES_OK;                                                  // the first field outside [lo, hi] is the one reported
    const auto need = [&](const char *field, int lo, int hi, int have, const char *note) {
        if (rc != SES_OK || (have >= lo && have <= hi)) return;
        char want[32];
        if (lo == hi) snprintf(want, sizeof want, "%d", lo);
        else snprintf(want, sizeof want, "%d .. %d", lo, hi);
        rc = set_error(SES_ERR_INVALID_ARG, "%s: %s needs %s=%s, got %d%s", who, d->name, field, want, have, note);
    };
    if (d->agents_hi) need("n_agents", d->agents_lo, d->agents_hi, cfg->n_agents, "");
    if (rc != SES_OK) return rc;                                      // (num_state may follow from n_agents)
    need("num_state", d->num_state(cfg), d->num_state(cfg), cfg->num_state, d->s_per_agent ? " (it follows from n_agents)" : "");
    need("num_action", d->A, d->A, cfg->num_action, "");
    if (d->discrete != EITHER) need("discrete_action", d->discrete, d->discrete, cfg->discrete_action != 0, "");
    need("gru", 0, d->gru_ok ? 1 : 0, cfg->gru, d->gru_ok ? "" : " (no GRU rollout is built for it)");
    need("pomdp", 0, d->pomdp_ok ? 1 : 0, cfg->pomdp != 0, " (it has no pomdp variant)");
    need("physics64", 0, d->physics64_ok ? 1 : 0, cfg->physics64,
         d->is_f64 ? " (its physics is float64 regardless)" : " (physics64 is a CartPole rollout option)");
    if (d->max_eval_ep) need("eval_ep_num", 1, d->max_eval_ep, cfg->eval_ep_num, "");
    if (rc == SES_OK) *row = d;
    return rc;
}

}  // namespace ses

extern "C" {

int ses_env_info(const ses_config *cfg, struct ses_env_info *out)
{
    using namespace ses;
    SES_REQUIRE(cfg && out, "ses_env_info: null argument");
    const EnvDesc *d;
    const int rc = env_check_config("ses_env_info", cfg, &d);
    if (rc != SES_OK) return rc;
    SES_REQUIRE(d, "ses_env_info: SES_ENV_NONE is no env");
    out->init_width = d->init_width(cfg);
    out->obs_width = d->obs_width(cfg);
    out->state_bytes = d->state_bytes(cfg);
    out->action_layout = d->action_layout(cfg);
    out->agents = d->agents(cfg);
    out->num_action = d->A;
    out->has_ep_steps = d->has_ep_steps;
    out->is_f64 = d->is_f64;
    out->init_lo = d->init_lo;
    out->init_hi = d->init_hi;
    return SES_OK;
}

int ses_env_state_bytes(ses_handle *h)
{
    using namespace ses;
    SES_REQUIRE(h, "ses_env_state_bytes: null handle");
    const EnvDesc *d = env_desc(h);
    SES_REQUIRE(d, "ses_env_state_bytes: handle has no env");
    return d->state_bytes(&h->cfg);
}

int ses_env_obs_width(ses_handle *h)
{
    using namespace ses;
    SES_REQUIRE(h, "ses_env_obs_width: null handle");
    const EnvDesc *d = env_desc(h);
    SES_REQUIRE(d, "ses_env_obs_width: handle has no env");
    return d->obs_width(&h->cfg);
}

int ses_env_reset(ses_handle *h, const float *init, int32_t n, void *state, float *obs)
{
    using namespace ses;
    SES_REQUIRE(h && init && state && obs, "ses_env_reset: null argument");
    SES_REQUIRE(n >= 1, "ses_env_reset: n must be >= 1");
    const EnvDesc *d = env_desc(h);
    SES_REQUIRE(d, "ses_env_reset: handle has no env");
    SES_REQUIRE(!h->cfg.physics64, "ses_env_reset: the step-wise CartPole is the float32 one (physics64 exists in the fused rollouts only)");
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    return d->reset(h, init, n, state, obs);
}

int ses_env_step_generic(ses_handle *h, void *state, const void *action, int32_t n, float *obs, float *reward, int32_t *done)
{
    using namespace ses;
    SES_REQUIRE(h && state && action && obs && reward && done, "ses_env_step_generic: null argument");
    SES_REQUIRE(n >= 1, "ses_env_step_generic: n must be >= 1");
    const EnvDesc *d = env_desc(h);
    SES_REQUIRE(d, "ses_env_step_generic: handle has no env");
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    return d->step(h, state, action, n, obs, reward, done);
}

}  // extern "C"
