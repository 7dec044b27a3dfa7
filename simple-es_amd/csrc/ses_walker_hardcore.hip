// ses_walker_hardcore.hip -- BipedalWalkerHardcore-v3: BipedalWalker-v3's body, observation, actions and reward on a terrain with
// stumps, pits and stairs (ses_walker_hardcore_env.h, DESIGN.md 7: the build's own definition, parity with gym unpinned), on the
// Box2D-style world of ses_b2.h with eight manifold slots per leg instead of four.
//   k_bwh_mlp<LPE>             : fused rollout, MLP policy, LPE lanes per env (the shape of k_rollout_box2d_mlp / k_w2d_mlp)
//   k_bwh_gru_ls               : fused rollout, GRU policy, the shared lockstep body of ses_gru_lockstep.h
//   k_bwh_env_reset / _step    : the step-wise env, one lane per env, state blob = HardcoreBlob (the env struct, then the terrain row)
//   k_policy_forward_gru<24, 4>: ses_policy_forward for this env's GRU shape (the MLP instance is ses_rollout.hip's)
//
// A unit of its own for the reason ses_walker2d.hip gives: a kernel added to an existing unit moves that unit's machine code.
// The env step is compiled once in this unit as two real functions, bwh_step and bwh_step_end, as bw_step / bw_step_end are
// (ses_walker.h).
//
// LDS.  An env's terrain is one row of BWH_ROW floats = 2192 bytes (two heights per column, 199 x 8; the riser count per column,
// 200 bytes; the column of each edge, 400 bytes: ses_walker_hardcore_env.h), 2.74 x BipedalWalker-v3's 800.  k_bwh_mlp<LPE> holds
// 64 / LPE rows next to the 5120-byte tanh table:
//      LPE   64     32     16     8      4       2       1
//      KiB   7.1    9.3    13.6   22.1   39.25   73.5    142.0
// One wave per SIMD means four single-wave workgroups in a CU's 160 KiB, 40 KiB each: LPE >= 4.  The plan therefore never puts
// more than WALKER_HARDCORE_MAX_EPW = 16 envs into a wave (ses_rollout_plan.h); 2 and 1 lanes per env exist for ses_set_tuning's
// forced shapes only and run one or two workgroups per CU.  k_bwh_gru_ls: 8 rows (17.1 KiB) + the lockstep block + the table.
#include "ses_lander.h"          // the B2_* macros of the device build
namespace ses {
constexpr uint64_t TAG_ENV_TERRAIN_BWH = 3ull;       // ses_walker.h's TAG_ENV_TERRAIN: the stream BipedalWalker-v3 draws its terrain from
}
// uniform in (-1, 1) and two raw words for terrain column i (host: tests/walker_hardcore_host.cpp)
#define B2_TERRAIN_RAND3(k0, k1, i, u, r, q)                                                                           \
    do {                                                                                                               \
        const uint4 w_ = ses::philox_words(((uint64_t)(k1) << 32) | (uint64_t)(k0), ses::TAG_ENV_TERRAIN_BWH, 0ull, 0u, \
                                           (uint32_t)(i));                                                             \
        u = ses::fma_(ses::u32_to_unit(w_.x), 2.0f, -1.0f);                                                            \
        r = w_.y;                                                                                                      \
        q = w_.z;                                                                                                      \
    } while (0)
#define B2_TERRAIN_RAND(k0, k1, i, u, r)                                                                               \
    do {                                                                                                               \
        uint32_t q_;                                                                                                   \
        B2_TERRAIN_RAND3(k0, k1, i, u, r, q_);                                                                         \
        (void)q_;                                                                                                      \
    } while (0)
#include "ses_walker_hardcore_env.h"
#include "ses_env_table.h"
#include "ses_gru_lockstep.h"
#include "ses_internal.h"
#include "ses_policy.h"
#include "ses_policy_forward.h"

namespace ses {

constexpr int BWH_ROW = b2l::BWH_ROW;

struct HardcoreState {
    b2l::WalkerHardcoreEnv env;
    const float *row;                        // LDS (rollouts) or the state blob (step-wise env): this env's terrain row
    b2l::WalkerPending pend;                 // between the two halves of a step
};

// the step-wise env's state blob
struct HardcoreBlob {
    b2l::WalkerHardcoreEnv env;
    float row[BWH_ROW];
};

__device__ __forceinline__ void bwh_obs(const HardcoreState &s, float (&obs)[24]) { b2l::walker_obs(s.env, obs); }

// one env step as two real functions, like bw_step / bw_step_end: state in the caller's private memory, no wave votes inside: the
// call may sit under any divergence (finished envs do not call)
__device__ __attribute__((noinline)) float bwh_step_end(HardcoreState &s, bool &done)
{
    const b2l::HardcoreTerrain terr{s.row};
    bool d;
    const float r = b2l::walker_step_end(s.env, terr, s.pend, d);
    done = d;
    return r;
}

__device__ __attribute__((noinline)) float bwh_step(HardcoreState &s, float a0, float a1, float a2, float a3, bool &done)
{
    {
        b2l::WalkerHardcoreEnv e = s.env;
        asm volatile("" ::: "memory");
        const b2l::HardcoreTerrain terr{s.row};
        const float act[4] = {a0, a1, a2, a3};
        b2l::WalkerPending pd;
        b2l::walker_step_begin(e, terr, act, pd);
        s.env = e;
        s.pend = pd;
    }
    return bwh_step_end(s, done);
}

// reset from one row of 4 floats ([0] force uniform, [1], [2] terrain key bit patterns); ends with one no-op step.  row: BWH_ROW
// floats owned by this env (every lane of the env writes identical values); all lanes of the wave call this together; the wave
// fences are bw_reset's.
__device__ __forceinline__ void bwh_reset(HardcoreState &s, const float *__restrict__ u, float *row)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    b2l::hardcore_terrain_generate(f2u(u[1]), f2u(u[2]), row, nullptr);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    s.row = row;
    b2l::walker_reset_state(s.env, u);
    bool done;
    (void)bwh_step(s, 0.0f, 0.0f, 0.0f, 0.0f, done);
}

// the adapter of the lockstep GRU body (as LanderLs in ses_rollout.hip): single-wave workgroups, one terrain row per env slot
struct HardcoreLs {
    static constexpr int S = 24, A = 4, INIT_W = 4;
    struct State {
        HardcoreState st;
    };
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u, int slot)
    {
        __shared__ float terrain[GL_EB][BWH_ROW];
        bwh_reset(s.st, u, terrain[slot]);
    }
    __device__ static __forceinline__ void observe(const State &s, float (&obs)[S]) { bwh_obs(s.st, obs); }
    __device__ static __forceinline__ float step(State &s, const float (&logits)[A], const TanhEntry *tab, bool freeze, bool &done)
    {
        float act[A];
#pragma unroll
        for (int k = 0; k < A; ++k) act[k] = tanh_(tab, logits[k]);
        float r = 0.0f;
        done = true;
        if (!freeze) r = bwh_step(s.st, act[0], act[1], act[2], act[3], done);      // a finished env is frozen
        return r;
    }
};

// MLP at LPE lanes per env, single-wave workgroups (k_rollout_box2d_mlp's shape): LPE <= 8: 32 / LPE hidden units per lane; above:
// the forward on every 16-lane row of the env's lanes.  envs_per_wave <= 64 / LPE different envs in the wave; the lane groups past
// the last one shadow it (same env, same path, same terrain row).  The lane's weight slice is re-read from the (L2-resident) row
// every step, so nothing of the policy has to stay in registers across the world step.
template <int LPE>
__global__ __launch_bounds__(64, WALKER_HARDCORE_MLP_WAVES_PER_SIMD) void k_bwh_mlp(const float *__restrict__ theta, const float *__restrict__ init,
                                                                                  int init_per_offspring, int n_rows, int E, int P, int max_step,
                                                                                  uint32_t obs_mask, int envs_per_wave,
                                                                                  double *__restrict__ ep_return, int32_t *__restrict__ ep_steps)
{
    constexpr int S = 24, A = 4;
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ float terrain[64 / LPE][BWH_ROW];                  // one terrain row per env
    stage_tanh_table(tanh_tab);
    const int n_env = n_rows * E;
    const int group = (int)threadIdx.x / LPE;
    const int slot = group < envs_per_wave ? group : envs_per_wave - 1;
    int env = (int)blockIdx.x * envs_per_wave + slot;
    const int sub = (int)(threadIdx.x % LPE);
    const bool valid = env < n_env && group < envs_per_wave;
    env = env < n_env ? env : n_env - 1;
    const int row = env / E, ep = env - row * E;
    HardcoreState st;
    bwh_reset(st, init + ((size_t)(init_per_offspring ? row : 0) * E + ep) * 4, terrain[slot]);
    double ret = 0.0;
    int steps = 0;
    bool done = false;
    for (int t = 0; t < max_step; ++t) {
        if (__ballot(!done) == 0ull) break;
        float obs[S], logits[A], act[A];
        bwh_obs(st, obs);
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
#pragma unroll
        for (int k = 0; k < A; ++k) act[k] = tanh_(tanh_tab, logits[k]);
        if (!done) {                                               // a finished env is frozen
            ret += (double)bwh_step(st, act[0], act[1], act[2], act[3], done);
            steps += 1;
        }
    }
    if (valid && sub == 0) {
        ep_return[env] = ret;
        if (ep_steps) ep_steps[env] = steps;
    }
}

// GRU lockstep, one offspring per single-wave workgroup (k_w2d_gru_ls's shape): a wave lives as long as the longest of its
// episodes and frees its SIMD slot for the next offspring when they are over
__global__ __launch_bounds__(64, WALKER_HARDCORE_MLP_WAVES_PER_SIMD) void k_bwh_gru_ls(const float *__restrict__ theta, const float *__restrict__ init,
                                                                                     int init_per_offspring, int n_rows, int E, int P, int max_step,
                                                                                     uint32_t obs_mask, double *__restrict__ ep_return,
                                                                                     int32_t *__restrict__ ep_steps)
{
    using EnvT = HardcoreLs;
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
#define SES_BWH_CASE(NP_, ODD_)                                                                                       \
    gru_lockstep_batch<EnvT, false, NP_, ODD_>(tanh_tab, lds, net, lane, nb, rows, max_step, obs_mask, ro, so, valid)
        switch (nb) {
            case 1: SES_BWH_CASE(1, true); break;
            case 2: SES_BWH_CASE(1, false); break;
            case 3: SES_BWH_CASE(2, true); break;
            case 4: SES_BWH_CASE(2, false); break;
            case 5: SES_BWH_CASE(3, true); break;
            case 6: SES_BWH_CASE(3, false); break;
            case 7: SES_BWH_CASE(4, true); break;
            default: SES_BWH_CASE(4, false); break;
        }
#undef SES_BWH_CASE
    }
}

// ---- the step-wise env: one lane per env; the terrain row is the blob's own -----------------------------------------------------
__global__ __launch_bounds__(64, WALKER_HARDCORE_MLP_WAVES_PER_SIMD) void k_bwh_env_reset(const float *__restrict__ init, int n,
                                                                                        HardcoreBlob *__restrict__ state, float *__restrict__ obs)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    HardcoreBlob &b = state[i];
    HardcoreState s;
    bwh_reset(s, init + (size_t)i * 4, b.row);
    b.env = s.env;
    float o[24];
    bwh_obs(s, o);
    for (int k = 0; k < 24; ++k) obs[(size_t)i * 24 + k] = o[k];
}

__global__ __launch_bounds__(64, WALKER_HARDCORE_MLP_WAVES_PER_SIMD) void k_bwh_env_step(HardcoreBlob *__restrict__ state, const float *__restrict__ action,
                                                                                       int n, float *__restrict__ obs, float *__restrict__ reward,
                                                                                       int32_t *__restrict__ done)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    HardcoreBlob &b = state[i];
    HardcoreState s;
    s.env = b.env;
    s.row = b.row;
    const float *a = action + (size_t)i * 4;
    bool d;
    const float r = bwh_step(s, a[0], a[1], a[2], a[3], d);
    b.env = s.env;
    float o[24];
    bwh_obs(s, o);
    for (int k = 0; k < 24; ++k) obs[(size_t)i * 24 + k] = o[k];
    reward[i] = r;
    done[i] = d ? 1 : 0;
}

// ---- host: the table row's entry functions (ses_env_table.h) -----------------------------------------------------------------
int walker_hardcore_env_state_bytes(const ses_config *) { return (int)sizeof(HardcoreBlob); }

int walker_hardcore_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs)
{
    hipLaunchKernelGGL(k_bwh_env_reset, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, init, n, (HardcoreBlob *)state, obs);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int walker_hardcore_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done)
{
    hipLaunchKernelGGL(k_bwh_env_step, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, (HardcoreBlob *)state, (const float *)action, n, obs,
                       reward, done);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int walker_hardcore_rollout(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode)
{
    SES_REQUIRE(mode == SES_MODE_EPISODIC, "ses_rollout: BipedalWalkerHardcore-v3 has no fixed-length mode");
    if (h->cfg.gru) {
        launch_rollout_kernel(h, k_bwh_gru_ls, dim3(a.n_rows), dim3(64), a);
        return SES_OK;
    }
    const int lpe = plan.box2d_lpe, epw = plan.box2d_epw;
    SES_REQUIRE(epw >= 1 && lpe >= 1 && epw * lpe <= 64, "ses_rollout: BipedalWalkerHardcore-v3 wave shape %d envs x %d lanes", epw, lpe);
    const dim3 grid(ceil_div(a.episodes(), epw));
    const auto launch = [&](auto lanes) { launch_rollout_kernel(h, k_bwh_mlp<lanes()>, grid, dim3(64), a, epw); };
    if (!with_lanes<64, 32, 16, 8, 4, 2, 1>(lpe, launch)) with_lanes<1>(1, launch);      // any other value: one lane per env
    return SES_OK;
}

// ses_policy_forward for a GRU policy of (num_state, num_action) = (24, 4); the caller has checked the shape
int walker_hardcore_policy_forward(ses_handle *h, const float *theta, const float *obs, float *hidden, int n, float *logits, float *act,
                                   int32_t *action)
{
    hipLaunchKernelGGL((k_policy_forward_gru<24, 4>), dim3(ceil_div(n, 4)), dim3(256), 0, h->stream, theta, obs, hidden, n, h->P, logits, act,
                       action);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

}  // namespace ses
