// ses_lander_discrete.hip -- LunarLander-v2, gym's discrete four-action lander (lunar_lander.py, continuous=False):
//   0 = no-op, 1 = fire left orientation engine, 2 = fire main engine, 3 = fire right orientation engine.
// gym sets m_power = 1 for action 2 and, for 1 and 3, direction = action - 2 with s_power = 1.  Those are exactly the values
// b2l::lander_step_begin computes from the continuous inputs (a0, a1) = (0, 0), (0, -1), (1, 0), (0, +1):
// (clamp(1, 0, 1) + 1) * 0.5 = 1, clamp(|+-1|, 0.5, 1) = 1, direction = sign(a1) -- so the discrete env IS ll_step (ses_lander.h)
// called through that table; reward, termination, dispersion noise, terrain and reset are the continuous env's.
// The policy head is GymEnvModel's discrete one: argmax over the four outputs, first maximum wins, no tanh.
//
// A unit of its own: the kernels of ses_rollout.hip reach .rodata PC-relative, so a kernel added there moves the hashes its
// profiles hang on (ses_internal.h, "load-bearing").  The lockstep and MFMA GRU bodies are the shared ones of
// ses_gru_lockstep.h and ses_rollout_bodies.h under kernels of this unit; the sequential GRU rollout and the MLP rollout are
// written out here (their continuous twins k_rollout_lander_gru and k_rollout_box2d_mlp keep their bodies inside the kernels:
// see ses_rollout_bodies.h).  The plan (ses_rollout_plan.h) picks the form and the wave shape by the continuous env's rules
// and rollout_lander hands them over.  ll_step is compiled once in this unit, as a real function, like there.
#include "ses_lander.h"
#include "ses_internal.h"
#include "ses_rollout_bodies.h"

namespace ses {

// (a0, a1) of ll_step for a discrete action; anything outside 0 .. 3 is the no-op
__device__ __forceinline__ void lander_discrete_action(int action, float &a0, float &a1)
{
    a0 = action == 2 ? 1.0f : 0.0f;
    a1 = action == 1 ? -1.0f : (action == 3 ? 1.0f : 0.0f);
}

// the adapter of the lockstep / MFMA GRU bodies (as LanderLs in ses_rollout.hip; step() takes the logits)
struct LanderDiscLs {
    static constexpr int S = 8, A = 4, INIT_W = 16;
    struct State {
        LanderState st;
    };
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u, int slot)
    {
        __shared__ float terrain[4][32][LL_TERRAIN_ROW];       // one terrain row per (wave, env slot); slot < 32
        ll_reset(s.st, u, terrain[threadIdx.x >> 6][slot]);
    }
    __device__ static __forceinline__ void observe(const State &s, float (&obs)[S]) { ll_obs(s.st, obs); }
    __device__ static __forceinline__ float step(State &s, const float (&logits)[A], const TanhEntry *, bool freeze,
                                                 bool &done)
    {
        float a0, a1;
        lander_discrete_action(argmax_first<A>(logits), a0, a1);
        float r = 0.0f;
        done = true;
        if (!freeze) r = ll_step(s.st, a0, a1, done);          // a finished env is frozen (the env code has no wave votes)
        return r;
    }
};

// ---- the kernels: the launch shapes and bounds of their continuous counterparts ------------------------------------------
// GRU, one offspring / one episode per wave (k_rollout_lander_gru)
__global__ __launch_bounds__(256, 2) void k_lld_gru_seq(const float *__restrict__ theta, const float *__restrict__ init,
                                                        int init_per_offspring, int n_rows, int E, int P, int max_step,
                                                        uint32_t obs_mask, double *__restrict__ ep_return,
                                                        int32_t *__restrict__ ep_steps, int ep_parallel)
{
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ __attribute__((aligned(16))) float vecs[4][64];
    __shared__ float terrain[4][LL_TERRAIN_ROW];                  // one terrain row per wave
    stage_tanh_table(tanh_tab);
    constexpr int S = 8, A = 4;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int unit = blockIdx.x * 4 + wave, n_units = ep_parallel ? n_rows * E : n_rows;   // padding waves replay the last unit
    const bool valid = unit < n_units;
    const int u = valid ? unit : n_units - 1;
    const int row = ep_parallel ? u / E : u;
    const int ep_begin = ep_parallel ? u - row * E : 0, ep_end = ep_parallel ? ep_begin + 1 : E;
    GruSlice<S, A> net;
    net.load(theta + (size_t)row * P, lane);
    float *vec = vecs[wave];
    for (int ep = ep_begin; ep < ep_end; ++ep) {
        LanderState st;
        ll_reset(st, init + ((size_t)(init_per_offspring ? row : 0) * E + ep) * 16, terrain[wave]);
        float h = 0.0f;
        wave_lds_sync();
        if (lane < 32) vec[2 * lane + 1] = 0.0f;
        wave_lds_sync();
        double ret = 0.0;
        int steps = 0;
        bool done = false;
        while (steps < max_step) {
            if (__builtin_amdgcn_readfirstlane((int)done)) break;
            float obs[S], logits[A];
            ll_obs(st, obs);
#pragma unroll
            for (int k = 0; k < S; ++k) obs[k] = ((obs_mask >> k) & 1u) ? 0.0f : obs[k];
            net.forward(tanh_tab, obs, h, vec, lane, logits);
            float a0, a1;
            lander_discrete_action(argmax_first<A>(logits), a0, a1);
            ret += (double)ll_step(st, a0, a1, done);
            steps += 1;
        }
        if (valid && lane == 0) {
            ep_return[(size_t)row * E + ep] = ret;
            if (ep_steps) ep_steps[(size_t)row * E + ep] = steps;
        }
    }
}

// GRU lockstep, one offspring per single-wave workgroup (k_rollout_gru_lockstep<LanderLs, false, 1>)
__global__ __launch_bounds__(64, 2) void k_lld_gru_ls(const float *__restrict__ theta, const float *__restrict__ init,
                                                      int init_per_offspring, int n_rows, int E, int P, int max_step,
                                                      uint32_t obs_mask, double *__restrict__ ep_return,
                                                      int32_t *__restrict__ ep_steps)
{
    using EnvT = LanderDiscLs;
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
#define SES_LLD_CASE(NP_, ODD_)                                                                                       \
    gru_lockstep_batch<EnvT, false, NP_, ODD_>(tanh_tab, lds, net, lane, nb, rows, max_step, obs_mask, ro, so, valid)
        switch (nb) {
            case 1: SES_LLD_CASE(1, true); break;
            case 2: SES_LLD_CASE(1, false); break;
            case 3: SES_LLD_CASE(2, true); break;
            case 4: SES_LLD_CASE(2, false); break;
            case 5: SES_LLD_CASE(3, true); break;
            case 6: SES_LLD_CASE(3, false); break;
            case 7: SES_LLD_CASE(4, true); break;
            default: SES_LLD_CASE(4, false); break;
        }
#undef SES_LLD_CASE
    }
}

// GRU lockstep with G offspring per wave, four waves per workgroup (k_rollout_gru_lockstep_multi<LanderLs, G>)
template <int G>
__global__ __launch_bounds__(256, 2) void k_lld_gru_ls_multi(const float *__restrict__ theta, const float *__restrict__ init,
                                                             int init_per_offspring, int n_rows, int E, int P, int max_step,
                                                             uint32_t obs_mask, double *__restrict__ ep_return,
                                                             int32_t *__restrict__ ep_steps)
{
    using EnvT = LanderDiscLs;
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ __attribute__((aligned(16))) GruLockstepLds<EnvT::S, EnvT::A> ldsv[4][G];
    stage_tanh_table(tanh_tab);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row0 = (blockIdx.x * 4 + wave) * G;
    if (row0 >= n_rows) return;                       // (no workgroup-level synchronisation after the table staging)
#define SES_LLD_CASE(NP_, ODD_)                                                                                          \
    gru_lockstep_multi_batch<EnvT, G, NP_, ODD_>(tanh_tab, ldsv[wave], theta, P, row0, n_rows, lane, E, init,              \
                                                 init_per_offspring, E, max_step, obs_mask, ep_return, ep_steps)
    switch (E) {                                      // E <= GL_EB (the form is chosen for such E only)
        case 1: SES_LLD_CASE(1, true); break;
        case 2: SES_LLD_CASE(1, false); break;
        case 3: SES_LLD_CASE(2, true); break;
        case 4: SES_LLD_CASE(2, false); break;
        case 5: SES_LLD_CASE(3, true); break;
        case 6: SES_LLD_CASE(3, false); break;
        case 7: SES_LLD_CASE(4, true); break;
        default: SES_LLD_CASE(4, false); break;
    }
#undef SES_LLD_CASE
}

// GRU on the 16x16x4 MFMA tiles, four offspring per workgroup (k_rollout_gru_mfma<LanderLs, false>)
__global__ __launch_bounds__(256, 2) void k_lld_gru_mfma(const float *__restrict__ theta, const float *__restrict__ init,
                                                         int init_per_offspring, int n_rows, int E, int P, int max_step,
                                                         uint32_t obs_mask, double *__restrict__ ep_return,
                                                         int32_t *__restrict__ ep_steps)
{
    using EnvT = LanderDiscLs;
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ __attribute__((aligned(16))) GruMfmaLds<EnvT::S, EnvT::A> ldsv[4];
    stage_tanh_table(tanh_tab);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int row = blockIdx.x * 4 + wave;
    const bool valid = row < n_rows;
    row = valid ? row : n_rows - 1;
    GruMfmaLds<EnvT::S, EnvT::A> &lds = ldsv[wave];
    GruMfma<EnvT::S, EnvT::A> net;
    net.load(theta + (size_t)row * P, lane, lds);
    wave_lds_sync();
    for (int e0 = 0; e0 < E; e0 += GM_EB) {
        const int nb = E - e0 < GM_EB ? E - e0 : GM_EB;
        const float *rows = init + ((size_t)(init_per_offspring ? row : 0) * E + e0) * EnvT::INIT_W;
        double *ro = ep_return ? ep_return + (size_t)row * E + e0 : nullptr;
        int32_t *so = ep_steps ? ep_steps + (size_t)row * E + e0 : nullptr;
        gru_mfma_batch<EnvT, false>(tanh_tab, lds, net, lane, nb, rows, max_step, obs_mask, ro, so, valid);
    }
}

// MLP at LPE lanes per env, single-wave workgroups, two waves per SIMD (k_rollout_box2d_mlp<LanderMlpEnv, LPE>): LPE <= 8: 32 / LPE
// hidden units per lane; above: the forward on every 16-lane row of the env's lanes.  envs_per_wave <= 64 / LPE different envs
// in the wave; the lane groups past the last one shadow it (same env, same path: a wave-step costs about as much as the wave
// carries DIFFERENT envs).  The lane's weight slice is re-read from the (L2-resident) row every step, so nothing of the
// policy has to stay in registers across the 20 000-instruction world step.
template <int LPE>
__global__ __launch_bounds__(64, 2) void k_lld_mlp(const float *__restrict__ theta, const float *__restrict__ init,
                                                   int init_per_offspring, int n_rows, int E, int P, int max_step, uint32_t obs_mask,
                                                   int envs_per_wave, double *__restrict__ ep_return, int32_t *__restrict__ ep_steps)
{
    constexpr int S = 8, A = 4;
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ float terrain[64 / LPE][LL_TERRAIN_ROW];            // one terrain row per env
    stage_tanh_table(tanh_tab);
    const int n_env = n_rows * E;
    const int group = (int)threadIdx.x / LPE;
    const int slot = group < envs_per_wave ? group : envs_per_wave - 1;
    int env = (int)blockIdx.x * envs_per_wave + slot;
    const int sub = (int)(threadIdx.x % LPE);
    const bool valid = env < n_env && group < envs_per_wave;
    env = env < n_env ? env : n_env - 1;
    const int row = env / E, ep = env - row * E;
    LanderState st;
    ll_reset(st, init + ((size_t)(init_per_offspring ? row : 0) * E + ep) * 16, terrain[slot]);
    double ret = 0.0;
    int steps = 0;
    bool done = false;
    for (int t = 0; t < max_step; ++t) {
        if (__ballot(!done) == 0ull) break;
        float obs[S], logits[A];
        ll_obs(st, obs);
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
        float a0, a1;
        lander_discrete_action(argmax_first<A>(logits), a0, a1);
        if (!done) {                                               // a finished env is frozen
            ret += (double)ll_step(st, a0, a1, done);
            steps += 1;
        }
    }
    if (valid && sub == 0) {
        ep_return[env] = ret;
        if (ep_steps) ep_steps[env] = steps;
    }
}

// step-wise env: one lane per env, int32 actions (k_envs_step_lander's discrete twin; the reset kernel is shared)
__global__ __launch_bounds__(64, 2) void k_lld_env_step(LanderBlob *__restrict__ state, const int32_t *__restrict__ action, int n,
                                                        float *__restrict__ obs, float *__restrict__ reward,
                                                        int32_t *__restrict__ done, uint32_t obs_mask)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    LanderBlob &b = state[i];
    LanderState s;
    s.env = b.env;
    s.ty = b.ty;
    float a0, a1;
    lander_discrete_action(action[i], a0, a1);
    bool d;
    const float r = ll_step(s, a0, a1, d);
    b.env = s.env;
    float o[8];
    ll_obs(s, o);
    for (int k = 0; k < 8; ++k) obs[(size_t)i * 8 + k] = ((obs_mask >> k) & 1u) ? 0.0f : o[k];
    reward[i] = r;
    done[i] = d ? 1 : 0;
}

// ---- host ------------------------------------------------------------------------------------------------------------
int lander_discrete_rollout(const ses_handle *h, const RolloutArgs &a, GruForm form, int lpe, int epw)
{
    const dim3 block(256);                                              // the GRU kernels: four waves per workgroup
    if (h->cfg.gru) {
        switch (form) {
            case GruForm::EpisodeParallel:
            case GruForm::Sequential: {                                     // one wave per (offspring, episode) / per offspring
                const bool epp = form == GruForm::EpisodeParallel;
                hipLaunchKernelGGL(k_lld_gru_seq, dim3(ceil_div(epp ? a.episodes() : a.n_rows, 4)), block, 0, h->stream, a.theta,
                                   a.init, a.per, a.n_rows, a.E, a.P, a.max_step, a.obs_mask, a.epr, a.ep_steps, epp ? 1 : 0);
                break;
            }
            case GruForm::Mfma:
                launch_rollout_kernel(h, k_lld_gru_mfma, dim3(ceil_div(a.n_rows, 4)), block, a);
                break;
            case GruForm::LockstepMulti4:
                launch_rollout_kernel(h, k_lld_gru_ls_multi<4>, dim3(ceil_div(a.n_rows, 16)), block, a);
                break;
            case GruForm::LockstepMulti2:
                launch_rollout_kernel(h, k_lld_gru_ls_multi<2>, dim3(ceil_div(a.n_rows, 8)), block, a);
                break;
            case GruForm::Lockstep:
                launch_rollout_kernel(h, k_lld_gru_ls, dim3(a.n_rows), dim3(64), a);
                break;
            default:
                return set_error(SES_ERR_INVALID_ARG, "ses_rollout: LunarLander-v2 has no GRU rollout of form %d", (int)form);
        }
    } else {
        SES_REQUIRE(epw >= 1 && lpe >= 1 && epw * lpe <= 64, "ses_rollout: LunarLander-v2 wave shape %d envs x %d lanes", epw, lpe);
        const dim3 grid(ceil_div(a.episodes(), epw));
        const auto launch = [&](auto lanes) { launch_rollout_kernel(h, k_lld_mlp<lanes()>, grid, dim3(64), a, epw); };
        if (!with_lanes<64, 32, 16, 8, 4, 2, 1>(lpe, launch)) with_lanes<1>(1, launch);      // any other value: one lane per env
    }
    return SES_OK;
}

int lander_discrete_env_step(ses_handle *h, void *state, const int32_t *action, int n, float *obs, float *reward, int32_t *done)
{
    hipLaunchKernelGGL(k_lld_env_step, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, (LanderBlob *)state, action, n, obs, reward, done,
                       h->obs_mask);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

}  // namespace ses
