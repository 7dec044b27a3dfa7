// ses_obs_norm.hip -- the running observation normaliser of ARS V2 (Mania, Guy & Recht 2018, Algorithm 2) for MLP policies on the
// eight float64 control envs (include/ses.h, ses_obs_norm_bind):
//   k_rollout_f64_mlp_norm : the MLP rollout of ses_f64_envs.hip whose policy sees the normalised observation; UPDATE also
//                            accumulates the statistics of the raw observations per env
//   k_obs_norm_merge       : their reduction over the envs in a fixed order and the merge into the run's statistics
// A unit, and so a code object, of its own: kernels reach the tanh table PC-relative, so a kernel added to ses_f64_envs.hip moves
// the machine code of every kernel there (ses_internal.h, "load-bearing").  With nothing bound a handle launches what it launched
// before this unit existed.  k_rollout_f64_mlp_norm repeats the body of k_rollout_f64_mlp instead of sharing a function with it
// for the reason ses_rollout_bodies.h gives: called from its kernel the body compiles to other machine code than inside it
// (the six 2-lane instances of the trig envs moved when it was tried).  THE TWO BODIES CHANGE TOGETHER; tests/test_gpu_obs_norm.py
// holds this one to that one bit for bit (fresh state: the identity).
#include "ses_f64_envs.h"

namespace ses {

// The policy sees on[k] = fl(fl(obs[k] - shift[k]) * scale[k]) in float32, shift and scale read once before the loop.  UPDATE:
// every step that is taken adds the RAW observation that produced its action to s1[k] and its square (exact in float64: the
// same bits with or without an fma) to s2[k], in step order; lane sub == 0 leaves (steps, s1, s2) of its env in partials,
// float64[2S + 1, n_env]: row 0 the step counts (ep_steps may be null), rows 1 .. S the sums, rows S + 1 .. 2S the sums of
// squares.  Lane groups that shadow the last env write nothing.  The accumulators are 4 S registers of chains that hang off the
// step's dependence chain, not in it; physics, rewards, termination and returns are those of k_rollout_f64_mlp.
template <class Env, int LPE, bool ONE_TRIG, bool UPDATE>
__global__ __launch_bounds__(64) void k_rollout_f64_mlp_norm(const float *__restrict__ theta, const float *__restrict__ init,
                                                             int init_per_offspring, int n_rows, int E, int P, int max_step,
                                                             double *__restrict__ ep_return, int32_t *__restrict__ ep_steps,
                                                             const float *__restrict__ affine, double *__restrict__ partials)
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
    float shift[S], scale[S];
    [[maybe_unused]] double s1[S], s2[S];
#pragma unroll
    for (int k = 0; k < S; ++k) {
        shift[k] = affine[k];
        scale[k] = affine[S + k];
        s1[k] = s2[k] = 0.0;
    }
    double ret = 0.0;
    int steps = 0;
    bool done = false;
    for (int t = 0; t < max_step; ++t) {
        if constexpr (Env::TERMINATES) {
            if (__ballot(!done) == 0ull) break;
        }
        float obs[S], on[S], logits[A];
        if constexpr (ONE_TRIG) {
            if constexpr (!Env::TRIG_ON_EXIT) Env::trig(st, tg);
            Env::observe_from(st, tg, obs);
        } else {
            Env::observe(st, obs);
        }
        if constexpr (UPDATE) {
            if (!Env::TERMINATES || !done) {                        // (the step below is taken: its observation counts)
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    const double o = (double)obs[k];
                    s1[k] += o;
                    s2[k] += o * o;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < S; ++k) on[k] = __fmul_rn(__fsub_rn(obs[k], shift[k]), scale[k]);
        if constexpr (LPE >= 4) net.forward(tanh_tab, on, logits);
        else mlp_forward_streamed<S, A, LPE>(th, sub, tanh_tab, on, logits);
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
        if constexpr (UPDATE) {
            partials[env] = (double)steps;
#pragma unroll
            for (int k = 0; k < S; ++k) {
                partials[(size_t)(1 + k) * n_env + env] = s1[k];
                partials[(size_t)(1 + S + k) * n_env + env] = s2[k];
            }
        }
    }
}

// Reduction over envs and merge, one workgroup per observation component k.  No floating-point atomics, and an order that is a
// function of n_env alone: lane l of 256 adds the partials of envs l, l + 256, ... ascending from +0.0, then a halving tree
// x[l] = x[l] + x[l + s], s = 128 ... 1 (the step counts go the same way: integers, exact in any order).  Thread 0 merges the
// batch (n_b, S1, S2) into stats[k] = (n, mean, M2), every float64 operation rounded once, and writes shift[k], scale[k];
// n_b == 0 writes nothing.  A component whose std is below 1e-7 gets scale 0 (ARS's std = inf).
// One launch of S <= 9 workgroups: each lane reads 3 ceil(n_env / 256) consecutive-across-lanes doubles, then eight barriers.
__global__ __launch_bounds__(256) void k_obs_norm_merge(const double *__restrict__ partials, int n_env, int S, double *__restrict__ stats,
                                                        float *__restrict__ affine)
{
    __shared__ double red[3][256];
    const int k = blockIdx.x, l = threadIdx.x;
    const double *rows[3] = {partials, partials + (size_t)(1 + k) * n_env, partials + (size_t)(1 + S + k) * n_env};
    double acc[3] = {0.0, 0.0, 0.0};
    for (int e = l; e < n_env; e += 256) {
#pragma unroll
        for (int r = 0; r < 3; ++r) acc[r] = __dadd_rn(acc[r], rows[r][e]);
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) red[r][l] = acc[r];
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (l < s) {
#pragma unroll
            for (int r = 0; r < 3; ++r) red[r][l] = __dadd_rn(red[r][l], red[r][l + s]);
        }
        __syncthreads();
    }
    if (l != 0) return;
    const double nb = red[0][0], S1 = red[1][0], S2 = red[2][0];
    if (nb == 0.0) return;
    const double n = stats[3 * k], mean = stats[3 * k + 1], M2 = stats[3 * k + 2];
    const double mb = __ddiv_rn(S1, nb);
    const double M2b = fmax(__dsub_rn(S2, __dmul_rn(S1, mb)), 0.0);
    const double N = __dadd_rn(n, nb);
    const double f = __ddiv_rn(nb, N);
    const double d = __dsub_rn(mb, mean);
    const double mean_new = __dadd_rn(mean, __dmul_rn(d, f));
    const double M2_new = __dadd_rn(__dadd_rn(M2, M2b), __dmul_rn(__dmul_rn(d, d), __dmul_rn(n, f)));
    stats[3 * k] = N;
    stats[3 * k + 1] = mean_new;
    stats[3 * k + 2] = M2_new;
    const double sd = N >= 2.0 ? __dsqrt_rn(__ddiv_rn(M2_new, __dsub_rn(N, 1.0))) : 1.0;
    affine[k] = (float)mean_new;
    affine[S + k] = sd < 1e-7 ? 0.0f : (float)__ddiv_rn(1.0, sd);
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// The MLP rollout of f64_rollout with a normaliser bound to the handle: the same lanes per env and step form;
// a.norm_partials (null: update off) picks the accumulating kernel.
int f64_rollout_norm(const ses_handle *h, const RolloutArgs &a)
{
    return with_f64_env(h->cfg.env_id, [&](auto env) -> int {
        using Env = decltype(env);
        const int lpe = f64_lanes_per_env(h, a.episodes());
        const bool update = a.norm_partials != nullptr;
        const bool known = with_lanes<1, 2, 4, 8, 16, 32>(lpe, [&](auto lanes) {
            auto kernel = update ? k_rollout_f64_mlp_norm<Env, lanes(), false, true> : k_rollout_f64_mlp_norm<Env, lanes(), false, false>;
            if constexpr (Env::HAS_TRIG) {
                if (!f64_generic_form(h))
                    kernel = update ? k_rollout_f64_mlp_norm<Env, lanes(), true, true> : k_rollout_f64_mlp_norm<Env, lanes(), true, false>;
            }
            hipLaunchKernelGGL(kernel, dim3(ceil_div(a.episodes() * lpe, 64)), dim3(64), 0, h->stream, a.theta, a.init, a.per, a.n_rows,
                               a.E, a.P, a.max_step, a.epr, a.ep_steps, a.norm_affine, a.norm_partials);
        });
        if (!known)
            return set_error(SES_ERR_INVALID_ARG, "ses_rollout: %s has no MLP rollout at %d lanes per env (1, 2, 4, 8, 16, 32)", Env::NAME,
                             lpe);
        SES_HIP_TRY(hipGetLastError());
        return SES_OK;
    });
}

// the reduction and merge of partials[2S + 1, n_env] into (stats, affine)
int f64_obs_norm_merge(const ses_handle *h, const double *partials, int n_env, double *stats, float *affine)
{
    const int S = h->cfg.num_state;                                 // (ses_create holds a float64 env to its observation width)
    hipLaunchKernelGGL(k_obs_norm_merge, dim3(S), dim3(256), 0, h->stream, partials, n_env, S, stats, affine);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

}  // namespace ses

extern "C" {

int ses_obs_norm_bind(ses_handle *h, double *stats, float *affine, int32_t update)
{
    using namespace ses;
    SES_REQUIRE(h, "ses_obs_norm_bind: null handle");
    if (!stats) {                                                   // unbind
        h->obs_norm_stats = nullptr;
        h->obs_norm_affine = nullptr;
        h->obs_norm_update = 0;
        return SES_OK;
    }
    SES_REQUIRE(affine, "ses_obs_norm_bind: stats without affine");
    SES_REQUIRE(update == 0 || update == 1, "ses_obs_norm_bind: update must be 0 or 1, got %d", update);
    if (!is_f64_env(h))
        return set_error(SES_ERR_UNSUPPORTED,
                         "ses_obs_norm_bind: the observation normaliser serves the eight float64 envs (Acrobot, MountainCar, Pendulum, "
                         "MountainCarContinuous, the inverted pendulums, the Reacher); env_id %d is not one of them",
                         h->cfg.env_id);
    if (h->cfg.gru)
        return set_error(SES_ERR_UNSUPPORTED, "ses_obs_norm_bind: a GRU policy runs the lockstep kernel shared with every other env, "
                                              "which has no normalising form (MLP policies only)");
    if (h->comm && h->comm_world > 1)
        return set_error(SES_ERR_UNSUPPORTED, "ses_obs_norm_bind: the handle has a communicator of world %d; one GPU only: the "
                                              "statistics would need an exchange",
                         h->comm_world);
    h->obs_norm_stats = stats;
    h->obs_norm_affine = affine;
    h->obs_norm_update = update;
    return SES_OK;
}

int ses_obs_norm_merge(ses_handle *h, const double *partials, int32_t n_env, double *stats, float *affine)
{
    using namespace ses;
    SES_REQUIRE(h && partials && stats && affine, "ses_obs_norm_merge: null argument");
    SES_REQUIRE(n_env >= 1, "ses_obs_norm_merge: n_env must be >= 1");
    if (!is_f64_env(h))
        return set_error(SES_ERR_UNSUPPORTED, "ses_obs_norm_merge: the observation normaliser serves the eight float64 envs; env_id %d "
                                              "is not one of them",
                         h->cfg.env_id);
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    return f64_obs_norm_merge(h, partials, n_env, stats, affine);
}

}  // extern "C"
