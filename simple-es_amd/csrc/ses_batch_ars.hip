// ses_batch_ars.hip -- the ars tail of R independent trials in one set of launches (ses_ars_generation_batch).
// The trials of a sweep sit one behind the other at a fixed stride, like the sep_cma_es batch (ses_batch_sepcma.hip): with n = 2 m
// rows per trial, trial r owns rows [r n, (r + 1) n) of the fitness vector and of the next population, pairs [r m, (r + 1) m) of the
// scores and the rank vector, and row r of mu [R, P].  Only the selection is ragged: b_r = elite_num_r sets the length of a trial's
// selected list and the number of 1024-pair chunks of its gradient.  Per trial, bit for bit what ses_ars_generation gives for its
// slice alone -- the orders are those of ses_ars.hip's header, pairs and rows counted from the trial's first:
//
//   scores      k_ars_scores of ses_ars.hip, launched as it is over the R m pairs
//   rank        the counting rank of ses_batch.hip (k_batch_rank_count, launched as it is with n := m): key = (ordered score bits,
//               index WITHIN the trial), -0 as +0
//   gradient    chunks of BARS_CHUNK = 1024 SELECTED pairs in rank order; thread c of 256 takes k = c, c + 256, c + 512, c + 768 (an
//               fma chain from 0), the 8-level LDS tree, one partial per chunk.  A workgroup whose chunk the trial does not have
//               returns without writing
//   sigma_R     the last workgroup of each trial, in double: the selected list, the two passes, {sigma_R, step}, best[r]
//   update      exactly the trial's own ceil(b_r / 1024) chunk partials in ascending order (never a zero partial of a chunk it does
//               not have: +0.0 would turn a -0 sum into +0), mu' = fl(mu + fl(step * G))
//   population  one Philox call per thread for 4 parameters of both rows of a pair, row = pair index within the trial,
//               d = fl(next_sigma * z), mu' +- d, no fma
//
// Four launches whatever R -- five where ses_ars_generation takes five (P > 1024, or the knob "ars_fused_apply_perturb" = 0) -- the
// trial a grid dimension of each; no launch needs an order between its workgroups: no ticket counters, no polling.  The
// per-generation records are read from a table in DEVICE memory the caller wrote: no host-to-device copy here.  The library never
// sees that table, so what a kernel derives from it is held inside the trial's slice first: b_r is clamped into [1, m], the chunk
// count into the chunks the grid has, every entry read from a selected list into the trial's m pairs (ars_pair's clamp).  A wrong
// table or a fitness vector with NaNs gives wrong numbers, never an access outside the caller's buffers.
#include "ses_internal.h"
#include "ses_rng.h"
#include "ses_tail.h"

namespace ses {

constexpr int BARS_CHUNK = 1024;              // selected pairs per gradient workgroup (ARS_CHUNK)
constexpr int BARS_FOLD_MAX_P = 1024;         // the update inside the population launch: up to this many parameters (ARS_FOLD_MAX_P)
constexpr int BARS_MAX_N = 2 * RANK_SORT_MIN; // rows per trial: the m = n / 2 scores are ranked by counting only
constexpr long long BARS_MAX_ROWS = 1ll << 20;

// what the sigma_R workgroup of a trial leaves for its update (ArsStat)
struct BarsStat {
    double sigma_r;
    float step;
    float pad;
};

// what the launches are given besides the fitness: the table, the shape, the scratch, the state
struct BarsShape {
    const ses_batch_ars_trial *trials;        // [R], device
    int R, m, chunks_max, P, P4, quads;
    float *partial;                           // scratch [R][chunks_max][P4]: the chunk partials of G
    BarsStat *stat;                           // scratch [R]
    int32_t *sel;                             // scratch [R][m]: sel[k] = the pair of rank k, k < b_r
    const float *mu;                          // [R, P]
    float *mu_out, *g_out;                    // [R, P]; g_out optional
    double *sigma_r_out;                      // [R], optional
    float *theta;                             // [R n, P]
    unsigned long long *stamp;
    int32_t *rank_to_clear;
    int n_clear;
};

__device__ __forceinline__ int bars_pair(int j, int m) { return j < 0 ? 0 : j >= m ? m - 1 : j; }
__device__ __forceinline__ int bars_b(int b, int m) { return b < 1 ? 1 : b > m ? m : b; }
// the chunk partials a trial has: ceil(b / 1024), held to what the grid computed
__device__ __forceinline__ int bars_chunks(int b, int chunks_max)
{
    const int c = (b + BARS_CHUNK - 1) / BARS_CHUNK;
    return c > chunks_max ? chunks_max : c;
}

__device__ __forceinline__ double bars_tree(double (&x)[256], double mine)
{
    __syncthreads();                                                     // (x may still be read from the previous tree)
    x[threadIdx.x] = mine;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) x[threadIdx.x] = __dadd_rn(x[threadIdx.x], x[threadIdx.x + s]);
        __syncthreads();
    }
    return x[0];
}

// ars_sigma_r per trial: one workgroup; rank, fitness, scores, sel are the trial's own slices
__device__ void bars_sigma_r(const int32_t *__restrict__ rank, const float *__restrict__ fitness, const float *__restrict__ scores,
                             int m, int b, double learning_rate, int32_t *sel, BarsStat *stat, float *best)
{
    __shared__ double x[256];
    for (int j = threadIdx.x; j < m; j += 256) {
        const int r = rank[j];
        if (r >= 0 && r < b) sel[r] = j;                                 // rank is a permutation of 0 .. m - 1: every entry written once
        if (r == 0 && best) *best = scores[j];                           // max(fitness of the trial)
    }
    __threadfence();
    __syncthreads();
    const long long count = 2ll * b;
    double acc = 0.0;
    for (long long e = threadIdx.x; e < count; e += 256)
        acc = __dadd_rn(acc, (double)fitness[2ll * bars_pair(sel[e >> 1], m) + (e & 1)]);
    const double mean = bars_tree(x, acc) / (double)count;
    acc = 0.0;
    for (long long e = threadIdx.x; e < count; e += 256) {
        const double dv = __dsub_rn((double)fitness[2ll * bars_pair(sel[e >> 1], m) + (e & 1)], mean);
        acc = __dadd_rn(acc, __dmul_rn(dv, dv));
    }
    const double var = bars_tree(x, acc) / (double)count;
    if (threadIdx.x == 0) {
        const double sr = __dsqrt_rn(var);
        stat->sigma_r = sr;
        stat->step = sr > 0.0 ? (float)(learning_rate / ((double)b * sr)) : 0.0f;
        stat->pad = 0.0f;
    }
}

// k_ars_grad_partial per trial: grid (R, quads * chunks_max + 1).  Workgroup w < quads * chunks_max of trial r: parameter quad
// q = w % quads, chunk = w / quads of the trial's selected list -- it returns at once where the trial has no such chunk.  Workgroup
// quads * chunks_max: the trial's sigma_R (above).
__global__ __launch_bounds__(256) void k_bars_grad_partial(BarsShape s, const int32_t *__restrict__ rank_all,
                                                           const float *__restrict__ fit_all, const float *__restrict__ scores_all,
                                                           float *__restrict__ best)
{
    const int r = blockIdx.x, w = blockIdx.y, m = s.m;
    const ses_batch_ars_trial tr = s.trials[r];                          // uniform
    const int b = bars_b(tr.b, m);
    const int32_t *__restrict__ rank = rank_all + (size_t)r * m;
    const float *__restrict__ fitness = fit_all + (size_t)r * 2 * m;
    if (w == s.quads * s.chunks_max) {                                   // workgroup-uniform
        bars_sigma_r(rank, fitness, scores_all + (size_t)r * m, m, b, tr.learning_rate, s.sel + (size_t)r * m, s.stat + r,
                     best ? best + r : nullptr);
        return;
    }
    __shared__ int32_t sel[BARS_CHUNK];
    __shared__ float red[4][256];
    const int q = w % s.quads, chunk = w / s.quads;
    const int k0 = chunk * BARS_CHUNK;
    if (k0 >= b) return;                                                 // workgroup-uniform: not one of this trial's chunks
    const int cnt = b - k0 < BARS_CHUNK ? b - k0 : BARS_CHUNK;
    for (int j = threadIdx.x; j < m; j += 256) {
        const int rk = rank[j] - k0;
        if (rk >= 0 && rk < cnt) sel[rk] = j;
    }
    __syncthreads();
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = threadIdx.x; k < cnt; k += 256) {
        const int j = bars_pair(sel[k], m);
        const float d = (float)((double)fitness[2 * j] - (double)fitness[2 * j + 1]);
        float z[4];
        normal4(tr.seed, tr.gen, (uint32_t)j, (uint32_t)q, z);
#pragma unroll
        for (int l = 0; l < 4; ++l) acc[l] = fma_(d, z[l], acc[l]);
    }
#pragma unroll
    for (int l = 0; l < 4; ++l) red[l][threadIdx.x] = acc[l];
    __syncthreads();
    for (int t = 128; t > 0; t >>= 1) {
        if (threadIdx.x < t) {
#pragma unroll
            for (int l = 0; l < 4; ++l) red[l][threadIdx.x] = red[l][threadIdx.x] + red[l][threadIdx.x + t];
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) s.partial[((size_t)r * s.chunks_max + chunk) * s.P4 + 4 * q + threadIdx.x] = red[threadIdx.x][0];
}

// ars_update_param per trial: G[p] = the trial's `chunks` chunk partials in ascending order; mu'[p] = fl(mu[p] + fl(step * G[p])).
// store: mu_out and the optional G are written.
__device__ __forceinline__ float bars_update_param(const BarsShape &s, int r, int chunks, int p, float step, bool store)
{
    const float *__restrict__ partial = s.partial + (size_t)r * s.chunks_max * s.P4;
    float g = partial[p];
    for (int c = 1; c < chunks; ++c) g = g + partial[(size_t)c * s.P4 + p];
    const size_t at = (size_t)r * s.P + p;
    const float mu_new = __fadd_rn(s.mu[at], __fmul_rn(step, g));
    if (store) {
        if (s.g_out) s.g_out[at] = g;
        s.mu_out[at] = mu_new;
    }
    return mu_new;
}

// k_ars_apply per trial: grid (R, ceil(P / 256)), a thread per parameter (policies above BARS_FOLD_MAX_P parameters, or the knob
// "ars_fused_apply_perturb" = 0)
__global__ __launch_bounds__(256) void k_bars_apply(BarsShape s)
{
    const int r = blockIdx.x, p = blockIdx.y * 256 + threadIdx.x;
    const BarsStat st = s.stat[r];
    if (p == 0 && s.sigma_r_out) s.sigma_r_out[r] = st.sigma_r;
    if (p >= s.P) return;
    bars_update_param(s, r, bars_chunks(bars_b(s.trials[r].b, s.m), s.chunks_max), p, st.step, true);
}

// k_ars_perturb per trial: `bpt` workgroups per trial, workgroup blockIdx.x serves trial blockIdx.x / bpt; a thread per (pair of the
// trial, quad): one Philox call, 4 consecutive parameters of both rows of the pair, one rounding per operation.  FUSED: EVERY
// workgroup first forms its trial's whole new mean itself into LDS (the trial's first workgroup also stores it) -- the same sums in
// the same order as k_bars_apply, so the two forms are bit-equal.  Not FUSED: the mean is read from mu_out, which k_bars_apply wrote
// on the same stream.  Either way the launch stamps the tail time and zeroes the rank vectors for the next generation's count.
template <bool FUSED>
__global__ __launch_bounds__(256) void k_bars_perturb(BarsShape s, int bpt)
{
    __shared__ float mu_new[FUSED ? BARS_FOLD_MAX_P : 1];
    const int r = blockIdx.x / bpt, blk = blockIdx.x - r * bpt;
    const long long t_all = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s.stamp && t_all == 0) *s.stamp = real_time();                   // ses_set_stamp: the next population is being written
    const ses_batch_ars_trial tr = s.trials[r];                          // uniform
    if (FUSED) {
        const BarsStat st = s.stat[r];
        if (blk == 0 && threadIdx.x == 0 && s.sigma_r_out) s.sigma_r_out[r] = st.sigma_r;
        const int chunks = bars_chunks(bars_b(tr.b, s.m), s.chunks_max);
        for (int p = threadIdx.x; p < s.P; p += 256) mu_new[p] = bars_update_param(s, r, chunks, p, st.step, blk == 0);
    }
    for (long long i = t_all; i < s.n_clear; i += (long long)gridDim.x * 256) s.rank_to_clear[i] = 0;
    if (FUSED) __syncthreads();
    const long long t = (long long)blk * 256 + threadIdx.x;              // within the trial
    if (t >= (long long)s.m * s.quads) return;
    const int j = (int)(t / s.quads);
    const int q = (int)(t - (long long)j * s.quads);
    const int lim = s.P - 4 * q < 4 ? s.P - 4 * q : 4;
    float z[4];
    normal4(tr.seed, tr.next_gen, (uint32_t)j, (uint32_t)q, z);
    const float *__restrict__ center = s.mu_out + (size_t)r * s.P + 4 * q;
    float *dst_even = s.theta + ((size_t)r * 2 * s.m + 2 * (size_t)j) * s.P + 4 * q;
    float *dst_odd = dst_even + s.P;
    for (int l = 0; l < lim; ++l) {
        const float c = FUSED ? mu_new[4 * q + l] : center[l];
        const float d = __fmul_rn(tr.next_sigma, z[l]);
        dst_even[l] = __fadd_rn(c, d);
        dst_odd[l] = __fsub_rn(c, d);
    }
}

static size_t bars_round256(size_t bytes) { return (bytes + 255) / 256 * 256; }

}  // namespace ses

extern "C" {

using namespace ses;

int ses_ars_generation_batch(ses_handle *h, const float *fitness, int32_t R, int32_t n, const int32_t *b,
                             const ses_batch_ars_trial *trials, const float *mu_in, float *mu_out, float *theta_next, float *best,
                             float *g_out, double *sigma_r_out)
{
    const char *who = "ses_ars_generation_batch";
    SES_REQUIRE(h && fitness && b && trials && mu_in && mu_out && theta_next, "%s: null argument", who);
    SES_REQUIRE(mu_in != mu_out, "%s: mu_in and mu_out must be distinct buffers", who);
    SES_REQUIRE(R >= 1, "%s: %d trials; there must be at least 1", who, R);
    SES_REQUIRE(n >= 4 && n % 2 == 0, "%s: %d rows per trial; ars samples in mirrored pairs: it must be even and >= 4", who, n);
    if (n > BARS_MAX_N)
        return set_error(SES_ERR_UNSUPPORTED, "%s: %d rows per trial; the batch tail ranks the pair scores by counting, up to %d rows "
                         "per trial", who, n, BARS_MAX_N);
    SES_REQUIRE((long long)R * n <= BARS_MAX_ROWS, "%s: %d trials x %d rows exceed %lld rows in all", who, R, n, BARS_MAX_ROWS);
    const int m = n / 2;
    int b_max = 1;
    for (int r = 0; r < R; ++r) {
        SES_REQUIRE(b[r] >= 1 && b[r] <= m, "%s: trial %d has b = %d directions of %d pairs; it must lie in [1, %d]", who, r, b[r], m, m);
        b_max = b[r] > b_max ? b[r] : b_max;
    }
    const int quads = (h->P + 3) / 4, P4 = 4 * quads;
    const int chunks_max = ceil_div(b_max, BARS_CHUNK);
    const int bpt = ceil_div((long long)m * quads, 256);                 // population workgroups per trial
    SES_REQUIRE((long long)quads * chunks_max + 1 <= 65535 && (long long)R * bpt < (1ll << 31),
                "%s: %d trials x %d rows x %d parameters exceed the launch grids", who, R, n, h->P);
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    const int pairs = R * m;
    const int jt = rank_count_slice(m);
    // scratch: the R rank vectors of m entries, one behind the other, where the solo tails keep their own | scores [R m] | BarsStat
    // [R] | sel [R][m] | chunk partials [R][chunks_max][P4].  Sized here, BEFORE the scores are written: it does not move under them.
    const size_t rank_bytes = bars_round256(sizeof(int32_t) * (size_t)pairs);
    const size_t scores_bytes = bars_round256(sizeof(float) * (size_t)pairs), stat_bytes = bars_round256(sizeof(BarsStat) * (size_t)R);
    const size_t sel_bytes = bars_round256(sizeof(int32_t) * (size_t)pairs);
    const int rc = ensure_reduce_scratch(h, rank_bytes + scores_bytes + stat_bytes + sel_bytes +
                                                sizeof(float) * (size_t)R * chunks_max * P4);
    if (rc != SES_OK) return rc;
    int32_t *rank = (int32_t *)h->red_scratch;
    float *scores = (float *)((char *)rank + rank_bytes);
    BarsStat *stat = (BarsStat *)((char *)scores + scores_bytes);
    int32_t *sel = (int32_t *)((char *)stat + stat_bytes);
    float *partial = (float *)((char *)sel + sel_bytes);
    hipLaunchKernelGGL(k_ars_scores, dim3(ceil_div(pairs, 256)), dim3(256), 0, h->stream, fitness, pairs, scores);
    // zero on entry: left so by the population-writing launch of the previous call, solo or batch, of the same entry count; a memset
    // otherwise.  From here to that launch the vector holds counts, and an early return leaves the cache saying so.
    const int zrc = tail_rank_take(h, rank, pairs);
    if (zrc != SES_OK) return zrc;
    h->counter_armed = nullptr;                     // the scores and partials may lie over the ticket counters of a solo layout
    hipLaunchKernelGGL(k_batch_rank_count, dim3(R, ceil_div(m, 256), ceil_div(m, jt)), dim3(256), 0, h->stream, scores, m, jt, rank);
    const BarsShape s{trials, R, m, chunks_max, h->P, P4, quads, partial, stat, sel, mu_in, mu_out, g_out, sigma_r_out, theta_next,
                      h->stamp, rank, pairs};
    hipLaunchKernelGGL(k_bars_grad_partial, dim3(R, quads * chunks_max + 1), dim3(256), 0, h->stream, s, rank, fitness, scores, best);
    if (h->tune.ars_fused_apply_perturb && h->P <= BARS_FOLD_MAX_P) {
        // the update inside the launch that draws the next population; it also clears the rank vectors
        hipLaunchKernelGGL(k_bars_perturb<true>, dim3(R * bpt), dim3(256), 0, h->stream, s, bpt);
    } else {
        hipLaunchKernelGGL(k_bars_apply, dim3(R, ceil_div(h->P, 256)), dim3(256), 0, h->stream, s);
        hipLaunchKernelGGL(k_bars_perturb<false>, dim3(R * bpt), dim3(256), 0, h->stream, s, bpt);
    }
    SES_HIP_TRY(hipGetLastError());
    tail_rank_cleared(h, rank, pairs);
    return SES_OK;
}

}  // extern "C"
