// ses_ars.hip -- the ars strategy: Augmented Random Search over the best mirrored directions (Mania, Guy & Recht 2018, "Simple random
// search provides a competitive approach to reinforcement learning", the V1-t form: top-b directions, the step divided by the standard
// deviation of the returns that were kept, a plain step, no Adam).  No reference counterpart: an eighth strategy with the shape of the
// pgpe tail.
//
//   population  n = 2 m rows, pair j = rows (2 j, 2 j + 1):  theta = mu +- sigma * z(seed, gen, row = j, p)     (pgpe's, scale = 1)
//   tail        pair scores -> rank of the m scores -> [gradient over the b selected pairs | sigma_R] -> update -> next population
//
// Only b of the m pairs contribute and the rank names them BEFORE the sum: a gradient workgroup inverts the rank vector for its chunk
// of 1024 SELECTED pairs into LDS (sel[k] = the pair of rank k) and draws Philox numbers for those pairs alone.  Summation order of
// G[p] (depends on (n, b) only): chunks of ARS_CHUNK = 1024 selected pairs in rank order; inside a chunk thread c of 256 takes
// k = c, c + 256, c + 512, c + 768 (an fma chain), an 8-level LDS tree combines the 256 threads (s = 128 ... 1: x[c] += x[c + s]),
// the chunk partials are added in ascending chunk order.  sigma_R: one further workgroup of the gradient launch, in double, see
// ars_sigma_r.
#include "ses_internal.h"
#include "ses_rng.h"
#include "ses_tail.h"

namespace ses {

constexpr int ARS_CHUNK = 1024;            // selected pairs per gradient workgroup
constexpr int ARS_FOLD_MAX_P = 1024;       // the update inside the perturbation launch: up to this many parameters ...
constexpr int ARS_FOLD_MAX_CHUNKS = 16;    // ... and this many chunk partials

// what the sigma_R workgroup leaves for the update
struct ArsStat {
    double sigma_r;
    float step;
    float pad;
};

// ---- pair scores ---------------------------------------------------------------------------------------------------------
// s_j = max(f[2j], f[2j+1]): the vector the rank kernels rank
__global__ __launch_bounds__(256) void k_ars_scores(const float *__restrict__ fitness, int m, float *__restrict__ scores)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    scores[j] = fmaxf(fitness[2 * j], fitness[2 * j + 1]);
}

// ---- sigma_R -------------------------------------------------------------------------------------------------------------
// One workgroup.  Writes the selected list sel[k] = pair of rank k (k < b) to global memory for itself, then the population standard
// deviation of the 2 b values e -> f[2 sel[e / 2] + (e & 1)], in double, two passes: thread c adds the elements c, c + 256, ... in
// ascending order to 0.0, the 8-level tree adds the threads; mean = sum / (2 b); the same for the squared deviations (product and
// sum rounded separately: no fma); sigma_R = sqrt(sum / (2 b)), correctly rounded.  step = lr / (b sigma_R), 0 where sigma_R = 0.
// A fitness vector with NaNs has no strict order: its rank vector is no permutation and leaves entries of the selected list unwritten.
// Every read of the list is held inside the population, whatever it finds there.
__device__ __forceinline__ int ars_pair(int j, int m) { return j < 0 ? 0 : j >= m ? m - 1 : j; }

__device__ __forceinline__ double ars_tree(double (&x)[256], double mine)
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

__device__ void ars_sigma_r(const int32_t *__restrict__ rank, const float *__restrict__ fitness, const float *__restrict__ scores,
                            int m, int b, double learning_rate, int32_t *sel, ArsStat *stat, float *best)
{
    __shared__ double x[256];
    for (int j = threadIdx.x; j < m; j += 256) {
        const int r = rank[j];
        if (r >= 0 && r < b) sel[r] = j;                                 // rank is a permutation of 0 .. m - 1: every entry written once
        if (r == 0 && best) *best = scores[j];                           // max(fitness)
    }
    __threadfence();
    __syncthreads();
    const long long count = 2ll * b;
    double acc = 0.0;
    for (long long e = threadIdx.x; e < count; e += 256)
        acc = __dadd_rn(acc, (double)fitness[2ll * ars_pair(sel[e >> 1], m) + (e & 1)]);
    const double mean = ars_tree(x, acc) / (double)count;
    acc = 0.0;
    for (long long e = threadIdx.x; e < count; e += 256) {
        const double dv = __dsub_rn((double)fitness[2ll * ars_pair(sel[e >> 1], m) + (e & 1)], mean);
        acc = __dadd_rn(acc, __dmul_rn(dv, dv));
    }
    const double var = ars_tree(x, acc) / (double)count;
    if (threadIdx.x == 0) {
        const double sr = __dsqrt_rn(var);
        stat->sigma_r = sr;
        stat->step = sr > 0.0 ? (float)(learning_rate / ((double)b * sr)) : 0.0f;
        stat->pad = 0.0f;
    }
}

// ---- gradient over the selected pairs --------------------------------------------------------------------------------------
// Workgroup w < quads * chunks: parameter quad q = w % quads, chunk = w / quads of the selected list.  d_k = (float)((double)f[2 sel_k]
// - (double)f[2 sel_k + 1]), G[p] += d_k z_{sel_k, p}: four float32 accumulators per thread, the LDS tree, one partial per chunk.
// Workgroup quads * chunks: sigma_R (above).  Unselected pairs draw nothing.
__global__ __launch_bounds__(256) void k_ars_grad_partial(const int32_t *__restrict__ rank, const float *__restrict__ fitness,
                                                          const float *__restrict__ scores, int m, int b, uint64_t seed,
                                                          uint64_t gen, int quads, int chunks, double learning_rate,
                                                          float *__restrict__ partial, int32_t *sel_all, ArsStat *stat,
                                                          float *__restrict__ best)
{
    if ((int)blockIdx.x == quads * chunks) {                             // workgroup-uniform
        ars_sigma_r(rank, fitness, scores, m, b, learning_rate, sel_all, stat, best);
        return;
    }
    __shared__ int32_t sel[ARS_CHUNK];
    __shared__ float red[4][256];
    const int q = blockIdx.x % quads, chunk = blockIdx.x / quads;
    const int k0 = chunk * ARS_CHUNK;
    const int cnt = b - k0 < ARS_CHUNK ? b - k0 : ARS_CHUNK;
    for (int j = threadIdx.x; j < m; j += 256) {
        const int r = rank[j] - k0;
        if (r >= 0 && r < cnt) sel[r] = j;
    }
    __syncthreads();
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k = threadIdx.x; k < cnt; k += 256) {
        const int j = ars_pair(sel[k], m);
        const float d = (float)((double)fitness[2 * j] - (double)fitness[2 * j + 1]);
        float z[4];
        normal4(seed, gen, (uint32_t)j, (uint32_t)q, z);
#pragma unroll
        for (int l = 0; l < 4; ++l) acc[l] = fma_(d, z[l], acc[l]);
    }
#pragma unroll
    for (int l = 0; l < 4; ++l) red[l][threadIdx.x] = acc[l];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
#pragma unroll
            for (int l = 0; l < 4; ++l) red[l][threadIdx.x] = red[l][threadIdx.x] + red[l][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < 4) partial[(size_t)chunk * (4 * quads) + 4 * q + threadIdx.x] = red[threadIdx.x][0];
}

// ---- update ------------------------------------------------------------------------------------------------------------
struct ArsUpdate {
    const float *partial;
    const ArsStat *stat;
    int chunks, P, P4;
    const float *mu;
    float *mu_out, *g_out;
    double *sigma_r_out;
};

// G[p] = the chunk partials in ascending order; mu'[p] = fl(mu[p] + fl(step * G[p])).  store: mu_out and the optional G are written.
__device__ __forceinline__ float ars_update_param(const ArsUpdate &u, int p, float step, bool store)
{
    float g = u.partial[p];
    for (int c = 1; c < u.chunks; ++c) g = g + u.partial[(size_t)c * u.P4 + p];
    const float mu_new = __fadd_rn(u.mu[p], __fmul_rn(step, g));
    if (store) {
        if (u.g_out) u.g_out[p] = g;
        u.mu_out[p] = mu_new;
    }
    return mu_new;
}

// a thread per parameter (policies above ARS_FOLD_MAX_P parameters, or the knob "ars_fused_apply_perturb" = 0)
__global__ __launch_bounds__(256) void k_ars_apply(ArsUpdate u)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p == 0 && u.sigma_r_out) *u.sigma_r_out = u.stat->sigma_r;
    if (p >= u.P) return;
    ars_update_param(u, p, u.stat->step, true);
}

// The mirrored perturbation (k_perturb_mirrored's thread layout with scale = 1: one thread = one Philox call = 4 consecutive parameters
// of both rows of one pair, rows global, one rounding per operation).  FUSED: EVERY workgroup first forms the whole new mean itself
// into LDS (k_pgpe_apply_perturb's form; workgroup 0 also stores it) -- the same sums in the same order as k_ars_apply, so the two
// forms are bit-equal.  Not FUSED: `center` is the mean to draw from.  Either way the launch stamps the tail time and zeroes the rank
// vector for the next generation's count.
template <bool FUSED>
__global__ __launch_bounds__(256) void k_ars_perturb(ArsUpdate u, const float *__restrict__ center, float sigma, uint64_t seed,
                                                     uint64_t gen, long long first_row, int n_rows, int P, int quads,
                                                     float *__restrict__ theta, unsigned long long *__restrict__ stamp,
                                                     int32_t *__restrict__ rank_to_clear, int n_clear)
{
    __shared__ float mu_new[FUSED ? ARS_FOLD_MAX_P : 1];
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (stamp && t == 0) *stamp = real_time();
    if (FUSED) {
        const float step = u.stat->step;
        if (t == 0 && u.sigma_r_out) *u.sigma_r_out = u.stat->sigma_r;
        for (int p = threadIdx.x; p < u.P; p += 256) mu_new[p] = ars_update_param(u, p, step, blockIdx.x == 0);
    }
    for (long long i = t; i < n_clear; i += (long long)gridDim.x * blockDim.x) rank_to_clear[i] = 0;
    if (FUSED) __syncthreads();
    if (n_rows <= 0) return;
    const long long pair0 = first_row >> 1;
    const long long pairs = ((first_row + n_rows - 1) >> 1) - pair0 + 1;
    if (t >= pairs * quads) return;
    const long long jl = t / quads;
    const int q = (int)(t - jl * quads);
    const long long j = pair0 + jl;
    const int lim = P - 4 * q < 4 ? P - 4 * q : 4;
    float z[4];
    normal4(seed, gen, (uint32_t)j, (uint32_t)q, z);
    const long long even = 2 * j - first_row, odd = even + 1;           // the pair's rows, counted from the shard's first
    const bool has_even = even >= 0, has_odd = odd < n_rows;
    float *dst_even = theta + (size_t)(has_even ? even : 0) * P + 4 * q;
    float *dst_odd = theta + (size_t)(has_odd ? odd : 0) * P + 4 * q;
    for (int l = 0; l < lim; ++l) {
        const float c = FUSED ? mu_new[4 * q + l] : center[4 * q + l];
        const float d = __fmul_rn(sigma, z[l]);
        if (has_even) dst_even[l] = __fadd_rn(c, d);
        if (has_odd) dst_odd[l] = __fsub_rn(c, d);
    }
}

static size_t round256(size_t bytes) { return (bytes + 255) / 256 * 256; }

}  // namespace ses

extern "C" {

using namespace ses;

int ses_ars_generation(ses_handle *h, const float *fitness, int32_t n, int32_t b, uint64_t seed, uint64_t gen, double sigma,
                       double learning_rate, const float *mu_in, float *mu_out, float next_sigma, uint64_t next_gen,
                       int64_t first_row, int32_t n_rows, float *theta_next, float *best, float *g_out, double *sigma_r_out)
{
    (void)sigma;                                                         // the evaluated population's sigma does not enter the update
    SES_REQUIRE(h && fitness && mu_in && mu_out, "ses_ars_generation: null argument");
    SES_REQUIRE(mu_in != mu_out, "ses_ars_generation: mu_in and mu_out must be distinct buffers");
    int rc = tail_check_rows("ses_ars_generation", n, true, first_row, n_rows, theta_next);
    if (rc != SES_OK) return rc;
    const int m = n / 2;
    SES_REQUIRE(b >= 1 && b <= m, "ses_ars_generation: b = %d directions of %d pairs; it must lie in [1, %d]", b, m, m);
    const int quads = (h->P + 3) / 4, P4 = 4 * quads;
    const int chunks = ceil_div(b, ARS_CHUNK);
    // The scratch: tail_rank_begin's own layout for a vector of m entries -- sorted tiles (m > RANK_SORT_MIN) | rank[m], rounded up
    // to 256 bytes -- and behind it, as the caller's bytes: scores[m] | ArsStat | sel[b] | the chunk partials.  The scores are
    // written BEFORE tail_rank_begin ranks them, so the buffer is sized here first (it does not move below: the same total).
    const size_t sorted_bytes = m > RANK_SORT_MIN ? sizeof(unsigned long long) * (size_t)ceil_div(m, RANK_TILE) * RANK_TILE : 0;
    const size_t rank_bytes = round256(sizeof(int32_t) * (size_t)m);
    const size_t scores_bytes = round256(sizeof(float) * (size_t)m), stat_bytes = round256(sizeof(ArsStat));
    const size_t sel_bytes = round256(sizeof(int32_t) * (size_t)b);
    const size_t extra_bytes = scores_bytes + stat_bytes + sel_bytes + sizeof(float) * (size_t)chunks * P4;
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    rc = ensure_reduce_scratch(h, sorted_bytes + rank_bytes + extra_bytes);
    if (rc != SES_OK) return rc;
    float *scores = (float *)((char *)h->red_scratch + sorted_bytes + rank_bytes);
    hipLaunchKernelGGL(k_ars_scores, dim3(ceil_div(m, 256)), dim3(256), 0, h->stream, fitness, m, scores);
    int32_t *rank;
    char *extra;
    rc = tail_rank_begin(h, scores, m, extra_bytes, &rank, (void **)&extra);
    if (rc != SES_OK) return rc;
    SES_REQUIRE((float *)extra == scores, "ses_ars_generation: the scratch layout moved under the scores");
    ArsStat *stat = (ArsStat *)(extra + scores_bytes);
    int32_t *sel = (int32_t *)(extra + scores_bytes + stat_bytes);
    float *partial = (float *)(extra + scores_bytes + stat_bytes + sel_bytes);
    hipLaunchKernelGGL(k_ars_grad_partial, dim3(quads * chunks + 1), dim3(256), 0, h->stream, rank, fitness, scores, m, b, seed, gen,
                       quads, chunks, learning_rate, partial, sel, stat, best);
    const ArsUpdate u{partial, stat, chunks, h->P, P4, mu_in, mu_out, g_out, sigma_r_out};
    const long long npairs = n_rows > 0 ? ((first_row + n_rows - 1) >> 1) - (first_row >> 1) + 1 : 1;
    const dim3 grid(ceil_div(npairs * quads, 256));
    if (h->tune.ars_fused_apply_perturb && h->P <= ARS_FOLD_MAX_P && chunks <= ARS_FOLD_MAX_CHUNKS && n_rows > 0) {
        // the update inside the launch that draws the next population; it also clears the rank vector
        hipLaunchKernelGGL(k_ars_perturb<true>, grid, dim3(256), 0, h->stream, u, nullptr, next_sigma, seed, next_gen,
                           (long long)first_row, n_rows, h->P, quads, theta_next, h->stamp, rank, m);
    } else {
        hipLaunchKernelGGL(k_ars_apply, dim3(ceil_div(h->P, 256)), dim3(256), 0, h->stream, u);
        hipLaunchKernelGGL(k_ars_perturb<false>, grid, dim3(256), 0, h->stream, u, mu_out, next_sigma, seed, next_gen,
                           (long long)first_row, n_rows, h->P, quads, theta_next, h->stamp, rank, m);
    }
    SES_HIP_TRY(hipGetLastError());
    tail_rank_cleared(h, rank, m);
    return SES_OK;
}

}  // extern "C"
