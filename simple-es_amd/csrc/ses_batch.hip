// ses_batch.hip -- the openai_es tail of R independent trials in one set of launches (ses_openai_generation_batch).
// A hyper-parameter sweep plays its trials as ONE device population of R x n rows (ses_rollout: rows are independent); this
// unit is the segmented tail behind it.  Trial r owns rows [r n, (r + 1) n) of the fitness vector and of the next population
// and row r of the [R, P] state matrices, and gets, bit for bit, what ses_openai_generation gives for its slice alone:
//
//   rank        the counting rank of ses_strategy.hip per trial: key = (ordered fitness bits, index WITHIN the trial), -0 as +0
//   gradient    chunks of BATCH_CHUNK = 1024 rows counted from the trial's first row; thread t of 256 takes rows row0 + t,
//               + 256, + 512, + 768 in ascending order (an fma chain), an 8-level LDS tree adds the pairs (t, t + s), s = 128 ... 1;
//               the weight is the closed form of the rank in double, sd formed on the device; row 0 of a trial is skipped
//   update      chunk partials added in ascending chunk order starting from chunk 0's value, * update_factor, adam_apply
//   population  row 0 of a trial = its new mean, every other row fma(next_sigma, z(seed, next_gen, row within the trial), mean)
//
// The trial is a grid dimension of every launch, so their number does not depend on R: rank, gradient, [update + population]
// for policies of up to 1024 parameters (three launches), rank, gradient, update, population above (four).  No launch needs an
// order between its workgroups: no ticket counters, no polling.  The per-trial scalars -- Philox keys, Adam's step scale, the
// update factor, the next sigma -- are read from a table in DEVICE memory that the caller wrote: no host-to-device copy here.
#include "ses_internal.h"
#include "ses_perturb_prologue.h"
#include "ses_rng.h"
#include "ses_tail.h"

namespace ses {

constexpr int BATCH_CHUNK = 1024;          // rows per gradient workgroup, counted from the trial's first row (ES_CHUNK)
constexpr int BATCH_FOLD_MAX_P = 1024;     // up to here the update runs inside the launch that writes the population
constexpr int BATCH_MAX_N = RANK_SORT_MIN; // rows per trial: the counting rank only
constexpr long long BATCH_MAX_ROWS = 1ll << 20;

// rank_key of ses_strategy.hip, restated (it lives in that unit, not in a header)
__device__ __forceinline__ unsigned long long batch_rank_key(uint32_t u, uint32_t index)
{
    u = u == 0x80000000u ? 0u : u;                                   // -0 -> +0
    const uint32_t ordered = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)ordered << 32) | (unsigned long long)index;
}

// k_rank_count_fitness per trial: grid (R, ceil(n / 256), ceil(n / jt)); rank[] must be zero on entry
__global__ __launch_bounds__(256) void k_batch_rank_count(const float *__restrict__ fit_all, int n, int jt,
                                                          int32_t *__restrict__ rank_all)
{
    const float *__restrict__ fit = fit_all + (size_t)blockIdx.x * n;
    int32_t *__restrict__ rank = rank_all + (size_t)blockIdx.x * n;
    const int i = blockIdx.y * 256 + threadIdx.x;
    const int j0 = blockIdx.z * jt;
    const int lim = n - j0 < jt ? n - j0 : jt;
    const int ic = i < n ? i : n - 1;
    const unsigned long long ki = batch_rank_key(f2u(fit[ic]), (uint32_t)ic);
    const uint32_t *__restrict__ fj = reinterpret_cast<const uint32_t *>(fit) + j0;   // uniform base: scalar loads below
    int count = 0;
    int k = 0;
    for (; k + 16 <= lim; k += 16) {
        uint32_t c[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) c[e] = fj[k + e];
#pragma unroll
        for (int e = 0; e < 16; ++e) count += (batch_rank_key(c[e], (uint32_t)(j0 + k + e)) > ki) ? 1 : 0;
    }
    for (; k < lim; ++k) count += (batch_rank_key(fj[k], (uint32_t)(j0 + k)) > ki) ? 1 : 0;
    if (i < n && count) atomicAdd(&rank[i], count);
}

// k_es_grad_partial_ranked<false> per trial: grid (R, quads, chunks) -> partial[trial][chunk][P4]; the thread that meets the
// trial's rank 0 reports best[trial] = max(fitness of the trial)
__global__ __launch_bounds__(256) void k_batch_grad_partial(const int32_t *__restrict__ rank_all,
                                                            const float *__restrict__ fit_all, int n,
                                                            const ses_batch_trial *__restrict__ trials, int P4, int chunks,
                                                            float *__restrict__ partial, float *__restrict__ best)
{
    __shared__ float red[4][256];
    const int r = blockIdx.x, q = blockIdx.y, c = blockIdx.z;
    const uint64_t seed = trials[r].seed, gen = trials[r].gen;            // uniform
    const int32_t *__restrict__ rank = rank_all + (size_t)r * n;
    const float *__restrict__ fitness = fit_all + (size_t)r * n;
    const int row0 = c * BATCH_CHUNK;
    const int row1 = row0 + BATCH_CHUNK < n ? row0 + BATCH_CHUNK : n;
    const double nm1 = (double)(n - 1);
    const double sd = sqrt((double)(n + 1) / (12.0 * nm1));           // closed-form std of the rank grid
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = row0 + threadIdx.x; i < row1; i += 256) {
        const int rk = rank[i];
        if (q == 0 && rk == 0 && best) best[r] = fitness[i];          // max(rewards), loop.py:82-84 `best_reward`
        if (i == 0) continue;                                          // the trial's mean itself: eps = 0
        const double centred = ((double)(n - 1 - rk) / nm1) - 0.5;     // offspring_strategies.py:394-396
        const float w = (float)(centred / sd);
        float z[4];
        normal4(seed, gen, (uint32_t)i, (uint32_t)q, z);
#pragma unroll
        for (int l = 0; l < 4; ++l) acc[l] = fma_(w, z[l], acc[l]);
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
    if (threadIdx.x < 4) partial[((size_t)r * chunks + c) * P4 + 4 * q + threadIdx.x] = red[threadIdx.x][0];
}

// what the launches that end the batch tail are given
struct BatchUpdate {
    const float *partial;                  // [R][chunks][P4]
    const ses_batch_trial *trials;         // [R], device
    int R, n, chunks, P, P4, quads;
    int blocks_per_trial;                  // workgroups of one trial in k_batch_apply_perturb / k_batch_apply
    const float *mu_in, *m_in, *v_in;      // [R, P]
    float *mu_out, *m_out, *v_out;         // [R, P], distinct from *_in
    float *theta;                          // [R n, P]
    unsigned long long *stamp;
    int32_t *rank_to_clear;
    int n_clear;
};

// quad q of row i of trial `tr` from the trial's new mean (k_perturb_openai: row 0 is the mean itself)
__device__ __forceinline__ void batch_row_quad(const BatchUpdate &u, const ses_batch_trial &tr, size_t row_global, int i, int q,
                                               const float *mu_new)
{
    const int lim = u.P - 4 * q < 4 ? u.P - 4 * q : 4;
    float *dst = u.theta + row_global * u.P + 4 * q;
    if (i == 0) {
        for (int l = 0; l < lim; ++l) dst[l] = mu_new[4 * q + l];
        return;
    }
    float z[4];
    normal4(tr.seed, tr.next_gen, (uint32_t)i, (uint32_t)q, z);
    for (int l = 0; l < lim; ++l) dst[l] = fma_(tr.next_sigma, z[l], mu_new[4 * q + l]);
}

// k_es_apply_perturb per trial (P <= BATCH_FOLD_MAX_P): workgroup blockIdx.x = trial * blocks_per_trial + b serves ONE trial -- it
// forms that trial's whole new mean in LDS, a thread per parameter (b == 0 also stores mu / m / v), and writes 256 (row, quad)
// items of the trial's rows from it.  The in and out matrices are distinct buffers: no workgroup reads what another replaced.
__global__ __launch_bounds__(256) void k_batch_apply_perturb(BatchUpdate u)
{
    __shared__ float mu_new[BATCH_FOLD_MAX_P];
    const int r = blockIdx.x / u.blocks_per_trial, b = blockIdx.x - r * u.blocks_per_trial;
    const ses_batch_trial tr = u.trials[r];                              // uniform
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u.stamp && t == 0) *u.stamp = real_time();
    const float *__restrict__ part = u.partial + (size_t)r * u.chunks * u.P4;
    for (int p = threadIdx.x; p < u.P; p += 256) {
        float sum = part[p];
        for (int c = 1; c < u.chunks; ++c) sum = sum + part[(size_t)c * u.P4 + p];
        const float g = sum * tr.update_factor;                          // offspring_strategies.py:414
        const size_t at = (size_t)r * u.P + p;
        float muv = u.mu_in[at], mv = u.m_in[at], vv = u.v_in[at];
        adam_apply(g, tr.adam_a, muv, mv, vv);
        mu_new[p] = muv;
        if (b == 0) { u.mu_out[at] = muv; u.m_out[at] = mv; u.v_out[at] = vv; }
    }
    // the rank vectors have been consumed by the gradient kernel: leave them zeroed for the next generation's count
    for (long long i = t; i < u.n_clear; i += (long long)gridDim.x * 256) u.rank_to_clear[i] = 0;
    __syncthreads();
    const long long item = (long long)b * 256 + threadIdx.x;
    if (item >= (long long)u.n * u.quads) return;
    const int i = (int)(item / u.quads);
    const int q = (int)(item - (long long)i * u.quads);
    batch_row_quad(u, tr, (size_t)r * u.n + i, i, q, mu_new);
}

// k_es_apply per trial (P > BATCH_FOLD_MAX_P): one wavefront per (trial, parameter); lane c fetches the partial of chunk c, the
// wave adds them in ascending chunk order through v_readlane
__global__ __launch_bounds__(256) void k_batch_apply(BatchUpdate u)
{
    const int r = blockIdx.x / u.blocks_per_trial, b = blockIdx.x - r * u.blocks_per_trial;
    const int p = b * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= u.P) return;                                                // wave-uniform
    const float *__restrict__ part = u.partial + (size_t)r * u.chunks * u.P4;
    float sum = 0.0f;
    for (int base = 0; base < u.chunks; base += 64) {
        const int cm = base + lane;
        const float mine = cm < u.chunks ? part[(size_t)cm * u.P4 + p] : 0.0f;
        const int cnt = u.chunks - base < 64 ? u.chunks - base : 64;
        for (int c = 0; c < cnt; ++c) {
            const float x = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine), c));
            sum = (base + c == 0) ? x : sum + x;
        }
    }
    if (lane != 0) return;
    const float g = sum * u.trials[r].update_factor;                     // offspring_strategies.py:414
    const size_t at = (size_t)r * u.P + p;
    float muv = u.mu_in[at], mv = u.m_in[at], vv = u.v_in[at];
    adam_apply(g, u.trials[r].adam_a, muv, mv, vv);
    u.mu_out[at] = muv; u.m_out[at] = mv; u.v_out[at] = vv;
}

// k_perturb_openai per trial: one thread per (row of the whole batch, quad), the mean read from mu_out[trial]
__global__ __launch_bounds__(256) void k_batch_perturb(BatchUpdate u)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u.stamp && t == 0) *u.stamp = real_time();
    for (long long i = t; i < u.n_clear; i += (long long)gridDim.x * 256) u.rank_to_clear[i] = 0;
    if (t >= (long long)u.R * u.n * u.quads) return;
    const long long row = t / u.quads;
    const int q = (int)(t - row * u.quads);
    const int r = (int)(row / u.n);
    const int i = (int)(row - (long long)r * u.n);
    batch_row_quad(u, u.trials[r], (size_t)row, i, q, u.mu_out + (size_t)r * u.P);
}

}  // namespace ses

extern "C" {

using namespace ses;

int ses_openai_generation_batch(ses_handle *h, const float *fitness, int32_t R, int32_t n, const ses_batch_trial *trials,
                                const float *mu_in, const float *m_in, const float *v_in, float *mu_out, float *m_out,
                                float *v_out, float *theta_next, float *best)
{
    const char *who = "ses_openai_generation_batch";
    SES_REQUIRE(h && fitness && trials && mu_in && m_in && v_in && mu_out && m_out && v_out && theta_next, "%s: null argument", who);
    SES_REQUIRE(mu_in != mu_out && m_in != m_out && v_in != v_out, "%s: in and out matrices must be distinct buffers", who);
    SES_REQUIRE(R >= 1, "%s: %d trials; there must be at least 1", who, R);
    SES_REQUIRE(n >= 2, "%s: %d rows per trial; there must be at least 2", who, n);
    if (n > BATCH_MAX_N)
        return set_error(SES_ERR_UNSUPPORTED, "%s: %d rows per trial; the batch tail ranks by counting, up to %d rows per trial", who, n,
                         BATCH_MAX_N);
    SES_REQUIRE((long long)R * n <= BATCH_MAX_ROWS, "%s: %d trials x %d rows exceed %lld rows in all", who, R, n, BATCH_MAX_ROWS);
    const int quads = (h->P + 3) / 4, P4 = 4 * quads;
    SES_REQUIRE(quads <= 65535 && (long long)R * ceil_div(h->P, 4) < (1ll << 31) && (long long)R * n * quads / 256 < (1ll << 31),
                "%s: %d trials x %d rows x %d parameters exceed the launch grids", who, R, n, h->P);
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    const int rows = R * n;
    const int jt = rank_count_slice(n);
    const int chunks = ceil_div(n, BATCH_CHUNK);
    // scratch: the R rank vectors, one behind the other, where ses_openai_generation keeps its own | chunk partials [R][chunks][P4]
    const size_t rank_bytes = (sizeof(int32_t) * (size_t)rows + 255) / 256 * 256;
    const int rc = ensure_reduce_scratch(h, rank_bytes + sizeof(float) * (size_t)R * chunks * P4);
    if (rc != SES_OK) return rc;
    int32_t *rank = (int32_t *)h->red_scratch;
    float *partial = (float *)((char *)rank + rank_bytes);
    // zero on entry: left so by the population-writing launch of the previous call, solo or batch, of the same row count; a memset
    // otherwise.  From here to that launch the vector holds counts, and an early return leaves the cache saying so.
    const int zrc = tail_rank_take(h, rank, rows);
    if (zrc != SES_OK) return zrc;
    h->counter_armed = nullptr;                     // the partials may lie over the ticket counters of a solo layout
    hipLaunchKernelGGL(k_batch_rank_count, dim3(R, ceil_div(n, 256), ceil_div(n, jt)), dim3(256), 0, h->stream, fitness, n, jt, rank);
    hipLaunchKernelGGL(k_batch_grad_partial, dim3(R, quads, chunks), dim3(256), 0, h->stream, rank, fitness, n, trials, P4, chunks,
                       partial, best);
    BatchUpdate u{partial, trials, R, n, chunks, h->P, P4, quads, 0, mu_in, m_in, v_in, mu_out, m_out, v_out, theta_next, h->stamp,
                  rank, rows};
    if (h->P <= BATCH_FOLD_MAX_P) {
        u.blocks_per_trial = ceil_div((long long)n * quads, 256);
        hipLaunchKernelGGL(k_batch_apply_perturb, dim3((unsigned)((long long)R * u.blocks_per_trial)), dim3(256), 0, h->stream, u);
    } else {
        u.blocks_per_trial = ceil_div(h->P, 4);
        hipLaunchKernelGGL(k_batch_apply, dim3((unsigned)((long long)R * u.blocks_per_trial)), dim3(256), 0, h->stream, u);
        hipLaunchKernelGGL(k_batch_perturb, dim3(ceil_div((long long)rows * quads, 256)), dim3(256), 0, h->stream, u);
    }
    SES_HIP_TRY(hipGetLastError());
    tail_rank_cleared(h, rank, rows);
    return SES_OK;
}

}  // extern "C"
