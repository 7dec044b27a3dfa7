// ses_pgpe.hip -- the pgpe strategy: PGPE with symmetric (mirrored) sampling and a per-parameter step size
// (Sehnke et al. 2010, "Parameter-exploring policy gradients"; the rank shaping and Adam of openai_es, Salimans et al. 2017).
// No reference counterpart: the reference has three strategies, this is a fourth with the shape of the openai_es tail.
//
//   population  n = 2 m rows, pair j = rows (2 j, 2 j + 1):  theta = mu +- (sigma * scale[p]) * z(seed, gen, row = j, p)
//   tail        rank -> pair gradient (chunk partials of Gmu, Gs) -> update of (mu, m, v, scale) -> next population
//
// One normal serves both rows of a pair, in the perturbation and in the gradient: half the Philox / Box-Muller draws of
// openai_es per row.  Summation order of Gmu[p] / Gs[p] (depends on n only): chunks of PGPE_CHUNK = 1024 pairs; inside a chunk
// thread c of 256 takes pairs c, c + 256, c + 512, c + 768 in ascending order (an fma chain), an 8-level LDS tree combines
// the 256 threads (s = 128, 64, ..., 1: x[c] += x[c + s]), the chunk partials are added in ascending chunk order.
#include "ses_internal.h"
#include "ses_perturb_prologue.h"
#include "ses_rng.h"
#include "ses_tail.h"

namespace ses {

constexpr int PGPE_CHUNK = 1024;           // pairs per gradient workgroup

// ---- mirrored perturbation ---------------------------------------------------------------------------------------------
// one thread = one Philox call = 4 consecutive parameters of BOTH rows of one pair.  Rows are global: the shard
// [first_row, first_row + n_rows) may begin with the odd row of a pair and end with the even row of one; the thread of such
// a pair writes the one row that belongs to the shard.  One rounding per operation (no fma): a float32 restatement in numpy
// is bit-exact.
__global__ __launch_bounds__(256) void k_perturb_mirrored(const float *__restrict__ mu, const float *__restrict__ scale,
                                                          float sigma, uint64_t seed, uint64_t gen, long long first_row,
                                                          int n_rows, int P, int quads, float *__restrict__ theta,
                                                          unsigned long long *__restrict__ stamp,
                                                          int32_t *__restrict__ rank_to_clear, int n_clear)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (stamp && t == 0) *stamp = real_time();                           // ses_set_stamp: the next population is being written
    // the rank vector has been consumed by the gradient kernel: leave it zeroed for the next generation's count
    for (long long i = t; i < n_clear; i += (long long)gridDim.x * blockDim.x) rank_to_clear[i] = 0;
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
    const bool has_even = even >= 0, has_odd = odd < n_rows;            // (even < n_rows and odd >= 0 by the pair range)
    float *dst_even = theta + (size_t)(has_even ? even : 0) * P + 4 * q;
    float *dst_odd = theta + (size_t)(has_odd ? odd : 0) * P + 4 * q;
    for (int l = 0; l < lim; ++l) {
        const float center = mu[4 * q + l];
        const float sig = __fmul_rn(sigma, scale[4 * q + l]);
        const float d = __fmul_rn(sig, z[l]);
        if (has_even) dst_even[l] = __fadd_rn(center, d);
        if (has_odd) dst_odd[l] = __fsub_rn(center, d);
    }
}

// ---- pair gradient -----------------------------------------------------------------------------------------------------
// One 256-thread workgroup per (parameter quad, chunk of PGPE_CHUNK pairs).  The rank-centring weights of the two rows are
// formed where they are used (the closed form of k_es_grad_partial_ranked, in double), then
//     d_j = (float)((w[2j] - w[2j+1]) / 2)   a_j = (float)((w[2j] + w[2j+1]) / 2)
//     Gmu[p] += d_j * z_jp                   Gs[p] += a_j * fma(z_jp, z_jp, -1)
// with eight float32 accumulators per thread (4 parameters x {mu, scale}), an LDS tree over the 256 threads and one partial
// per chunk: partial[chunk][p] for Gmu, partial[chunks * P4 + chunk * P4 + p] for Gs.  The single-rounding fma of z * z - 1
// keeps a relative bound where fl(z * z) - 1 cancels (|z| near 1).  The thread that meets rank 0 reports best = max(fitness).
__global__ __launch_bounds__(256) void k_pgpe_grad_partial(const int32_t *__restrict__ rank, const float *__restrict__ fitness,
                                                           int n, uint64_t seed, uint64_t gen, int P4, int chunks,
                                                           float *__restrict__ partial, float *__restrict__ best)
{
    __shared__ float red[8][256];
    const int q = blockIdx.x;
    const int pairs = n >> 1;
    const int pair0 = blockIdx.y * PGPE_CHUNK;
    const int pair1 = pair0 + PGPE_CHUNK < pairs ? pair0 + PGPE_CHUNK : pairs;
    const double nm1 = (double)(n - 1);
    const double sd = sqrt((double)(n + 1) / (12.0 * nm1));           // closed-form std of the rank grid
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = pair0 + threadIdx.x; j < pair1; j += 256) {
        const int2 r = reinterpret_cast<const int2 *>(rank)[j];
        if (q == 0 && best) {                                          // max(rewards)
            if (r.x == 0) *best = fitness[2 * j];
            if (r.y == 0) *best = fitness[2 * j + 1];
        }
        const double w0 = (((double)(n - 1 - r.x) / nm1) - 0.5) / sd;
        const double w1 = (((double)(n - 1 - r.y) / nm1) - 0.5) / sd;
        const float d = (float)((w0 - w1) * 0.5);
        const float a = (float)((w0 + w1) * 0.5);
        float z[4];
        normal4(seed, gen, (uint32_t)j, (uint32_t)q, z);
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            acc[l] = fma_(d, z[l], acc[l]);
            acc[4 + l] = fma_(a, fma_(z[l], z[l], -1.0f), acc[4 + l]);
        }
    }
#pragma unroll
    for (int l = 0; l < 8; ++l) red[l][threadIdx.x] = acc[l];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
#pragma unroll
            for (int l = 0; l < 8; ++l) red[l][threadIdx.x] = red[l][threadIdx.x] + red[l][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < 8) {
        const int half = threadIdx.x >> 2, l = threadIdx.x & 3;
        partial[((size_t)half * chunks + blockIdx.y) * P4 + 4 * q + l] = red[threadIdx.x][0];
    }
}

// ---- update ------------------------------------------------------------------------------------------------------------
// What the update of one generation is given: the chunk partials, the constants, the vectors it reads and writes.
struct PgpeUpdate {
    const float *partial;
    int chunks, P, P4;
    float sigma, cm;
    double adam_a;
    float cs, lo_f, hi_f, scale_lo, scale_hi;
    const float *mu, *m, *v, *scale;
    float *mu_out, *m_out, *v_out, *scale_out, *gmu_out, *gs_out;
};

// Parameter p from its two sums, with sig_p = fl(sigma * scale[p]) the one the evaluated population was drawn with:
//     grad_mu = fl(fl(Gmu * sig_p) * cm)                cm = (float)(-1 / m)          -> adam_apply (unchanged helper)
//     ds = fl(fl(Gs * scale) * cs)                      cs = (float)(sigma_learning_rate / m)
//     s1 = fl(scale + ds), clipped to [scale * lo_f, scale * hi_f] (lo_f, hi_f = (float)(1 -+ sigma_max_change)), then to
//     [scale_lo, scale_hi].
// store: (mu, m, v, scale)_out and the optional sums are written (inputs and outputs are distinct buffers, the caller ping-pongs).
__device__ __forceinline__ void pgpe_update_param(const PgpeUpdate &u, int p, float gmu, float gs, bool store, float &mu_new,
                                                  float &scale_new)
{
    const float sc = u.scale[p];
    const float sig = __fmul_rn(u.sigma, sc);
    const float g = __fmul_rn(__fmul_rn(gmu, sig), u.cm);
    float muv = u.mu[p], mv = u.m[p], vv = u.v[p];
    adam_apply(g, u.adam_a, muv, mv, vv);
    const float ds = __fmul_rn(__fmul_rn(gs, sc), u.cs);
    const float s1 = __fadd_rn(sc, ds);
    const float s2 = fminf(fmaxf(s1, __fmul_rn(sc, u.lo_f)), __fmul_rn(sc, u.hi_f));
    mu_new = muv;
    scale_new = fminf(fmaxf(s2, u.scale_lo), u.scale_hi);
    if (!store) return;
    if (u.gmu_out) u.gmu_out[p] = gmu;
    if (u.gs_out) u.gs_out[p] = gs;
    u.mu_out[p] = muv; u.m_out[p] = mv; u.v_out[p] = vv;
    u.scale_out[p] = scale_new;
}

// One wavefront per parameter, k_es_apply's form: lane c fetches the two partials of chunk c, the wave adds them in ascending
// chunk order through v_readlane; lane 0 updates the parameter.
__global__ __launch_bounds__(256) void k_pgpe_apply(PgpeUpdate u)
{
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= u.P) return;                                                // wave-uniform
    const float *part_s = u.partial + (size_t)u.chunks * u.P4;
    float gmu = 0.0f, gs = 0.0f;
    for (int base = 0; base < u.chunks; base += 64) {
        const int cmine = base + lane;
        const float mine_mu = cmine < u.chunks ? u.partial[(size_t)cmine * u.P4 + p] : 0.0f;
        const float mine_s = cmine < u.chunks ? part_s[(size_t)cmine * u.P4 + p] : 0.0f;
        const int cnt = u.chunks - base < 64 ? u.chunks - base : 64;
        for (int c = 0; c < cnt; ++c) {
            const float x = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine_mu), c));
            const float y = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine_s), c));
            gmu = (base + c == 0) ? x : gmu + x;
            gs = (base + c == 0) ? y : gs + y;
        }
    }
    if (lane != 0) return;
    float mu_new, scale_new;
    pgpe_update_param(u, p, gmu, gs, true, mu_new, scale_new);
}

// k_pgpe_apply and k_perturb_mirrored in one launch, for policies of up to PGPE_FOLD_MAX_P parameters and PGPE_FOLD_MAX_CHUNKS
// chunks (k_es_apply_perturb's form): EVERY workgroup forms the whole new mean and scale itself -- a thread per parameter, the
// chunk partials added in ascending order, pgpe_update_param -- into LDS and draws its pairs from there; workgroup 0 also stores
// the new state.  The same sums in the same order, so the two forms are bit-equal (tuning knob "pgpe_fused_apply_perturb").
constexpr int PGPE_FOLD_MAX_P = 1024;
constexpr int PGPE_FOLD_MAX_CHUNKS = 16;
__global__ __launch_bounds__(256) void k_pgpe_apply_perturb(PgpeUpdate u, float next_sigma, uint64_t seed, uint64_t gen,
                                                            long long first_row, int n_rows, int quads, float *__restrict__ theta,
                                                            unsigned long long *__restrict__ stamp,
                                                            int32_t *__restrict__ rank_to_clear, int n_clear)
{
    __shared__ float mu_new[PGPE_FOLD_MAX_P];
    __shared__ float sig_new[PGPE_FOLD_MAX_P];
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (stamp && t == 0) *stamp = real_time();
    const float *part_s = u.partial + (size_t)u.chunks * u.P4;
    for (int p = threadIdx.x; p < u.P; p += 256) {
        float gmu = u.partial[p], gs = part_s[p];
        for (int c = 1; c < u.chunks; ++c) {
            gmu = gmu + u.partial[(size_t)c * u.P4 + p];
            gs = gs + part_s[(size_t)c * u.P4 + p];
        }
        float mn, sn;
        pgpe_update_param(u, p, gmu, gs, blockIdx.x == 0, mn, sn);
        mu_new[p] = mn;
        sig_new[p] = __fmul_rn(next_sigma, sn);
    }
    for (long long i = t; i < n_clear; i += (long long)gridDim.x * blockDim.x) rank_to_clear[i] = 0;
    __syncthreads();
    const long long pair0 = first_row >> 1;
    const long long pairs = ((first_row + n_rows - 1) >> 1) - pair0 + 1;
    if (t >= pairs * quads) return;
    const long long jl = t / quads;
    const int q = (int)(t - jl * quads);
    const long long j = pair0 + jl;
    const int lim = u.P - 4 * q < 4 ? u.P - 4 * q : 4;
    float z[4];
    normal4(seed, gen, (uint32_t)j, (uint32_t)q, z);
    const long long even = 2 * j - first_row, odd = even + 1;
    const bool has_even = even >= 0, has_odd = odd < n_rows;
    float *dst_even = theta + (size_t)(has_even ? even : 0) * u.P + 4 * q;
    float *dst_odd = theta + (size_t)(has_odd ? odd : 0) * u.P + 4 * q;
    for (int l = 0; l < lim; ++l) {
        const float center = mu_new[4 * q + l];
        const float d = __fmul_rn(sig_new[4 * q + l], z[l]);
        if (has_even) dst_even[l] = __fadd_rn(center, d);
        if (has_odd) dst_odd[l] = __fsub_rn(center, d);
    }
}

static void launch_perturb_mirrored(ses_handle *h, const float *mu, const float *scale, float sigma, uint64_t seed, uint64_t gen,
                                    long long first_row, int n_rows, float *theta, int32_t *rank_to_clear, int n_clear)
{
    const int quads = (h->P + 3) / 4;
    const long long pairs = n_rows > 0 ? ((first_row + n_rows - 1) >> 1) - (first_row >> 1) + 1 : 1;
    hipLaunchKernelGGL(k_perturb_mirrored, dim3(ceil_div(pairs * quads, 256)), dim3(256), 0, h->stream, mu, scale, sigma, seed, gen,
                       first_row, n_rows, h->P, quads, theta, h->stamp, rank_to_clear, n_clear);
}

}  // namespace ses

extern "C" {

using namespace ses;

int ses_perturb_mirrored(ses_handle *h, const float *mu, const float *scale, float sigma, uint64_t seed, uint64_t gen,
                         int64_t first_row, int32_t n_rows, float *theta)
{
    SES_REQUIRE(h && mu && scale && theta, "ses_perturb_mirrored: null argument");
    SES_REQUIRE(n_rows >= 1 && first_row >= 0 && first_row + n_rows <= (1ll << 30), "ses_perturb_mirrored: row range");
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    launch_perturb_mirrored(h, mu, scale, sigma, seed, gen, (long long)first_row, n_rows, theta, nullptr, 0);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int ses_pgpe_generation(ses_handle *h, const float *fitness, int32_t n, uint64_t seed, uint64_t gen, double sigma, double adam_a,
                        double sigma_learning_rate, double sigma_max_change, float scale_lo, float scale_hi, const float *mu_in,
                        const float *m_in, const float *v_in, const float *scale_in, float *mu_out, float *m_out, float *v_out,
                        float *scale_out, float next_sigma, uint64_t next_gen, int64_t first_row, int32_t n_rows,
                        float *theta_next, float *best, float *gmu_out, float *gs_out)
{
    SES_REQUIRE(h && fitness && mu_in && m_in && v_in && scale_in && mu_out && m_out && v_out && scale_out,
                "ses_pgpe_generation: null argument");
    SES_REQUIRE(mu_in != mu_out && m_in != m_out && v_in != v_out && scale_in != scale_out,
                "ses_pgpe_generation: in and out vectors must be distinct buffers");
    int rc = tail_check_rows("ses_pgpe_generation", n, true, first_row, n_rows, theta_next);
    if (rc != SES_OK) return rc;
    SES_REQUIRE(sigma_max_change >= 0.0 && sigma_max_change < 1.0 && scale_lo > 0.0f && scale_lo <= scale_hi,
                "ses_pgpe_generation: bad sigma_max_change / scale limits");
    const int quads = (h->P + 3) / 4, P4 = 4 * quads;
    const int pairs = n / 2;
    const int chunks = ceil_div(pairs, PGPE_CHUNK);
    // behind the rank vector: the chunk partials of Gmu, then of Gs
    int32_t *rank;
    float *partial;
    rc = tail_rank_begin(h, fitness, n, sizeof(float) * 2 * (size_t)chunks * P4, &rank, (void **)&partial);
    if (rc != SES_OK) return rc;
    hipLaunchKernelGGL(k_pgpe_grad_partial, dim3(quads, chunks), dim3(256), 0, h->stream, rank, fitness, n, seed, gen, P4, chunks,
                       partial, best);
    const PgpeUpdate u{partial, chunks, h->P, P4, (float)sigma, (float)(-1.0 / (double)pairs), adam_a,
                       (float)(sigma_learning_rate / (double)pairs), (float)(1.0 - sigma_max_change), (float)(1.0 + sigma_max_change),
                       scale_lo, scale_hi, mu_in, m_in, v_in, scale_in, mu_out, m_out, v_out, scale_out, gmu_out, gs_out};
    if (h->tune.pgpe_fused_apply_perturb && h->P <= PGPE_FOLD_MAX_P && chunks <= PGPE_FOLD_MAX_CHUNKS && n_rows > 0) {
        // the update inside the launch that draws the next population; it also clears the rank vector
        const long long npairs = ((first_row + n_rows - 1) >> 1) - (first_row >> 1) + 1;
        hipLaunchKernelGGL(k_pgpe_apply_perturb, dim3(ceil_div(npairs * quads, 256)), dim3(256), 0, h->stream, u, next_sigma, seed,
                           next_gen, (long long)first_row, n_rows, quads, theta_next, h->stamp, rank, n);
    } else {
        hipLaunchKernelGGL(k_pgpe_apply, dim3(ceil_div(h->P, 4)), dim3(256), 0, h->stream, u);
        // the next population from the new (mu, scale); the launch also clears the rank vector for the next generation
        launch_perturb_mirrored(h, mu_out, scale_out, next_sigma, seed, next_gen, (long long)first_row, n_rows, theta_next, rank, n);
    }
    SES_HIP_TRY(hipGetLastError());
    tail_rank_cleared(h, rank, n);
    return SES_OK;
}

}  // extern "C"
