// ses_sepcma.hip -- the sep_cma_es strategy: CMA-ES with a diagonal covariance (Ros & Hansen 2008, "A simple modification in
// CMA-ES achieving linear time and space complexity") and cumulative step-size adaptation whose scalar lives on the device.
// No reference counterpart: a fifth strategy with the shape of the openai_es / pgpe tail.
//
//   population  n rows:  theta[i] = mu + ((sigma * step) * sqrt(C[p])) * z(seed, gen, row = i, p)
//   tail        rank -> weighted sums (chunk partials of Sz, Szz over the mu best rows) -> update of (mu, C, p_sigma, p_c, step)
//               in ONE workgroup (the update of every parameter needs |p_sigma'|^2, a sum over all of P) -> next population
//
// Summation order of Sz[p] / Szz[p] (depends on n only): chunks of SEPCMA_CHUNK = 1024 rows; inside a chunk thread c of 256 takes
// rows c, c + 256, c + 512, c + 768 in ascending order (an fma chain; a row of rank >= mu is skipped and draws nothing), an
// 8-level LDS tree combines the 256 threads (s = 128, 64, ..., 1: x[c] += x[c + s]), the chunk partials are added in ascending
// chunk order.  Order of norm2 = sum_p (double)p_sigma'[p]^2: thread c of 1024 adds the squares of p = c, c + 1024, ... in
// ascending order to 0.0, a 10-level LDS tree combines the 1024 threads (s = 512, ..., 1: x[c] += x[c + s]).  No workgroup waits
// for another inside a kernel.
#include <cmath>

#include "ses_internal.h"
#include "ses_math.h"
#include "ses_rng.h"
#include "ses_tail.h"

namespace ses {

constexpr int SEPCMA_UPDATE_THREADS = 1024;  // the one workgroup of the update

// ---- perturbation --------------------------------------------------------------------------------------------------------
// one thread = one Philox call = 4 consecutive parameters of one row.  Rows are global.  One rounding per operation (no fma,
// sqrt correctly rounded): a float32 restatement in numpy is bit-exact.  step is read from device memory: the update kernel of
// the same stream wrote it.
__global__ __launch_bounds__(256) void k_perturb_sepcma(const float *__restrict__ mu, const float *__restrict__ C,
                                                        const float *__restrict__ step, float sigma, uint64_t seed, uint64_t gen,
                                                        long long first_row, int n_rows, int P, int quads,
                                                        float *__restrict__ theta, unsigned long long *__restrict__ stamp,
                                                        int32_t *__restrict__ rank_to_clear, int n_clear)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (stamp && t == 0) *stamp = real_time();                           // ses_set_stamp: the next population is being written
    // the rank vector has been consumed by the sums kernel: leave it zeroed for the next generation's count
    for (long long i = t; i < n_clear; i += (long long)gridDim.x * blockDim.x) rank_to_clear[i] = 0;
    if (n_rows <= 0 || t >= (long long)n_rows * quads) return;
    const long long il = t / quads;
    const int q = (int)(t - il * quads);
    const int lim = P - 4 * q < 4 ? P - 4 * q : 4;
    const float s0 = __fmul_rn(sigma, step[0]);
    float z[4];
    normal4(seed, gen, (uint32_t)(first_row + il), (uint32_t)q, z);
    float *dst = theta + (size_t)il * P + 4 * q;
    for (int l = 0; l < lim; ++l) {
        const float sd = __fmul_rn(s0, __builtin_sqrtf(C[4 * q + l]));
        dst[l] = __fadd_rn(mu[4 * q + l], __fmul_rn(sd, z[l]));
    }
}

// ---- weighted sums -------------------------------------------------------------------------------------------------------
// One 256-thread workgroup per (parameter quad, chunk of SEPCMA_CHUNK rows).  w = weights[rank] for rank < mu; the other rows
// are skipped.  Eight float32 accumulators per thread (4 parameters x {Sz, Szz}):
//     Sz[p] = fma(w, z, Sz[p])        Szz[p] = fma(w, fl(z z), Szz[p])
// an LDS tree over the 256 threads and one partial per chunk: partial[(half * chunks + chunk) * P4 + p], half 0 = Sz, 1 = Szz.
// The thread that meets rank 0 reports best = max(fitness).
__global__ __launch_bounds__(256) void k_sepcma_sums_partial(const int32_t *__restrict__ rank, const float *__restrict__ fitness,
                                                             int n, int mu, const float *__restrict__ weights, uint64_t seed,
                                                             uint64_t gen, int P4, int chunks, float *__restrict__ partial,
                                                             float *__restrict__ best)
{
    __shared__ float red[8][256];
    const int q = blockIdx.x;
    const int row0 = blockIdx.y * SEPCMA_CHUNK;
    const int row1 = row0 + SEPCMA_CHUNK < n ? row0 + SEPCMA_CHUNK : n;
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = row0 + threadIdx.x; i < row1; i += 256) {
        const int r = rank[i];
        if (r == 0 && q == 0 && best) *best = fitness[i];               // max(rewards)
        if (r >= mu) continue;
        const float w = weights[r];
        float z[4];
        normal4(seed, gen, (uint32_t)i, (uint32_t)q, z);
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            acc[l] = fma_(w, z[l], acc[l]);
            acc[4 + l] = fma_(w, __fmul_rn(z[l], z[l]), acc[4 + l]);
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

// ---- update --------------------------------------------------------------------------------------------------------------
// What the update of one generation is given: the chunk partials, the constants (formed on the host in double, cast once), the
// vectors it reads and writes.
struct SepcmaUpdate {
    const float *partial;
    int chunks, P, P4;
    float sigma;                       // the curr_sigma the evaluated population was drawn with
    float a_s, b_s, a_c, hb1, c1f, cmuf, k0_h1, k0_h0, var_lo, var_hi, step_lo, step_hi;
    double hsig_scale, hsig_thr, cs_over_ds, chi;
    const float *mu, *C, *ps, *pc, *step;
    float *mu_out, *C_out, *ps_out, *pc_out, *step_out, *sums;   // sums: scratch [2 * P4], Sz then Szz
    float *sz_out, *szz_out;
    double *norm2_out;
};

// ONE workgroup of SEPCMA_UPDATE_THREADS threads.  First loop over p (stride 1024): the chunk partials added in ascending order,
// p_sigma' written, its square added in double.  Block tree for norm2.  Thread 0: the scalar path in double, (h, step') into LDS.
// Second loop: p_c', mu', C' (each thread revisits the parameters whose sums it formed, so the scratch needs no fence).
__global__ __launch_bounds__(SEPCMA_UPDATE_THREADS) void k_sepcma_update(SepcmaUpdate u)
{
    __shared__ double red[SEPCMA_UPDATE_THREADS];
    __shared__ int h_sh;
    const int c = threadIdx.x;
    const float *part_zz = u.partial + (size_t)u.chunks * u.P4;
    double acc = 0.0;
    for (int p = c; p < u.P; p += SEPCMA_UPDATE_THREADS) {
        float sz = u.partial[p], szz = part_zz[p];
        for (int k = 1; k < u.chunks; ++k) {
            sz = sz + u.partial[(size_t)k * u.P4 + p];
            szz = szz + part_zz[(size_t)k * u.P4 + p];
        }
        u.sums[p] = sz;
        u.sums[u.P4 + p] = szz;
        if (u.sz_out) u.sz_out[p] = sz;
        if (u.szz_out) u.szz_out[p] = szz;
        const float psn = __fadd_rn(__fmul_rn(u.a_s, u.ps[p]), __fmul_rn(u.b_s, sz));
        u.ps_out[p] = psn;
        acc = acc + (double)psn * (double)psn;                            // the square is exact in double
    }
    red[c] = acc;
    __syncthreads();
    for (int s = SEPCMA_UPDATE_THREADS / 2; s > 0; s >>= 1) {
        if (c < s) red[c] = red[c] + red[c + s];
        __syncthreads();
    }
    const float step_old = u.step[0];
    if (c == 0) {
        const double norm2 = red[0];
        const double nrm = sqrt(norm2);
        h_sh = nrm * u.hsig_scale < u.hsig_thr ? 1 : 0;
        double e = u.cs_over_ds * (nrm / u.chi - 1.0);
        if (e > 1.0) e = 1.0;
        const float sn = (float)((double)step_old * exp(e));
        u.step_out[0] = fminf(fmaxf(sn, u.step_lo), u.step_hi);
        if (u.norm2_out) u.norm2_out[0] = norm2;
    }
    __syncthreads();
    const bool h = h_sh != 0;
    const float hb = h ? u.hb1 : 0.0f;
    const float k0 = h ? u.k0_h1 : u.k0_h0;
    const float s0 = __fmul_rn(u.sigma, step_old);
    for (int p = c; p < u.P; p += SEPCMA_UPDATE_THREADS) {
        const float sz = u.sums[p], szz = u.sums[u.P4 + p];
        const float Cv = u.C[p];
        const float sC = __builtin_sqrtf(Cv);
        const float y = __fmul_rn(sC, sz);
        const float pcn = __fadd_rn(__fmul_rn(u.a_c, u.pc[p]), __fmul_rn(hb, y));
        const float sd = __fmul_rn(s0, sC);
        u.pc_out[p] = pcn;
        u.mu_out[p] = __fadd_rn(u.mu[p], __fmul_rn(sd, sz));
        const float cn = __fadd_rn(__fadd_rn(__fmul_rn(k0, Cv), __fmul_rn(u.c1f, __fmul_rn(pcn, pcn))),
                                   __fmul_rn(u.cmuf, __fmul_rn(Cv, szz)));
        u.C_out[p] = fminf(fmaxf(cn, u.var_lo), u.var_hi);
    }
}

static void launch_perturb_sepcma(ses_handle *h, const float *mu, const float *C, const float *step, float sigma, uint64_t seed,
                                  uint64_t gen, long long first_row, int n_rows, float *theta, int32_t *rank_to_clear, int n_clear)
{
    const int quads = (h->P + 3) / 4;
    const long long threads = n_rows > 0 ? (long long)n_rows * quads : 1;
    hipLaunchKernelGGL(k_perturb_sepcma, dim3(ceil_div(threads, 256)), dim3(256), 0, h->stream, mu, C, step, sigma, seed, gen,
                       first_row, n_rows, h->P, quads, theta, h->stamp, rank_to_clear, n_clear);
}

}  // namespace ses

extern "C" {

using namespace ses;

int ses_perturb_sepcma(ses_handle *h, const float *mu, const float *C, const float *step, float sigma, uint64_t seed, uint64_t gen,
                       int64_t first_row, int32_t n_rows, float *theta)
{
    SES_REQUIRE(h && mu && C && step && theta, "ses_perturb_sepcma: null argument");
    SES_REQUIRE(n_rows >= 1 && first_row >= 0 && first_row + n_rows <= (1ll << 30), "ses_perturb_sepcma: row range");
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    launch_perturb_sepcma(h, mu, C, step, sigma, seed, gen, (long long)first_row, n_rows, theta, nullptr, 0);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int ses_sepcma_generation(ses_handle *h, const float *fitness, int32_t n, uint64_t seed, uint64_t gen, double sigma, double hsig_scale,
                          const ses_sepcma_params *p, const float *weights, const float *mu_in, const float *C_in,
                          const float *ps_in, const float *pc_in, const float *step_in, float *mu_out, float *C_out, float *ps_out,
                          float *pc_out, float *step_out, float next_sigma, uint64_t next_gen, int64_t first_row, int32_t n_rows,
                          float *theta_next, float *best, float *sz_out, float *szz_out, double *norm2_out)
{
    SES_REQUIRE(h && fitness && p && weights && mu_in && C_in && ps_in && pc_in && step_in && mu_out && C_out && ps_out && pc_out &&
                    step_out, "ses_sepcma_generation: null argument");
    SES_REQUIRE(mu_in != mu_out && C_in != C_out && ps_in != ps_out && pc_in != pc_out && step_in != step_out,
                "ses_sepcma_generation: in and out vectors must be distinct buffers");
    int rc = tail_check_rows("ses_sepcma_generation", n, false, first_row, n_rows, theta_next);
    if (rc != SES_OK) return rc;
    SES_REQUIRE(p->mu >= 1 && p->mu <= n, "ses_sepcma_generation: mu = %d outside [1, %d]", p->mu, n);
    SES_REQUIRE(p->scale_lo > 0.0f && p->scale_lo <= p->scale_hi && p->step_lo > 0.0f && p->step_lo <= p->step_hi,
                "ses_sepcma_generation: bad scale / step limits");
    SES_REQUIRE(p->mueff >= 1.0 && p->c_sigma > 0.0 && p->c_sigma < 1.0 && p->d_sigma > 0.0 && p->c_c > 0.0 && p->c_c <= 1.0 &&
                    p->c_1 >= 0.0 && p->c_mu >= 0.0 && p->c_1 + p->c_mu <= 1.0 && p->chi > 0.0 && hsig_scale > 0.0,
                "ses_sepcma_generation: constants out of range");
    const int quads = (h->P + 3) / 4, P4 = 4 * quads;
    const int chunks = ceil_div(n, SEPCMA_CHUNK);
    // behind the rank vector: the chunk partials of Sz, then of Szz | Sz, Szz
    int32_t *rank;
    float *partial;
    rc = tail_rank_begin(h, fitness, n, sizeof(float) * 2 * (size_t)(chunks + 1) * P4, &rank, (void **)&partial);
    if (rc != SES_OK) return rc;
    float *sums = partial + 2 * (size_t)chunks * P4;
    hipLaunchKernelGGL(k_sepcma_sums_partial, dim3(quads, chunks), dim3(256), 0, h->stream, rank, fitness, n, p->mu, weights, seed, gen,
                       P4, chunks, partial, best);
    const double P = (double)h->P;
    SepcmaUpdate u;
    u.partial = partial; u.chunks = chunks; u.P = h->P; u.P4 = P4;
    u.sigma = (float)sigma;
    u.a_s = (float)(1.0 - p->c_sigma);
    u.b_s = (float)std::sqrt(p->c_sigma * (2.0 - p->c_sigma) * p->mueff);
    u.a_c = (float)(1.0 - p->c_c);
    u.hb1 = (float)std::sqrt(p->c_c * (2.0 - p->c_c) * p->mueff);
    u.c1f = (float)p->c_1;
    u.cmuf = (float)p->c_mu;
    u.k0_h1 = (float)(1.0 - p->c_1 - p->c_mu + 0.0);
    u.k0_h0 = (float)(1.0 - p->c_1 - p->c_mu + p->c_1 * p->c_c * (2.0 - p->c_c));
    u.var_lo = p->scale_lo * p->scale_lo;           // float32 products (-ffp-contract=off)
    u.var_hi = p->scale_hi * p->scale_hi;
    u.step_lo = p->step_lo; u.step_hi = p->step_hi;
    u.hsig_scale = hsig_scale;
    u.hsig_thr = (1.4 + 2.0 / (P + 1.0)) * p->chi;
    u.cs_over_ds = p->c_sigma / p->d_sigma;
    u.chi = p->chi;
    u.mu = mu_in; u.C = C_in; u.ps = ps_in; u.pc = pc_in; u.step = step_in;
    u.mu_out = mu_out; u.C_out = C_out; u.ps_out = ps_out; u.pc_out = pc_out; u.step_out = step_out; u.sums = sums;
    u.sz_out = sz_out; u.szz_out = szz_out; u.norm2_out = norm2_out;
    hipLaunchKernelGGL(k_sepcma_update, dim3(1), dim3(SEPCMA_UPDATE_THREADS), 0, h->stream, u);
    // the next population from the new (mu, C, step); the launch also clears the rank vector for the next generation
    launch_perturb_sepcma(h, mu_out, C_out, step_out, next_sigma, seed, next_gen, (long long)first_row, n_rows, theta_next, rank, n);
    SES_HIP_TRY(hipGetLastError());
    tail_rank_cleared(h, rank, n);
    return SES_OK;
}

}  // extern "C"
