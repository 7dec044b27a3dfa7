// ses_lmma.hip -- the lm_ma_es strategy: limited-memory matrix adaptation ES (Loshchilov, Glasmachers & Beyer 2019, "Large scale
// black-box optimization by limited-memory matrix adaptation") with cumulative step-size adaptation whose scalar lives on the
// device.  No reference counterpart: a sixth strategy with the shape of the pgpe / sep_cma_es tail.
//
//   population  n rows:  v_0 = z(seed, gen, row = i);  v_{j+1} = ad[j] v_j + (cd[j] <M_j, v_j>) M_j, j < m_active;
//               theta[i] = mu + (sigma * step) v_last -- a chain of m_active DEPENDENT workgroup-wide dot products per row
//   tail        rank -> weighted sums (k_sepcma_sums_partial as it is: the chunk partials of Sz; its Szz half is not read) ->
//               update of (mu, p_sigma, M, step) in ONE workgroup -> next population
//
// Order of a row's dot <M_j, v_j> (k_perturb_lmma; depends on P only).  The row is held by T threads, T = 64 for P <= 256 and 256
// above; thread c owns the parameter quads q = c, c + T, c + 2T, ... (parameters 4q .. 4q + 3, what one Philox call draws).
//   1. four fma chains per thread, one per position l = 0..3 inside a quad, each over the thread's quads in ascending order:
//      a_l = fma(M[4q + l], v[4q + l], a_l) from +0;
//   2. x = (a_0 + a_1) + (a_2 + a_3);
//   3. a butterfly over the 64 lanes of the wave: x[lane] = x[lane] + x[lane ^ s], s = 32, 16, 8, 4, 2, 1 (every lane ends with
//      the same bits: the addition is commutative);
//   4. T = 256 only: the four wave sums w[0..3] go through LDS (ONE barrier per dot: the slots are double-buffered), every lane
//      takes y = w[lane & 3] and y[lane] = y[lane] + y[lane ^ s], s = 2, 1: (w0 + w2) + (w1 + w3) up to commutation.
// Order of the update's dot <M_j, u_j> (k_lmma_update, 1024 threads): thread c takes p = c, c + 1024, ... in ascending order as
// ONE fma chain from +0, the same 64-lane butterfly, the 16 wave sums through LDS, y = w[lane & 15] and a butterfly s = 8, 4, 2, 1.
// Sz and norm2 are summed in ses_sepcma.hip's orders.  No workgroup waits for another inside a kernel.
#include <cmath>

#include "ses_internal.h"
#include "ses_math.h"
#include "ses_rng.h"
#include "ses_tail.h"

namespace ses {

constexpr int LMMA_MAX_M = 32;               // direction vectors (SES_LMMA_MAX_MEMORY)
constexpr int LMMA_MAX_P = 16384;            // parameters a row's workgroup / the update's workgroup holds in registers (SES_LMMA_MAX_P)
constexpr int LMMA_UPDATE_THREADS = 1024;    // the one workgroup of the update
constexpr int LMMA_UPDATE_ROUNDS = LMMA_MAX_P / LMMA_UPDATE_THREADS;

// rows of M and of theta start at multiples of P floats: 4-byte alignment is all a quad's address has
typedef float lmma_f4 __attribute__((ext_vector_type(4), aligned(4)));

// x[lane] + x[lane ^ s] for s = WIDTH / 2 ... 1: the sum over each aligned group of WIDTH lanes, the same bits in every lane
template <int WIDTH>
__device__ __forceinline__ float lane_butterfly(float x)
{
#pragma unroll
    for (int s = WIDTH / 2; s > 0; s >>= 1) x = x + __shfl_xor(x, s, 64);
    return x;
}

// ---- perturbation --------------------------------------------------------------------------------------------------------
struct LmmaPerturb {
    const float *mu, *M, *step;
    float sigma;
    int n_rows, P, quads, m_active;
    uint64_t seed, gen;
    long long first_row;
    float *theta, *dots_out;
    unsigned long long *stamp;
    int32_t *rank_to_clear;
    int n_clear;
    float cd[LMMA_MAX_M], ad[LMMA_MAX_M];
};

// the thread's quads of row j of M; zero outside [0, P): such a position adds nothing to a dot
template <int T, int QR>
__device__ __forceinline__ void lmma_load_row(const float *__restrict__ Mj, int P, int quads, int c, float (&dst)[QR][4])
{
#pragma unroll
    for (int r = 0; r < QR; ++r) {
        const int q = c + r * T;
        if (4 * q + 4 <= P) {
            const lmma_f4 x = *(const lmma_f4 *)(Mj + 4 * q);
            dst[r][0] = x.x; dst[r][1] = x.y; dst[r][2] = x.z; dst[r][3] = x.w;
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l) dst[r][l] = (q < quads && 4 * q + l < P) ? Mj[4 * q + l] : 0.0f;
        }
    }
}

// One workgroup of T threads = one row; QR = quads per thread the registers hold (T * QR * 4 >= P).  v stays in registers across
// the chain, M streams from L2 (the next vector's loads are issued before the current dot's reduction is waited for).  Rows are
// global.  One rounding per operation outside the dots (no fma there): a float32 restatement in numpy that is given the dots is
// bit-exact.  step is read from device memory: the update kernel of the same stream wrote it.
template <int T, int QR>
__global__ __launch_bounds__(T) void k_perturb_lmma(LmmaPerturb a)
{
    constexpr int W = T / 64;
    __shared__ float part[2][W];
    const int c = threadIdx.x;
    if (a.stamp && blockIdx.x == 0 && c == 0) *a.stamp = real_time();   // ses_set_stamp: the next population is being written
    // the rank vector has been consumed by the sums kernel: leave it zeroed for the next generation's count
    for (long long i = (long long)blockIdx.x * T + c; i < a.n_clear; i += (long long)gridDim.x * T) a.rank_to_clear[i] = 0;
    const long long il = blockIdx.x;
    if (il >= a.n_rows) return;                                         // (the whole workgroup: no barrier is left behind)
    const int P = a.P, quads = a.quads;
    const float s0 = __fmul_rn(a.sigma, a.step[0]);
    float v[QR][4], Mc[QR][4], Mn[QR][4];
#pragma unroll
    for (int r = 0; r < QR; ++r) {
        const int q = c + r * T;
        if (q < quads) {
            normal4(a.seed, a.gen, (uint32_t)(a.first_row + il), (uint32_t)q, v[r]);
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l) v[r][l] = 0.0f;
        }
    }
    if (a.m_active > 0) lmma_load_row<T, QR>(a.M, P, quads, c, Mc);
    for (int j = 0; j < a.m_active; ++j) {
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int r = 0; r < QR; ++r) {
#pragma unroll
            for (int l = 0; l < 4; ++l) acc[l] = fma_(Mc[r][l], v[r][l], acc[l]);
        }
        if (j + 1 < a.m_active) lmma_load_row<T, QR>(a.M + (size_t)(j + 1) * P, P, quads, c, Mn);
        float dot = lane_butterfly<64>((acc[0] + acc[1]) + (acc[2] + acc[3]));
        if (W > 1) {
            if ((c & 63) == 0) part[j & 1][c >> 6] = dot;
            __syncthreads();                                            // the only barrier of this dot: dot j + 1 uses the other slots
            dot = lane_butterfly<W>(part[j & 1][c & (W - 1)]);
        }
        if (c == 0 && a.dots_out) a.dots_out[il * a.m_active + j] = dot;
        const float g = __fmul_rn(a.cd[j], dot), ad = a.ad[j];
#pragma unroll
        for (int r = 0; r < QR; ++r) {
#pragma unroll
            for (int l = 0; l < 4; ++l) v[r][l] = __fadd_rn(__fmul_rn(ad, v[r][l]), __fmul_rn(g, Mc[r][l]));
        }
        if (j + 1 < a.m_active) {
#pragma unroll
            for (int r = 0; r < QR; ++r) {
#pragma unroll
                for (int l = 0; l < 4; ++l) Mc[r][l] = Mn[r][l];
            }
        }
    }
    float *dst = a.theta + (size_t)il * P;
#pragma unroll
    for (int r = 0; r < QR; ++r) {
        const int q = c + r * T;
        if (4 * q + 4 <= P) {
            const lmma_f4 m4 = *(const lmma_f4 *)(a.mu + 4 * q);
            lmma_f4 o;
            o.x = __fadd_rn(m4.x, __fmul_rn(s0, v[r][0]));
            o.y = __fadd_rn(m4.y, __fmul_rn(s0, v[r][1]));
            o.z = __fadd_rn(m4.z, __fmul_rn(s0, v[r][2]));
            o.w = __fadd_rn(m4.w, __fmul_rn(s0, v[r][3]));
            *(lmma_f4 *)(dst + 4 * q) = o;
        } else if (q < quads) {
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (4 * q + l < P) dst[4 * q + l] = __fadd_rn(a.mu[4 * q + l], __fmul_rn(s0, v[r][l]));
        }
    }
}

// ---- update --------------------------------------------------------------------------------------------------------------
struct LmmaUpdate {
    const float *partial;              // the Sz half of k_sepcma_sums_partial's chunk partials
    int chunks, P, P4, m, m_active;
    float sigma;                       // the curr_sigma the evaluated population was drawn with
    float a_s, b_s, step_lo, step_hi;
    double cs_over_ds, chi;
    const float *mu, *ps, *M, *step;
    float *mu_out, *ps_out, *M_out, *step_out;
    float *sz_out, *sd_out, *sdots_out;
    double *norm2_out;
    float cd[LMMA_MAX_M], ad[LMMA_MAX_M], ac[LMMA_MAX_M], bc[LMMA_MAX_M];
};

// ONE workgroup of LMMA_UPDATE_THREADS threads; thread c owns the parameters p = c, c + 1024, ... and keeps their Sz and u in
// registers.  Chunk partials added in ascending order, p_sigma' written, its square added in double; block tree for norm2; thread
// 0: the scalar path in double.  Then the chain of the transform on u_0 = Sz with the OLD vectors (M'[j] is written as M[j] passes
// through the registers), mu', and M'[j] of the vectors the chain did not visit.
__global__ __launch_bounds__(LMMA_UPDATE_THREADS) void k_lmma_update(LmmaUpdate u)
{
    __shared__ double red[LMMA_UPDATE_THREADS];
    __shared__ float part[2][LMMA_UPDATE_THREADS / 64];
    const int c = threadIdx.x;
    float sz[LMMA_UPDATE_ROUNDS], uv[LMMA_UPDATE_ROUNDS], Mc[LMMA_UPDATE_ROUNDS];
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < LMMA_UPDATE_ROUNDS; ++r) {
        const int p = c + r * LMMA_UPDATE_THREADS;
        sz[r] = 0.0f;
        if (p < u.P) {
            float s = u.partial[p];
            for (int k = 1; k < u.chunks; ++k) s = s + u.partial[(size_t)k * u.P4 + p];
            sz[r] = s;
            if (u.sz_out) u.sz_out[p] = s;
            const float psn = __fadd_rn(__fmul_rn(u.a_s, u.ps[p]), __fmul_rn(u.b_s, s));
            u.ps_out[p] = psn;
            acc = acc + (double)psn * (double)psn;                        // the square is exact in double
        }
        uv[r] = sz[r];
    }
    red[c] = acc;
    __syncthreads();
    for (int s = LMMA_UPDATE_THREADS / 2; s > 0; s >>= 1) {
        if (c < s) red[c] = red[c] + red[c + s];
        __syncthreads();
    }
    const float step_old = u.step[0];
    if (c == 0) {
        const double norm2 = red[0];
        double e = u.cs_over_ds * (sqrt(norm2) / u.chi - 1.0);
        if (e > 1.0) e = 1.0;
        const float sn = (float)((double)step_old * exp(e));
        u.step_out[0] = fminf(fmaxf(sn, u.step_lo), u.step_hi);
        if (u.norm2_out) u.norm2_out[0] = norm2;
    }
    const float s0 = __fmul_rn(u.sigma, step_old);
    for (int j = 0; j < u.m; ++j) {
        const float *Mj = u.M + (size_t)j * u.P;
        float *Mo = u.M_out + (size_t)j * u.P;
        const float acj = u.ac[j], bcj = u.bc[j];
        float chain = 0.0f;
#pragma unroll
        for (int r = 0; r < LMMA_UPDATE_ROUNDS; ++r) {
            const int p = c + r * LMMA_UPDATE_THREADS;
            Mc[r] = 0.0f;
            if (p < u.P) {
                Mc[r] = Mj[p];
                Mo[p] = __fadd_rn(__fmul_rn(acj, Mc[r]), __fmul_rn(bcj, sz[r]));
            }
            chain = fma_(Mc[r], uv[r], chain);
        }
        if (j >= u.m_active) continue;                                   // (uniform: every thread sees the same j and m_active)
        float dot = lane_butterfly<64>(chain);
        if ((c & 63) == 0) part[j & 1][c >> 6] = dot;
        __syncthreads();                                                // one barrier per dot: dot j + 1 uses the other slots
        dot = lane_butterfly<16>(part[j & 1][c & 15]);
        if (c == 0 && u.sdots_out) u.sdots_out[j] = dot;
        const float g = __fmul_rn(u.cd[j], dot), ad = u.ad[j];
#pragma unroll
        for (int r = 0; r < LMMA_UPDATE_ROUNDS; ++r) uv[r] = __fadd_rn(__fmul_rn(ad, uv[r]), __fmul_rn(g, Mc[r]));
    }
#pragma unroll
    for (int r = 0; r < LMMA_UPDATE_ROUNDS; ++r) {
        const int p = c + r * LMMA_UPDATE_THREADS;
        if (p < u.P) {
            u.mu_out[p] = __fadd_rn(u.mu[p], __fmul_rn(s0, uv[r]));
            if (u.sd_out) u.sd_out[p] = uv[r];
        }
    }
}

static int launch_perturb_lmma(ses_handle *h, const float *mu, const float *M, const float *step, const ses_lmma_params *p,
                               int m_active, float sigma, uint64_t seed, uint64_t gen, long long first_row, int n_rows, float *theta,
                               float *dots_out, int32_t *rank_to_clear, int n_clear)
{
    LmmaPerturb a;
    a.mu = mu; a.M = M; a.step = step; a.sigma = sigma;
    a.n_rows = n_rows; a.P = h->P; a.quads = (h->P + 3) / 4; a.m_active = m_active;
    a.seed = seed; a.gen = gen; a.first_row = first_row;
    a.theta = theta; a.dots_out = dots_out; a.stamp = h->stamp; a.rank_to_clear = rank_to_clear; a.n_clear = n_clear;
    for (int j = 0; j < LMMA_MAX_M; ++j) { a.cd[j] = p->cd[j]; a.ad[j] = p->ad[j]; }
    const dim3 grid(n_rows > 0 ? n_rows : 1);
    if (a.quads <= 64) hipLaunchKernelGGL((k_perturb_lmma<64, 1>), grid, dim3(64), 0, h->stream, a);
    else if (a.quads <= 2 * 256) hipLaunchKernelGGL((k_perturb_lmma<256, 2>), grid, dim3(256), 0, h->stream, a);
    else if (a.quads <= 8 * 256) hipLaunchKernelGGL((k_perturb_lmma<256, 8>), grid, dim3(256), 0, h->stream, a);
    else hipLaunchKernelGGL((k_perturb_lmma<256, 16>), grid, dim3(256), 0, h->stream, a);
    return SES_OK;
}

static int lmma_check_params(ses_handle *h, const ses_lmma_params *p, const float *M, int m_active, const char *who)
{
    if (h->P > LMMA_MAX_P)
        return set_error(SES_ERR_UNSUPPORTED, "%s: %d parameters; the lm_ma_es kernels hold at most %d", who, h->P, LMMA_MAX_P);
    SES_REQUIRE(p->m >= 0 && p->m <= LMMA_MAX_M, "%s: memory = %d outside [0, %d]", who, p->m, LMMA_MAX_M);
    SES_REQUIRE(m_active >= 0 && m_active <= p->m, "%s: m_active = %d outside [0, memory = %d]", who, m_active, p->m);
    SES_REQUIRE(p->m == 0 || M, "%s: null direction vectors", who);
    return SES_OK;
}

}  // namespace ses

extern "C" {

using namespace ses;

int ses_perturb_lmma(ses_handle *h, const float *mu, const float *M, const float *step, const ses_lmma_params *p, int32_t m_active,
                     float sigma, uint64_t seed, uint64_t gen, int64_t first_row, int32_t n_rows, float *theta, float *dots_out)
{
    SES_REQUIRE(h && mu && step && p && theta, "ses_perturb_lmma: null argument");
    const int rc = lmma_check_params(h, p, M, m_active, "ses_perturb_lmma");
    if (rc != SES_OK) return rc;
    SES_REQUIRE(n_rows >= 1 && first_row >= 0 && first_row + n_rows <= (1ll << 30), "ses_perturb_lmma: row range");
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    launch_perturb_lmma(h, mu, M, step, p, m_active, sigma, seed, gen, (long long)first_row, n_rows, theta, dots_out, nullptr, 0);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int ses_lmma_generation(ses_handle *h, const float *fitness, int32_t n, uint64_t seed, uint64_t gen, double sigma,
                        const ses_lmma_params *p, const float *weights, int32_t m_active, int32_t m_active_next, const float *mu_in,
                        const float *ps_in, const float *M_in, const float *step_in, float *mu_out, float *ps_out, float *M_out,
                        float *step_out, float next_sigma, uint64_t next_gen, int64_t first_row, int32_t n_rows, float *theta_next,
                        float *best, float *sz_out, float *sd_out, float *sdots_out, double *norm2_out, float *dots_next_out)
{
    SES_REQUIRE(h && fitness && p && weights && mu_in && ps_in && step_in && mu_out && ps_out && step_out,
                "ses_lmma_generation: null argument");
    int rc = lmma_check_params(h, p, M_in, m_active, "ses_lmma_generation");
    if (rc == SES_OK) rc = lmma_check_params(h, p, M_out, m_active_next, "ses_lmma_generation");
    if (rc != SES_OK) return rc;
    SES_REQUIRE(mu_in != mu_out && ps_in != ps_out && step_in != step_out && (p->m == 0 || M_in != M_out),
                "ses_lmma_generation: in and out vectors must be distinct buffers");
    rc = tail_check_rows("ses_lmma_generation", n, false, first_row, n_rows, theta_next);
    if (rc != SES_OK) return rc;
    SES_REQUIRE(p->mu >= 1 && p->mu <= n, "ses_lmma_generation: mu = %d outside [1, %d]", p->mu, n);
    SES_REQUIRE(p->step_lo > 0.0f && p->step_lo <= p->step_hi, "ses_lmma_generation: bad step limits");
    SES_REQUIRE(p->mueff >= 1.0 && p->c_sigma > 0.0 && p->c_sigma < 1.0 && p->d_sigma > 0.0 && p->chi > 0.0,
                "ses_lmma_generation: constants out of range");
    const int quads = (h->P + 3) / 4, P4 = 4 * quads;
    const int chunks = ceil_div(n, SEPCMA_CHUNK);
    // behind the rank vector: the chunk partials of Sz, then of Szz (k_sepcma_sums_partial's layout)
    int32_t *rank;
    float *partial;
    rc = tail_rank_begin(h, fitness, n, sizeof(float) * 2 * (size_t)chunks * P4, &rank, (void **)&partial);
    if (rc != SES_OK) return rc;
    hipLaunchKernelGGL(k_sepcma_sums_partial, dim3(quads, chunks), dim3(256), 0, h->stream, rank, fitness, n, p->mu, weights, seed, gen,
                       P4, chunks, partial, best);
    LmmaUpdate u;
    u.partial = partial; u.chunks = chunks; u.P = h->P; u.P4 = P4; u.m = p->m; u.m_active = m_active;
    u.sigma = (float)sigma;
    u.a_s = (float)(1.0 - p->c_sigma);
    u.b_s = (float)std::sqrt(p->c_sigma * (2.0 - p->c_sigma) * p->mueff);
    u.step_lo = p->step_lo; u.step_hi = p->step_hi;
    u.cs_over_ds = p->c_sigma / p->d_sigma;
    u.chi = p->chi;
    u.mu = mu_in; u.ps = ps_in; u.M = M_in; u.step = step_in;
    u.mu_out = mu_out; u.ps_out = ps_out; u.M_out = M_out; u.step_out = step_out;
    u.sz_out = sz_out; u.sd_out = sd_out; u.sdots_out = sdots_out; u.norm2_out = norm2_out;
    for (int j = 0; j < LMMA_MAX_M; ++j) { u.cd[j] = p->cd[j]; u.ad[j] = p->ad[j]; u.ac[j] = p->ac[j]; u.bc[j] = p->bc[j]; }
    hipLaunchKernelGGL(k_lmma_update, dim3(1), dim3(LMMA_UPDATE_THREADS), 0, h->stream, u);
    // the next population from the new (mu, M, step); the launch also clears the rank vector for the next generation
    launch_perturb_lmma(h, mu_out, M_out, step_out, p, m_active_next, next_sigma, seed, next_gen, (long long)first_row, n_rows,
                        theta_next, dots_next_out, rank, n);
    SES_HIP_TRY(hipGetLastError());
    tail_rank_cleared(h, rank, n);
    return SES_OK;
}

}  // extern "C"
