// ses_batch_sepcma.hip -- the sep_cma_es tail of R independent trials in one set of launches (ses_sepcma_generation_batch).
// The trials of a sweep sit one behind the other at a fixed stride, like the openai_es batch (ses_batch.hip): trial r owns rows
// [r n, (r + 1) n) of the fitness vector and of the next population and row r of the state matrices mu, C, ps, pc [R, P] and
// step [R].  Only the selection is ragged: mu_r = elite_num_r, and with it the weight row and every constant, differ per trial.
// Per trial, bit for bit what ses_sepcma_generation gives for its slice alone -- the orders are those of ses_sepcma.hip's header,
// rows counted from the trial's first row:
//
//   rank        the counting rank of ses_batch.hip (k_batch_rank_count, launched as it is): key = (ordered fitness bits, index
//               WITHIN the trial), -0 as +0
//   sums        chunks of SEPCMA_CHUNK = 1024 rows; thread c of 256 takes rows c, c + 256, c + 512, c + 768 in ascending order (an
//               fma chain; a row of rank >= mu_r is skipped and draws nothing), the 8-level LDS tree, one partial per chunk
//   update      ONE 1024-thread workgroup per trial: the chunk partials in ascending order, p_sigma', norm2 in double with the
//               10-level tree, the scalar path on thread 0 in double, then p_c', mu', C'
//   population  one Philox call per thread for 4 parameters, row = index within the trial, s0 = fl(sigma * step_out[r]), no fma
//
// Four launches whatever R, the trial a grid dimension of each; no launch needs an order between its workgroups: no ticket
// counters, no polling.  The per-generation records, the constants and the weights are read from tables in DEVICE memory the caller
// wrote: no host-to-device copy here.  The library never sees those tables, so the one index a kernel derives from them, mu_r, is
// clamped into [1, n] first: a wrong table gives wrong numbers, never an access outside the caller's buffers.
#include "ses_internal.h"
#include "ses_math.h"
#include "ses_rng.h"
#include "ses_tail.h"

namespace ses {

constexpr int BSEP_UPDATE_THREADS = 1024;     // the one workgroup of a trial's update (SEPCMA_UPDATE_THREADS)
constexpr int BSEP_MAX_N = RANK_SORT_MIN;     // rows per trial: the counting rank only
constexpr long long BSEP_MAX_ROWS = 1ll << 20;

// what the launches are given besides the fitness: the tables, the shape, the state matrices
struct BsepShape {
    const ses_batch_sepcma_trial *trials;     // [R], device
    const ses_batch_sepcma_consts *consts;    // [R], device
    const float *weights;                     // [R, n], device
    int R, n, chunks, P, P4, quads;
    float *partial;                           // scratch [R][2][chunks][P4]: the chunk partials of Sz, then of Szz
    float *sums;                              // scratch [R][2][P4]: Sz, Szz
    const float *mu, *C, *ps, *pc, *step;     // [R, P]; step [R]
    float *mu_out, *C_out, *ps_out, *pc_out, *step_out;
    float *theta;                             // [R n, P]
    unsigned long long *stamp;
    int32_t *rank_to_clear;
    int n_clear;
};

// k_sepcma_sums_partial per trial: grid (R, quads, chunks); the thread that meets the trial's rank 0 reports best[trial]
__global__ __launch_bounds__(256) void k_bsep_sums_partial(BsepShape s, const int32_t *__restrict__ rank_all,
                                                           const float *__restrict__ fit_all, float *__restrict__ best)
{
    __shared__ float red[8][256];
    const int r = blockIdx.x, q = blockIdx.y, chunk = blockIdx.z;
    const uint64_t seed = s.trials[r].seed, gen = s.trials[r].gen;       // uniform
    int mu = s.consts[r].mu;
    mu = mu < 1 ? 1 : (mu > s.n ? s.n : mu);                             // the weight row has n entries
    const int32_t *__restrict__ rank = rank_all + (size_t)r * s.n;
    const float *__restrict__ fitness = fit_all + (size_t)r * s.n;
    const float *__restrict__ weights = s.weights + (size_t)r * s.n;
    const int row0 = chunk * SEPCMA_CHUNK;
    const int row1 = row0 + SEPCMA_CHUNK < s.n ? row0 + SEPCMA_CHUNK : s.n;
    float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = row0 + threadIdx.x; i < row1; i += 256) {
        const int rk = rank[i];
        if (rk == 0 && q == 0 && best) best[r] = fitness[i];            // max(rewards)
        if (rk >= mu) continue;
        const float w = weights[rk];
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
    for (int t = 128; t > 0; t >>= 1) {
        if (threadIdx.x < t) {
#pragma unroll
            for (int l = 0; l < 8; ++l) red[l][threadIdx.x] = red[l][threadIdx.x] + red[l][threadIdx.x + t];
        }
        __syncthreads();
    }
    if (threadIdx.x < 8) {
        const int half = threadIdx.x >> 2, l = threadIdx.x & 3;
        s.partial[(((size_t)r * 2 + half) * s.chunks + chunk) * s.P4 + 4 * q + l] = red[threadIdx.x][0];
    }
}

// k_sepcma_update per trial: grid R, ONE workgroup of BSEP_UPDATE_THREADS threads each.  Every thread revisits in the second loop
// the parameters whose sums it formed in the first, so the scratch needs no fence; the in and out matrices are distinct buffers.
__global__ __launch_bounds__(BSEP_UPDATE_THREADS) void k_bsep_update(BsepShape s)
{
    __shared__ double red[BSEP_UPDATE_THREADS];
    __shared__ int h_sh;
    const int r = blockIdx.x, c = threadIdx.x;
    const ses_batch_sepcma_consts k = s.consts[r];                       // uniform
    const ses_batch_sepcma_trial tr = s.trials[r];
    const float *__restrict__ part_z = s.partial + (size_t)r * 2 * s.chunks * s.P4;
    const float *__restrict__ part_zz = part_z + (size_t)s.chunks * s.P4;
    float *__restrict__ sums = s.sums + (size_t)r * 2 * s.P4;
    const size_t at = (size_t)r * s.P;
    double acc = 0.0;
    for (int p = c; p < s.P; p += BSEP_UPDATE_THREADS) {
        float sz = part_z[p], szz = part_zz[p];
        for (int j = 1; j < s.chunks; ++j) {
            sz = sz + part_z[(size_t)j * s.P4 + p];
            szz = szz + part_zz[(size_t)j * s.P4 + p];
        }
        sums[p] = sz;
        sums[s.P4 + p] = szz;
        const float psn = __fadd_rn(__fmul_rn(k.a_s, s.ps[at + p]), __fmul_rn(k.b_s, sz));
        s.ps_out[at + p] = psn;
        acc = acc + (double)psn * (double)psn;                            // the square is exact in double
    }
    red[c] = acc;
    __syncthreads();
    for (int t = BSEP_UPDATE_THREADS / 2; t > 0; t >>= 1) {
        if (c < t) red[c] = red[c] + red[c + t];
        __syncthreads();
    }
    const float step_old = s.step[r];
    if (c == 0) {
        const double norm2 = red[0];
        const double nrm = sqrt(norm2);
        h_sh = nrm * tr.hsig_scale < k.hsig_thr ? 1 : 0;
        double e = k.cs_over_ds * (nrm / k.chi - 1.0);
        if (e > 1.0) e = 1.0;
        const float sn = (float)((double)step_old * exp(e));
        s.step_out[r] = fminf(fmaxf(sn, k.step_lo), k.step_hi);
    }
    __syncthreads();
    const bool h = h_sh != 0;
    const float hb = h ? k.hb1 : 0.0f;
    const float k0 = h ? k.k0_h1 : k.k0_h0;
    const float s0 = __fmul_rn(tr.sigma, step_old);
    for (int p = c; p < s.P; p += BSEP_UPDATE_THREADS) {
        const float sz = sums[p], szz = sums[s.P4 + p];
        const float Cv = s.C[at + p];
        const float sC = __builtin_sqrtf(Cv);
        const float y = __fmul_rn(sC, sz);
        const float pcn = __fadd_rn(__fmul_rn(k.a_c, s.pc[at + p]), __fmul_rn(hb, y));
        const float sd = __fmul_rn(s0, sC);
        s.pc_out[at + p] = pcn;
        s.mu_out[at + p] = __fadd_rn(s.mu[at + p], __fmul_rn(sd, sz));
        const float cn = __fadd_rn(__fadd_rn(__fmul_rn(k0, Cv), __fmul_rn(k.c1f, __fmul_rn(pcn, pcn))),
                                   __fmul_rn(k.cmuf, __fmul_rn(Cv, szz)));
        s.C_out[at + p] = fminf(fmaxf(cn, k.var_lo), k.var_hi);
    }
}

// k_perturb_sepcma per trial: one thread per (row of the whole batch, quad), the new (mu, C, step) read from the _out matrices the
// update launch of the same stream wrote.  The launch also leaves the rank vectors zeroed for the next generation's count.
__global__ __launch_bounds__(256) void k_bsep_perturb(BsepShape s)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s.stamp && t == 0) *s.stamp = real_time();                       // ses_set_stamp: the next population is being written
    for (long long i = t; i < s.n_clear; i += (long long)gridDim.x * 256) s.rank_to_clear[i] = 0;
    if (t >= (long long)s.R * s.n * s.quads) return;
    const long long row = t / s.quads;
    const int q = (int)(t - row * s.quads);
    const int r = (int)(row / s.n);
    const int i = (int)(row - (long long)r * s.n);
    const int lim = s.P - 4 * q < 4 ? s.P - 4 * q : 4;
    const ses_batch_sepcma_trial tr = s.trials[r];
    const float s0 = __fmul_rn(tr.next_sigma, s.step_out[r]);
    float z[4];
    normal4(tr.seed, tr.next_gen, (uint32_t)i, (uint32_t)q, z);
    const float *__restrict__ mu = s.mu_out + (size_t)r * s.P + 4 * q;
    const float *__restrict__ C = s.C_out + (size_t)r * s.P + 4 * q;
    float *dst = s.theta + (size_t)row * s.P + 4 * q;
    for (int l = 0; l < lim; ++l) {
        const float sd = __fmul_rn(s0, __builtin_sqrtf(C[l]));
        dst[l] = __fadd_rn(mu[l], __fmul_rn(sd, z[l]));
    }
}

}  // namespace ses

extern "C" {

using namespace ses;

int ses_sepcma_generation_batch(ses_handle *h, const float *fitness, int32_t R, int32_t n, const int32_t *mu,
                                const ses_batch_sepcma_trial *trials, const ses_batch_sepcma_consts *consts, const float *weights,
                                const float *mu_in, const float *C_in, const float *ps_in, const float *pc_in, const float *step_in,
                                float *mu_out, float *C_out, float *ps_out, float *pc_out, float *step_out, float *theta_next,
                                float *best)
{
    const char *who = "ses_sepcma_generation_batch";
    SES_REQUIRE(h && fitness && mu && trials && consts && weights && mu_in && C_in && ps_in && pc_in && step_in && mu_out && C_out &&
                    ps_out && pc_out && step_out && theta_next, "%s: null argument", who);
    SES_REQUIRE(mu_in != mu_out && C_in != C_out && ps_in != ps_out && pc_in != pc_out && step_in != step_out,
                "%s: in and out matrices must be distinct buffers", who);
    SES_REQUIRE(R >= 1, "%s: %d trials; there must be at least 1", who, R);
    SES_REQUIRE(n >= 4, "%s: %d rows per trial; there must be at least 4", who, n);
    if (n > BSEP_MAX_N)
        return set_error(SES_ERR_UNSUPPORTED, "%s: %d rows per trial; the batch tail ranks by counting, up to %d rows per trial", who, n,
                         BSEP_MAX_N);
    SES_REQUIRE((long long)R * n <= BSEP_MAX_ROWS, "%s: %d trials x %d rows exceed %lld rows in all", who, R, n, BSEP_MAX_ROWS);
    for (int r = 0; r < R; ++r)
        SES_REQUIRE(mu[r] >= 1 && mu[r] <= n, "%s: trial %d has mu = %d outside [1, %d]", who, r, mu[r], n);
    const int quads = (h->P + 3) / 4, P4 = 4 * quads;
    SES_REQUIRE(quads <= 65535 && (long long)R * n * quads / 256 < (1ll << 31),
                "%s: %d trials x %d rows x %d parameters exceed the launch grids", who, R, n, h->P);
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    const int rows = R * n;
    const int jt = rank_count_slice(n);
    const int chunks = ceil_div(n, SEPCMA_CHUNK);
    // scratch: the R rank vectors, one behind the other, where the solo tails keep their own | chunk partials [R][2][chunks][P4] |
    // sums [R][2][P4]
    const size_t rank_bytes = (sizeof(int32_t) * (size_t)rows + 255) / 256 * 256;
    const size_t partial_floats = (size_t)R * 2 * chunks * P4;
    const int rc = ensure_reduce_scratch(h, rank_bytes + sizeof(float) * (partial_floats + (size_t)R * 2 * P4));
    if (rc != SES_OK) return rc;
    int32_t *rank = (int32_t *)h->red_scratch;
    float *partial = (float *)((char *)rank + rank_bytes);
    // zero on entry: left so by the population-writing launch of the previous call, solo or batch, of the same row count; a memset
    // otherwise.  From here to that launch the vector holds counts, and an early return leaves the cache saying so.
    const int zrc = tail_rank_take(h, rank, rows);
    if (zrc != SES_OK) return zrc;
    h->counter_armed = nullptr;                     // the partials may lie over the ticket counters of a solo layout
    hipLaunchKernelGGL(k_batch_rank_count, dim3(R, ceil_div(n, 256), ceil_div(n, jt)), dim3(256), 0, h->stream, fitness, n, jt, rank);
    const BsepShape s{trials, consts, weights, R, n, chunks, h->P, P4, quads, partial, partial + partial_floats, mu_in, C_in, ps_in,
                      pc_in, step_in, mu_out, C_out, ps_out, pc_out, step_out, theta_next, h->stamp, rank, rows};
    hipLaunchKernelGGL(k_bsep_sums_partial, dim3(R, quads, chunks), dim3(256), 0, h->stream, s, rank, fitness, best);
    hipLaunchKernelGGL(k_bsep_update, dim3(R), dim3(BSEP_UPDATE_THREADS), 0, h->stream, s);
    hipLaunchKernelGGL(k_bsep_perturb, dim3(ceil_div((long long)rows * quads, 256)), dim3(256), 0, h->stream, s);
    SES_HIP_TRY(hipGetLastError());
    tail_rank_cleared(h, rank, rows);
    return SES_OK;
}

}  // extern "C"
