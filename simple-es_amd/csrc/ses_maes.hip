// ses_maes.hip -- the ma_es strategy: matrix adaptation ES (Beyer & Sendhoff 2017, "Simplify your covariance matrix adaptation
// evolution strategy") with the full P x P transformation matrix M and cumulative step-size adaptation whose scalar lives on the
// device.  No reference counterpart: a seventh strategy with the shape of the sep_cma_es / lm_ma_es tail, for policies of up to
// MAES_MAX_P = 1024 parameters (M is 4 MB there).  A unit of its own: the kernels of the other units keep their machine code.
//
//   population  n rows:  D = Z M^T (one GEMM, Z regenerated from Philox inside the kernel), theta = mu + (sigma * step) D
//   tail        rank -> weighted sums (k_sepcma_sums_partial as it is: the chunk partials of Sz; its Szz half is not read) ->
//               vectors (Sz, p_sigma', norm2, step', the list of selected rows) in ONE workgroup -> Sd = M Sz, qv = M p_sigma', mu'
//               (a wave per row of M) -> G = (W D)^T Z over the selected rows (one GEMM), M' in its epilogue -> next population
//
// Both GEMMs run on v_mfma_f32_32x32x2_f32 with ONE fp32 accumulator chain per 32 x 32 output tile, k-blocks in ascending order
// from +0.  The instruction adds its two products one after the other with one rounding each (tools/mfma_exact.hip), so
//     D[i][p] = the chain  acc = fma(z_i[q], M[p][q], acc)  over q = 0, 1, ..., P - 1 (an odd P adds fma(+0, +0, acc) once more)
//     G[p][q] = the chain  acc = fma(fl(w_j D[s_j][p]), z_{s_j}[q], acc)  over the selected rows s_0 < s_1 < ... (ascending ROW
//               index; an odd count adds fma(+0, +0, acc) once more)
// whatever tile an element falls into: the orders depend on P and on the set of selected rows only, and a row range that starts off
// a tile boundary, or D recomputed by another launch, gives the same bits.
// A workgroup is four waves = four column tiles of one row tile.  The operands of MAES_KC = 32 values of k are staged in LDS, every
// tile k-major with rows of 33 floats (a staging write walks k or the row, a fragment read walks the row: all free of bank
// conflicts bar one pair).  The four waves share one draw of the noise, which is the A operand of both GEMMs (the update forms
// G^T): a Philox call per (row, quad) and chunk for the whole workgroup.  Two LDS buffers, one barrier per chunk; the
// next chunk's global loads and Philox calls are issued around the current chunk's MFMAs.  No workgroup waits for another.
// Order of Sd[p] = sum_q M[p][q] Sz[q] and qv[p] = sum_q M[p][q] p_sigma'[q] (k_maes_matvec; depends on P only): one wave per p, lane
// l takes q = l, l + 64, ... in ascending order as ONE fma chain from +0 (acc = fma(M[p][q], x[q], acc)), then over the 64 lanes
// x[lane] = x[lane] + x[lane ^ s] for s = 32, 16, 8, 4, 2, 1.  Sz and norm2 are summed in ses_sepcma.hip's orders.
#include <cmath>

#include "ses_internal.h"
#include "ses_math.h"
#include "ses_rng.h"
#include "ses_tail.h"

namespace ses {

constexpr int MAES_MAX_P = 1024;             // parameters (SES_MAES_MAX_P): M is MAES_MAX_P^2 floats
constexpr int MAES_KC = 32;                  // values of k staged per chunk = 16 k-blocks of the MFMA
constexpr int MAES_WAVES = 4;                // waves per workgroup = column tiles that share a row tile's A operand
constexpr int MAES_COLS = 32 * MAES_WAVES;   // columns per workgroup
constexpr int MAES_LDB = 33;                 // floats per k-row of a staged tile
constexpr int MAES_VEC_THREADS = 1024;       // the one workgroup of k_maes_vectors

typedef float maes_f32x16 __attribute__((ext_vector_type(16)));

struct MaesLds {
    float a[2][MAES_KC][MAES_LDB];                   // [k][row of the tile]
    float b[2][MAES_WAVES][MAES_KC][MAES_LDB];       // [column tile][k][column]
};

// the 16 k-blocks (fewer in the last chunk) of one staged chunk: lane l holds A[row = l & 31][k = 2 j + (l >> 5)] and
// B[k = 2 j + (l >> 5)][column = l & 31]
__device__ __forceinline__ maes_f32x16 maes_chunk_mfma(const MaesLds &lds, int buf, int wave, int lane, int nkb, maes_f32x16 acc)
{
    const float *af = &lds.a[buf][lane >> 5][lane & 31];
    const float *bf = &lds.b[buf][wave][lane >> 5][lane & 31];
#pragma unroll
    for (int j = 0; j < MAES_KC / 2; ++j)
        if (j < nkb) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(af[2 * MAES_LDB * j], bf[2 * MAES_LDB * j], acc, 0, 0, 0);
    return acc;
}

// ---- perturbation: D = Z M^T, theta = mu + s D ---------------------------------------------------------------------------
struct MaesPerturb {
    const float *mu, *M, *step;
    float sigma;
    int n_rows, P, quads;
    uint64_t seed, gen;
    long long first_row;
    float *theta, *d_out;
    unsigned long long *stamp;
    int32_t *rank_to_clear;
    int n_clear;
};

// Workgroup (x, y) = rows [32 x, 32 x + 32) of the range, columns [128 y, 128 y + 128); wave w owns the columns from 128 y + 32 w.
// Rows are global.  Outside [0, P) both operands of a k are +0; rows and columns that do not exist run on whatever the clamped
// index gives (zeros for M) and are not stored.  step is read from device memory: the update of the same stream wrote it.
__global__ __launch_bounds__(64 * MAES_WAVES) void k_maes_perturb(MaesPerturb a)
{
    __shared__ MaesLds lds;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long lin = ((long long)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + t;
    if (a.stamp && lin == 0) *a.stamp = real_time();                    // ses_set_stamp: the next population is being written
    // the rank vector has been consumed by the tail: leave it zeroed for the next generation's count
    for (long long i = lin; i < a.n_clear; i += (long long)gridDim.x * gridDim.y * blockDim.x) a.rank_to_clear[i] = 0;
    if (a.n_rows <= 0) return;                                          // (the whole grid: no barrier is left behind)
    const int P = a.P;
    const long long row0 = (long long)blockIdx.x * 32;
    const int p0 = blockIdx.y * MAES_COLS;
    const int nchunks = (P + MAES_KC - 1) / MAES_KC, kblocks = (P + 1) / 2;
    // staging roles: the noise of (row zr, quad zq of the chunk); M[p0 + mr + 8 i][k0 + mk], i < 16
    const int zr = t & 31, zq = t >> 5;
    const int mk = t & 31, mr = t >> 5;
    float z[4], m[16];
    bool m_in = false;
    auto fetch = [&](int chunk) {
        const int k0 = chunk * MAES_KC;
        const int q = chunk * (MAES_KC / 4) + zq;
        if (q < a.quads) {
            normal4(a.seed, a.gen, (uint32_t)(a.first_row + row0 + zr), (uint32_t)q, z);
#pragma unroll
            for (int l = 0; l < 4; ++l)
                if (4 * q + l >= P) z[l] = 0.0f;
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l) z[l] = 0.0f;
        }
        // (every load is made, from a clamped address, and what lies outside M is dropped when the values are staged: sixteen loads in
        //  flight behind the MFMAs, not sixteen round trips in front of them)
        const int kc = k0 + mk < P ? k0 + mk : P - 1;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int p = p0 + mr + 8 * i;
            m[i] = a.M[(size_t)(p < P ? p : P - 1) * P + kc];
        }
        m_in = k0 + mk < P;
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int l = 0; l < 4; ++l) lds.a[buf][4 * zq + l][zr] = z[l];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = mr + 8 * i;
            lds.b[buf][c >> 5][mk][c & 31] = (m_in && p0 + c < P) ? m[i] : 0.0f;
        }
    };
    const bool active = p0 + 32 * wave < P;                             // (a wave without columns still stages its share)
    maes_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    fetch(0);
    stage(0);
    __syncthreads();
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        const int buf = chunk & 1;
        const bool more = chunk + 1 < nchunks;
        if (more) fetch(chunk + 1);
        const int left = kblocks - chunk * (MAES_KC / 2);
        if (active) acc = maes_chunk_mfma(lds, buf, wave, lane, left < MAES_KC / 2 ? left : MAES_KC / 2, acc);
        __builtin_amdgcn_sched_barrier(0);                              // (the staging waits for the loads: it stays behind the MFMAs)
        if (more) stage(buf ^ 1);
        __syncthreads();                                                // the only barrier of a chunk: the next one fills the other buffer
    }
    const int p = p0 + 32 * wave + (lane & 31);
    if (!active || p >= P) return;
    const float s0 = __fmul_rn(a.sigma, a.step[0]);
    const float mup = a.theta ? a.mu[p] : 0.0f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long long il = row0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (il >= a.n_rows) continue;
        const float d = acc[r];
        if (a.d_out) a.d_out[(size_t)il * P + p] = d;
        if (a.theta) a.theta[(size_t)il * P + p] = __fadd_rn(mup, __fmul_rn(s0, d));
    }
}

// ---- the vectors of the update ----------------------------------------------------------------------------------------------
struct MaesVectors {
    const float *partial;              // the Sz half of k_sepcma_sums_partial's chunk partials
    const int32_t *rank;
    const float *weights;
    int chunks, P, P4, n, mu;
    float a_s, b_s, step_lo, step_hi;
    double cs_over_ds, chi;
    const float *ps, *step;
    float *ps_out, *step_out, *sz, *sz_out, *wsel;
    int32_t *sel;
    double *norm2_out;
};

// ONE workgroup of MAES_VEC_THREADS threads.  Chunk partials added in ascending order, Sz and p_sigma' written, the squares added in
// double (ses_sepcma.hip's orders); thread 0: the scalar path in double.  Then the selected rows (rank < mu) in ascending row index:
// thread c counts those among its own run of consecutive rows, a scan over the threads places them; sel[j] = the row, wsel[j] = its weight.
__global__ __launch_bounds__(MAES_VEC_THREADS) void k_maes_vectors(MaesVectors u)
{
    __shared__ double red[MAES_VEC_THREADS];
    __shared__ int scan[MAES_VEC_THREADS];
    const int c = threadIdx.x;
    double acc = 0.0;
    for (int p = c; p < u.P; p += MAES_VEC_THREADS) {
        float s = u.partial[p];
        for (int k = 1; k < u.chunks; ++k) s = s + u.partial[(size_t)k * u.P4 + p];
        u.sz[p] = s;
        if (u.sz_out) u.sz_out[p] = s;
        const float psn = __fadd_rn(__fmul_rn(u.a_s, u.ps[p]), __fmul_rn(u.b_s, s));
        u.ps_out[p] = psn;
        acc = acc + (double)psn * (double)psn;                            // the square is exact in double
    }
    red[c] = acc;
    const int per = (u.n + MAES_VEC_THREADS - 1) / MAES_VEC_THREADS;
    const long long lo = (long long)c * per;
    const int i0 = lo < u.n ? (int)lo : u.n, i1 = lo + per < u.n ? (int)(lo + per) : u.n;
    int cnt = 0;
    for (int i = i0; i < i1; ++i) cnt += u.rank[i] < u.mu ? 1 : 0;
    scan[c] = cnt;
    __syncthreads();
    for (int s = MAES_VEC_THREADS / 2; s > 0; s >>= 1) {
        if (c < s) red[c] = red[c] + red[c + s];
        __syncthreads();
    }
    if (c == 0) {
        const double norm2 = red[0];
        double e = u.cs_over_ds * (sqrt(norm2) / u.chi - 1.0);
        if (e > 1.0) e = 1.0;
        const float sn = (float)((double)u.step[0] * exp(e));
        u.step_out[0] = fminf(fmaxf(sn, u.step_lo), u.step_hi);
        if (u.norm2_out) u.norm2_out[0] = norm2;
    }
    for (int s = 1; s < MAES_VEC_THREADS; s <<= 1) {                    // inclusive scan of the counts
        const int add = c >= s ? scan[c - s] : 0;
        __syncthreads();
        scan[c] += add;
        __syncthreads();
    }
    int j = scan[c] - cnt;
    for (int i = i0; i < i1; ++i) {
        const int r = u.rank[i];
        if (r < u.mu && j < u.mu) {
            u.sel[j] = i;
            u.wsel[j] = u.weights[r];
            ++j;
        }
    }
    // the ranks are a permutation, so exactly mu rows are selected -- unless a NaN fitness has broken the count: the list then stays
    // inside its mu entries, and entries no row claimed carry weight 0
    for (int k = scan[MAES_VEC_THREADS - 1] + c; k < u.mu; k += MAES_VEC_THREADS) {
        u.sel[k] = 0;
        u.wsel[k] = 0.0f;
    }
}

// x[lane] + x[lane ^ s] for s = 32 ... 1: the sum over the wave, the same bits in every lane
__device__ __forceinline__ float maes_wave_sum(float x)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) x = x + __shfl_xor(x, s, 64);
    return x;
}

struct MaesMatvec {
    const float *M, *sz, *ps_new, *mu, *step;
    int P;
    float sigma;                       // the curr_sigma the evaluated population was drawn with
    float *sd, *qv, *mu_out, *sd_out, *qv_out;
};

// one wave per row p of the OLD M: Sd[p], qv[p] (the order in the header of this file) and mu'[p] with the old step
__global__ __launch_bounds__(256) void k_maes_matvec(MaesMatvec u)
{
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= u.P) return;
    const float *Mp = u.M + (size_t)p * u.P;
    float sd = 0.0f, qv = 0.0f;
    for (int q = lane; q < u.P; q += 64) {
        const float m = Mp[q];
        sd = fma_(m, u.sz[q], sd);
        qv = fma_(m, u.ps_new[q], qv);
    }
    sd = maes_wave_sum(sd);
    qv = maes_wave_sum(qv);
    if (lane != 0) return;
    u.sd[p] = sd;
    u.qv[p] = qv;
    if (u.sd_out) u.sd_out[p] = sd;
    if (u.qv_out) u.qv_out[p] = qv;
    u.mu_out[p] = __fadd_rn(u.mu[p], __fmul_rn(__fmul_rn(u.sigma, u.step[0]), sd));
}

// ---- update: G = (W D)^T Z over the selected rows, M' in the epilogue ----------------------------------------------------------
struct MaesUpdate {
    const float *D, *M, *qv, *ps_new, *wsel;
    const int32_t *sel;
    int P, quads, mu;
    uint64_t seed, gen;
    float a_m, c1h, cmuh;
    float *M_out, *g_out;
};

// The kernel forms G^T, so that the noise is again the operand the four waves share: workgroup (x, y) = columns q in [32 x, 32 x + 32)
// of G (the rows of the MFMA tile), rows p in [128 y, 128 y + 128) (its columns; wave w owns those from 128 y + 32 w).  k walks the
// selected rows: A[q][j] = the noise of (row sel[j], column q), B[j][p] = fl(wsel[j] D[sel[j]][p]); past the last selected row both
// are +0.  The product of an fma commutes, so every element is the chain stated in the header.  The epilogue turns each wave's tile
// round in LDS: M and M' are read and written along q.
__global__ __launch_bounds__(64 * MAES_WAVES) void k_maes_update(MaesUpdate u)
{
    __shared__ MaesLds lds;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int P = u.P;
    const int q0 = blockIdx.x * 32, p0 = blockIdx.y * MAES_COLS;
    const int nchunks = (u.mu + MAES_KC - 1) / MAES_KC, kblocks = (u.mu + 1) / 2;
    // staging roles: the noise of (selected row k0 + zj, quad q0 / 4 + zq); B[k0 + bj + 2 i][p0 + bp], i < 16
    const int zj = t & 31, zq = t >> 5;
    const int bp = t & (MAES_COLS - 1), bj = t >> 7;
    float z[4], b[16], w[16], w_next[16];
    int row[16], zrow;
    // the rows and weights of a chunk's selected rows are read one chunk ahead of its D: a load whose address hangs on a load is a
    // round trip of its own, and sixteen of them in front of the MFMAs were most of this kernel's time.  Every load is made, from a
    // clamped index; what lies past the selection or past P is dropped when the values are staged, behind the MFMAs.
    auto fetch_rows = [&](int chunk) {
        const int k0 = chunk * MAES_KC;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int j = k0 + bj + 2 * i, jc = j < u.mu ? j : u.mu - 1;
            row[i] = u.sel[jc];
            w_next[i] = u.wsel[jc];
        }
        zrow = u.sel[k0 + zj < u.mu ? k0 + zj : u.mu - 1];
    };
    const int pc = p0 + bp < P ? p0 + bp : P - 1;
    auto fetch = [&](int chunk) {                                       // (after fetch_rows(chunk))
        const int k0 = chunk * MAES_KC;
        const int q = q0 / 4 + zq;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            b[i] = u.D[(size_t)row[i] * P + pc];
            w[i] = k0 + bj + 2 * i < u.mu ? w_next[i] : 0.0f;
        }
        if (k0 + zj < u.mu && q < u.quads) {
            normal4(u.seed, u.gen, (uint32_t)zrow, (uint32_t)q, z);
        } else {
#pragma unroll
            for (int l = 0; l < 4; ++l) z[l] = 0.0f;
        }
        fetch_rows(chunk + 1);
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int l = 0; l < 4; ++l) lds.a[buf][zj][4 * zq + l] = z[l];
#pragma unroll
        for (int i = 0; i < 16; ++i) lds.b[buf][bp >> 5][bj + 2 * i][bp & 31] = p0 + bp < P ? __fmul_rn(w[i], b[i]) : 0.0f;
    };
    const bool active = p0 + 32 * wave < P;
    maes_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    fetch_rows(0);
    fetch(0);
    stage(0);
    __syncthreads();
    for (int chunk = 0; chunk < nchunks; ++chunk) {
        const int buf = chunk & 1;
        const bool more = chunk + 1 < nchunks;
        if (more) fetch(chunk + 1);
        const int left = kblocks - chunk * (MAES_KC / 2);
        if (active) acc = maes_chunk_mfma(lds, buf, wave, lane, left < MAES_KC / 2 ? left : MAES_KC / 2, acc);
        __builtin_amdgcn_sched_barrier(0);                              // (the staging waits for the loads: it stays behind the MFMAs)
        if (more) stage(buf ^ 1);
        __syncthreads();
    }
    // acc[r] = G[p0 + 32 wave + (lane & 31)][q0 + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)]: through the wave's own B tile of buffer 0
    // (every wave is past its last read of it) as tile[p][q], then 16 passes of two rows p, the lanes along q
    float (*tile)[MAES_LDB] = lds.b[0][wave];
    if (active) {
#pragma unroll
        for (int r = 0; r < 16; ++r) tile[lane & 31][(r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)] = acc[r];
    }
    __syncthreads();
    const int q = q0 + (lane & 31);
    if (!active || q >= P) return;
    const float psq = u.ps_new[q];
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int pl = 2 * it + (lane >> 5), p = p0 + 32 * wave + pl;
        if (p >= P) continue;
        const float g = tile[pl][lane & 31];
        const size_t at = (size_t)p * P + q;
        if (u.g_out) u.g_out[at] = g;
        u.M_out[at] = __fadd_rn(__fadd_rn(__fmul_rn(u.a_m, u.M[at]), __fmul_rn(u.c1h, __fmul_rn(u.qv[p], psq))), __fmul_rn(u.cmuh, g));
    }
}

static void launch_perturb_maes(ses_handle *h, const float *mu, const float *M, const float *step, float sigma, uint64_t seed,
                                uint64_t gen, long long first_row, int n_rows, float *theta, float *d_out, unsigned long long *stamp,
                                int32_t *rank_to_clear, int n_clear)
{
    MaesPerturb a;
    a.mu = mu; a.M = M; a.step = step; a.sigma = sigma;
    a.n_rows = n_rows; a.P = h->P; a.quads = (h->P + 3) / 4;
    a.seed = seed; a.gen = gen; a.first_row = first_row;
    a.theta = theta; a.d_out = d_out; a.stamp = stamp; a.rank_to_clear = rank_to_clear; a.n_clear = n_clear;
    const dim3 grid(n_rows > 0 ? ceil_div(n_rows, 32) : 1, n_rows > 0 ? ceil_div(h->P, MAES_COLS) : 1);
    hipLaunchKernelGGL(k_maes_perturb, grid, dim3(64 * MAES_WAVES), 0, h->stream, a);
}

static int maes_check_handle(ses_handle *h, const char *who)
{
    if (h->P > MAES_MAX_P)
        return set_error(SES_ERR_UNSUPPORTED, "%s: %d parameters; the ma_es kernels hold at most %d (lm_ma_es serves larger policies)",
                         who, h->P, MAES_MAX_P);
    return SES_OK;
}

}  // namespace ses

extern "C" {

using namespace ses;

int ses_perturb_maes(ses_handle *h, const float *mu, const float *M, const float *step, float sigma, uint64_t seed, uint64_t gen,
                     int64_t first_row, int32_t n_rows, float *theta, float *d_out)
{
    SES_REQUIRE(h && mu && M && step && (theta || d_out), "ses_perturb_maes: null argument");
    const int rc = maes_check_handle(h, "ses_perturb_maes");
    if (rc != SES_OK) return rc;
    SES_REQUIRE(n_rows >= 1 && first_row >= 0 && first_row + n_rows <= (1ll << 30), "ses_perturb_maes: row range");
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    launch_perturb_maes(h, mu, M, step, sigma, seed, gen, (long long)first_row, n_rows, theta, d_out, h->stamp, nullptr, 0);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int ses_maes_generation(ses_handle *h, const float *fitness, int32_t n, uint64_t seed, uint64_t gen, double sigma,
                        const ses_maes_params *p, const float *weights, const float *mu_in, const float *ps_in, const float *M_in,
                        const float *step_in, const float *d_in, float *mu_out, float *ps_out, float *M_out, float *step_out,
                        float next_sigma, uint64_t next_gen, int64_t first_row, int32_t n_rows, float *theta_next, float *d_next_out,
                        float *best, float *sz_out, float *sd_out, float *qv_out, float *g_out, double *norm2_out)
{
    SES_REQUIRE(h && fitness && p && weights && mu_in && ps_in && M_in && step_in && mu_out && ps_out && M_out && step_out,
                "ses_maes_generation: null argument");
    int rc = maes_check_handle(h, "ses_maes_generation");
    if (rc != SES_OK) return rc;
    SES_REQUIRE(mu_in != mu_out && ps_in != ps_out && M_in != M_out && step_in != step_out && (!d_in || d_in != d_next_out),
                "ses_maes_generation: in and out buffers must be distinct");
    rc = tail_check_rows("ses_maes_generation", n, false, first_row, n_rows, theta_next);
    if (rc != SES_OK) return rc;
    SES_REQUIRE(p->mu >= 1 && p->mu <= n, "ses_maes_generation: mu = %d outside [1, %d]", p->mu, n);
    SES_REQUIRE(p->step_lo > 0.0f && p->step_lo <= p->step_hi, "ses_maes_generation: bad step limits");
    SES_REQUIRE(p->mueff >= 1.0 && p->c_sigma > 0.0 && p->c_sigma < 1.0 && p->d_sigma > 0.0 && p->chi > 0.0 && p->c_1 >= 0.0 &&
                    p->c_mu >= 0.0 && p->c_1 + p->c_mu <= 1.0,
                "ses_maes_generation: constants out of range");
    const int P = h->P, quads = (P + 3) / 4, P4 = 4 * quads;
    const int chunks = ceil_div(n, SEPCMA_CHUNK);
    // behind the rank vector: the chunk partials of Sz, then of Szz (k_sepcma_sums_partial's layout) | Sz | Sd | qv | the weights
    // and the rows of the selection | D of all n rows where the caller has none
    const size_t floats = 2 * (size_t)chunks * P4 + 3 * (size_t)P4 + 2 * (size_t)p->mu + (d_in ? 0 : (size_t)n * P);
    int32_t *rank;
    float *partial;
    rc = tail_rank_begin(h, fitness, n, sizeof(float) * floats, &rank, (void **)&partial);
    if (rc != SES_OK) return rc;
    float *sz = partial + 2 * (size_t)chunks * P4, *sd = sz + P4, *qv = sd + P4, *wsel = qv + P4;
    int32_t *sel = (int32_t *)(wsel + p->mu);
    if (!d_in) {
        // the rows this rank never drew (the replicated tail of a sharded run): the same chains, hence the same bits
        float *d_all = (float *)(sel + p->mu);
        launch_perturb_maes(h, mu_in, M_in, step_in, (float)sigma, seed, gen, 0, n, nullptr, d_all, nullptr, nullptr, 0);
        d_in = d_all;
    }
    hipLaunchKernelGGL(k_sepcma_sums_partial, dim3(quads, chunks), dim3(256), 0, h->stream, rank, fitness, n, p->mu, weights, seed, gen,
                       P4, chunks, partial, best);
    MaesVectors v;
    v.partial = partial; v.rank = rank; v.weights = weights;
    v.chunks = chunks; v.P = P; v.P4 = P4; v.n = n; v.mu = p->mu;
    v.a_s = (float)(1.0 - p->c_sigma);
    v.b_s = (float)std::sqrt(p->c_sigma * (2.0 - p->c_sigma) * p->mueff);
    v.step_lo = p->step_lo; v.step_hi = p->step_hi;
    v.cs_over_ds = p->c_sigma / p->d_sigma;
    v.chi = p->chi;
    v.ps = ps_in; v.step = step_in;
    v.ps_out = ps_out; v.step_out = step_out; v.sz = sz; v.sz_out = sz_out; v.wsel = wsel; v.sel = sel; v.norm2_out = norm2_out;
    hipLaunchKernelGGL(k_maes_vectors, dim3(1), dim3(MAES_VEC_THREADS), 0, h->stream, v);
    MaesMatvec m;
    m.M = M_in; m.sz = sz; m.ps_new = ps_out; m.mu = mu_in; m.step = step_in; m.P = P; m.sigma = (float)sigma;
    m.sd = sd; m.qv = qv; m.mu_out = mu_out; m.sd_out = sd_out; m.qv_out = qv_out;
    hipLaunchKernelGGL(k_maes_matvec, dim3(ceil_div(P, 4)), dim3(256), 0, h->stream, m);
    MaesUpdate u;
    u.D = d_in; u.M = M_in; u.qv = qv; u.ps_new = ps_out; u.wsel = wsel; u.sel = sel;
    u.P = P; u.quads = quads; u.mu = p->mu; u.seed = seed; u.gen = gen;
    u.a_m = p->a_m; u.c1h = p->c1h; u.cmuh = p->cmuh;
    u.M_out = M_out; u.g_out = g_out;
    hipLaunchKernelGGL(k_maes_update, dim3(ceil_div(P, 32), ceil_div(P, MAES_COLS)), dim3(64 * MAES_WAVES), 0, h->stream, u);
    // the next population from the new (mu, M, step); the launch also clears the rank vector for the next generation
    launch_perturb_maes(h, mu_out, M_out, step_out, next_sigma, seed, next_gen, (long long)first_row, n_rows, theta_next, d_next_out,
                        h->stamp, rank, n);
    SES_HIP_TRY(hipGetLastError());
    tail_rank_cleared(h, rank, n);
    return SES_OK;
}

}  // extern "C"
