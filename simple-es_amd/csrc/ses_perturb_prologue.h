// ses_perturb_prologue.h -- the end of an openai_es generation as device functions: the Adam update of the mean from the
// gradient's chunk partials, and the rows of the next population drawn from it.  Two kernels compile this one text:
// k_es_apply_perturb (ses_strategy.hip: a launch of its own, every row of the population) and the rollout kernels that
// form the rows they are about to run themselves (ses_rollout.hip: k_rollout_cartpole_mlp_handover_perturb).
#pragma once
#include "ses_internal.h"
#include "ses_rng.h"

namespace ses {

// ------------------------------------------------------------------------------------------------ K5
// Adam exactly as optimizers.py:42-57 evaluates it under numpy >= 2 promotion rules:
// float32 moments, float64 step, float32 parameter store.
__device__ __forceinline__ void adam_apply(float g, double adam_a, float &mu, float &m, float &v)
{
    const float b1 = 0.99f, b2 = 0.999f;
    const float omb1 = (float)(1.0 - 0.99), omb2 = (float)(1.0 - 0.999);
    const float mn = (b1 * m) + (omb1 * g);
    const float vn = (b2 * v) + (omb2 * (g * g));
    const double num = (-adam_a) * (double)mn;
    const float den = __builtin_sqrtf(vn) + 1e-08f;
    const double step = num / (double)den;
    m = mn;
    v = vn;
    mu = (float)((double)mu + step);
}

// Parameter p of the update in two halves, so that a caller can put work between the loads and their use: the operands (the first
// UPDATE_PRELOAD chunk partials, mu, m, v), then the chunk partials added in ascending chunk order, the factor, Adam -- k_es_apply's
// arithmetic.
constexpr int UPDATE_PRELOAD = 4;
struct UpdateOperands {
    float part[UPDATE_PRELOAD];
    float mu, m, v;
};
__device__ __forceinline__ UpdateOperands es_update_load(const PerturbUpdate &u, int p)
{
    UpdateOperands o;
#pragma unroll
    for (int c = 0; c < UPDATE_PRELOAD; ++c) o.part[c] = c < u.chunks ? u.partial[(size_t)c * u.P4 + p] : 0.0f;
    o.mu = u.mu_in[p]; o.m = u.m_in[p]; o.v = u.v_in[p];
    return o;
}
__device__ __forceinline__ void es_update_finish(const PerturbUpdate &u, int p, UpdateOperands &o)
{
    float sum = o.part[0];
#pragma unroll
    for (int c = 1; c < UPDATE_PRELOAD; ++c)
        if (c < u.chunks) sum = sum + o.part[c];
    for (int c = UPDATE_PRELOAD; c < u.chunks; ++c) sum = sum + u.partial[(size_t)c * u.P4 + p];
    const float g = sum * u.update_factor;                                // offspring_strategies.py:414
    adam_apply(g, u.adam_a, o.mu, o.m, o.v);
}

// The whole new mean into mu_new[P] (LDS), a thread per parameter, by EVERY workgroup; workgroup 0 also stores mu / m / v.  The
// grid clears the rank vector, thread 0 writes the time stamp.  The in and out vectors are distinct buffers, so no workgroup can
// read a value another one has already replaced.  `first`: the operands of parameter threadIdx.x, already loaded (or null).  No
// barrier inside: the caller synchronises before mu_new is read.
__device__ __forceinline__ void perturb_update_mean(const PerturbUpdate &u, float *mu_new, UpdateOperands *first = nullptr)
{
    const int block = (int)blockDim.x;
    const long long t = (long long)blockIdx.x * block + threadIdx.x;
    if (u.stamp && t == 0) *u.stamp = real_time();
    for (int p = threadIdx.x; p < u.P; p += block) {
        UpdateOperands o = (first && p == (int)threadIdx.x) ? *first : es_update_load(u, p);
        es_update_finish(u, p, o);
        mu_new[p] = o.mu;
        if (blockIdx.x == 0) { u.mu_out[p] = o.mu; u.m_out[p] = o.m; u.v_out[p] = o.v; }
    }
    for (long long i = t; i < u.n_clear; i += (long long)gridDim.x * block) u.rank_to_clear[i] = 0;
}

// quad q of row i of this rank's shard (global row first_row + i; global row 0 = the mean itself): up to four values
__device__ __forceinline__ int perturb_row_quad(const PerturbUpdate &u, const float *mu_new, int i, int q, float (&out)[4])
{
    const int lim = u.P - 4 * q < 4 ? u.P - 4 * q : 4;
    const long long row = u.first_row + i;
    if (row == 0) {
        for (int l = 0; l < lim; ++l) out[l] = mu_new[4 * q + l];
        return lim;
    }
    float z[4];
    normal4(u.seed, u.gen, (uint32_t)row, (uint32_t)q, z);
    for (int l = 0; l < lim; ++l) out[l] = fma_(u.sigma, z[l], mu_new[4 * q + l]);
    return lim;
}

// consecutive rows of the shard
struct RowSpan {
    int row0, rows;
};
// the rows that hold envs [env0, env1) at E envs per row
__device__ __forceinline__ RowSpan rows_of_envs(int env0, int env1, int E)
{
    if (env1 <= env0) return RowSpan{0, 0};
    const int r0 = env0 / E;
    return RowSpan{r0, (env1 - 1) / E - r0 + 1};
}
// (how many rows n consecutive envs can touch at most: max_rows_of_envs, ses_rollout_plan.h)

// The prologue of a rollout workgroup that forms its own rows: the new mean (perturb_update_mean), then the rows of spans a and b
// -- the rows its waves are about to run -- into lds_rows (span a's rows first, P floats each) AND into u.theta, the population
// in global memory, which stays an output of the generation.  A row that two workgroups need is formed and stored by both: the
// same bits.  tanh_lds (or null): the tanh table is staged on the way, as stage_tanh_table does.  Every thread of the workgroup
// must call it (two barriers); nothing waits on another workgroup.
// Order: the loads of the update and of the table go out first; the normals of the workgroup's first items -- which depend on
// (seed, generation, row, quad) only -- are drawn while they fly, up to PERTURB_BATCH items per thread side by side (a wave of the
// rollout kernels shares its SIMD with one other wave: a single Philox + Box-Muller chain would wait on itself); then Adam, the
// barrier, and the rows.
constexpr int PERTURB_BATCH = 3;
struct PerturbItems {
    float z[PERTURB_BATCH][4];
    int i[PERTURB_BATCH], q[PERTURB_BATCH], s[PERTURB_BATCH];     // row of the shard, quad, LDS row slot
};
template <int K>
__device__ __forceinline__ void perturb_draw(const PerturbUpdate &u, RowSpan a, RowSpan b, int base, int items, PerturbItems &it)
{
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int w = base + k * (int)blockDim.x + (int)threadIdx.x;
        w = w < items ? w : items - 1;                                   // (a lane past the last item draws it again and stores nothing)
        const int s = w / u.quads;
        it.s[k] = s;
        it.q[k] = w - s * u.quads;
        it.i[k] = s < a.rows ? a.row0 + s : b.row0 + (s - a.rows);
        normal4(u.seed, u.gen, (uint32_t)(u.first_row + it.i[k]), (uint32_t)it.q[k], it.z[k]);
    }
}
// how many of the next PERTURB_BATCH items per thread THIS WAVE has (wave-uniform)
__device__ __forceinline__ int perturb_batch_count(int base, int items)
{
    const int left = items - (base + ((int)threadIdx.x & ~63));
    const int n = left <= 0 ? 0 : (left + (int)blockDim.x - 1) / (int)blockDim.x;
    return __builtin_amdgcn_readfirstlane(n < PERTURB_BATCH ? n : PERTURB_BATCH);
}
__device__ __forceinline__ void perturb_draw_n(const PerturbUpdate &u, RowSpan a, RowSpan b, int base, int items, int n, PerturbItems &it)
{
    if (n >= 3) perturb_draw<3>(u, a, b, base, items, it);
    else if (n == 2) perturb_draw<2>(u, a, b, base, items, it);
    else if (n == 1) perturb_draw<1>(u, a, b, base, items, it);
}
// One quad of a row from registers to its LDS slot and to the population: v[l] for l < lim.  P is even (the host's eligibility
// check, cartpole_perturb_rollout_ok) and theta is 8-byte aligned (rollout_with checks it), so a row starts 8-byte aligned at every quad, in
// LDS and in theta, and lim is 2 or 4: one or two 8-byte stores each.
__device__ __forceinline__ void perturb_store_quad(float *dst, float *row, const float (&v)[4], int lim)
{
    const float2 lo = make_float2(v[0], v[1]), hi = make_float2(v[2], v[3]);
    *reinterpret_cast<float2 *>(dst) = lo;
    if (lim > 2) *reinterpret_cast<float2 *>(dst + 2) = hi;
    *reinterpret_cast<float2 *>(row) = lo;
    if (lim > 2) *reinterpret_cast<float2 *>(row + 2) = hi;
}
// The rows of the items drawn: no array here is indexed by a run-time value, so the normals stay in registers (a loop over
// l < lim kept PerturbItems in scratch memory and waited for every 4-byte store).  The four means of a quad come by one 16-byte
// LDS read (mu_new is 16-byte aligned and holds u.P4 floats: the lanes past P of the last quad are read and never stored), the
// fma_s follow back to back in the operand order of perturb_row_quad, and the predicate l < lim guards the stores alone.
__device__ __forceinline__ void perturb_store(const PerturbUpdate &u, const float *mu_new, float *lds_rows, int base, int items, int n,
                                              const PerturbItems &it)
{
#pragma unroll
    for (int k = 0; k < PERTURB_BATCH; ++k) {
        if (k >= n || base + k * (int)blockDim.x + (int)threadIdx.x >= items) continue;
        const int q = it.q[k];
        const int lim = u.P - 4 * q < 4 ? u.P - 4 * q : 4;
        const bool mean_row = u.first_row + it.i[k] == 0;                 // global row 0 = the mean itself
        const float4 m4 = *reinterpret_cast<const float4 *>(mu_new + 4 * q);
        const float m[4] = {m4.x, m4.y, m4.z, m4.w};
        float v[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const float r = fma_(u.sigma, it.z[k][l], m[l]);
            v[l] = mean_row ? m[l] : r;
        }
        perturb_store_quad(u.theta + (size_t)it.i[k] * u.P + 4 * q, lds_rows + (size_t)it.s[k] * u.P + 4 * q, v, lim);
    }
}

template <int PLACE_DWORDS>
__device__ __forceinline__ void perturb_prologue(const PerturbUpdate &u, RowSpan a, RowSpan b, float *mu_new, float *lds_rows,
                                                 TanhEntry *tanh_lds)
{
    const int tid = (int)threadIdx.x, block = (int)blockDim.x;
    const int items = (a.rows + b.rows) * u.quads;
    UpdateOperands first{};
    if (tid < u.P) first = es_update_load(u, tid);
    const float4 *tanh_src = reinterpret_cast<const float4 *>(&SES_TANH_TABLE[0][0]);
    float4 tv{};
    if (tanh_lds && tid < SES_TANH_N) tv = tanh_src[tid];
    PerturbItems it;
    int n = perturb_batch_count(0, items);
    perturb_draw_n(u, a, b, 0, items, n, it);
    if (tanh_lds) {
        if (tid < SES_TANH_N) tanh_lds[tid] = TanhEntry{tv.x, tv.y, tv.z, tv.w};
        for (int i = tid + block; i < SES_TANH_N; i += block) {
            const float4 v = tanh_src[i];
            tanh_lds[i] = TanhEntry{v.x, v.y, v.z, v.w};
        }
    }
    perturb_update_mean(u, mu_new, &first);
    __syncthreads();
    perturb_store(u, mu_new, lds_rows, 0, items, n, it);
    for (int base = PERTURB_BATCH * block; base < items; base += PERTURB_BATCH * block) {
        n = perturb_batch_count(base, items);
        perturb_draw_n(u, a, b, base, items, n, it);
        perturb_store(u, mu_new, lds_rows, base, items, n, it);
    }
    __syncthreads();
    // WHERE the code behind the prologue lies decides its speed: the step loops of the pair kernel, moved by 4, 16 or 48 bytes, take
    // 5 % longer (0.1787 -> 0.1880 ms per generation at the headline); moved by 32 or 64 bytes they do not (NOTES.md, the serial path).
    // The compiler aligns no loop, so every edit of this prologue used to move them.  Here the code restarts on a 256-byte line, and
    // PLACE_DWORDS no-ops (the caller's constant, one per kernel instance; executed once per wave) put the loops where they were
    // measured.  After an edit of the BODY behind the prologue, look at the loop heads again (tests/test_pair_loop_placement.py).
    // Round 13: every step loop behind this point also restarts on a 32-byte line of its own plus a per-loop count (place_loop,
    // ses_policy.h; PrologueLoopPads, ses_rollout.hip), so an edit of one loop's body no longer moves the loops behind it.
    asm volatile(".p2align 8\n\t.rept %0\n\ts_nop 0\n\t.endr" ::"n"(PLACE_DWORDS));
}

}  // namespace ses
