// ses_batch_elite.hip -- the simple_evolution / simple_genetic tail of R independent trials in one set of launches
// (ses_elite_generation_batch).  The trials of a sweep sit one behind the other in one fitness vector and one population matrix,
// but unlike the openai_es batch (ses_batch.hip) they are RAGGED: trial r owns rows [row0_r, row0_r + n_r) and the parent rows
// [parent0_r, parent0_r + (1 | elite_num_r)), and n_r, elite_num_r differ between the trials.  Per trial, bit for bit what the solo
// sequence  ses_rank_center -> ses_elite_select -> ses_perturb(row_ids, parent_idx) -> [ses_elite_mean] -> ses_perturb  gives:
//
//   rank        counting rank over the trial's own rows, all keys in LDS (k_elite_rank_select_small minus the episode mean):
//               key = (ordered fitness bits, index WITHIN the trial), -0 as +0; best[r] = the fitness of rank 0
//   elites      ids[j] = the row of rank j, j < elite_num; its parent-map entry in closed form (elite_map below): no map array
//   elite row   parents_in[..] verbatim for a negative entry, else fma(pop_sigma, z(seed, gen, ids[j], quad), parents_in[..])
//   evolution   aliasing flags and state as k_elite_select; the new mu is k_elite_mean_philox's in-place sum / (float)k
//   genetic     parents_out[parent0 + j] = elite row j, best first
//   population  row i of the trial from parents_out by the same map, with next_sigma and z(seed, next_gen, i, quad)
//
// Three launches whatever R, the trial a grid dimension of each; no launch needs an order between its workgroups: no ticket
// counters, no polling.  The records are read from a table in DEVICE memory the caller wrote; the library never sees them, so
// every index a kernel derives from a record is clamped into [0, rows_total) / [0, parents_total) by trial_view() first: a wrong
// table gives wrong numbers, never an access outside the caller's buffers.
#include "ses_internal.h"
#include "ses_rng.h"
#include "ses_tail.h"

namespace ses {

constexpr int BELITE_MAX_N = 1024;              // rows per trial: one workgroup ranks a trial (elite_tail_small's limit)
constexpr long long BELITE_MAX_ROWS = 1ll << 20;

// rank_key of ses_strategy.hip, restated (it lives in that unit, not in a header)
__device__ __forceinline__ unsigned long long belite_rank_key(uint32_t u, uint32_t index)
{
    u = u == 0x80000000u ? 0u : u;                                   // -0 -> +0
    const uint32_t ordered = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)ordered << 32) | (unsigned long long)index;
}

// what the kernels are given besides their own arrays: the host's view of the table
struct BeliteShape {
    const ses_batch_elite_trial *trials;   // [R], device
    int evolution;                         // 1: simple_evolution (one parent row per trial), 0: simple_genetic (elite_num rows)
    int n_max, k_max, rows_total, parents_total;
    int P, quads;
};

// a record with every index forced inside the caller's buffers; the identity for a table that agrees with the host arguments
struct TrialView {
    int row0, n, k, parent0, per;
};
__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }
__device__ __forceinline__ TrialView trial_view(const BeliteShape &s, const ses_batch_elite_trial &tr)
{
    TrialView v;
    v.n = clampi(tr.n, 1, s.n_max);                                       // n_max <= min(1024, rows_total): checked by the host
    v.row0 = clampi(tr.row0, 0, s.rows_total - v.n);
    v.k = clampi(tr.elite_num, 1, v.n < s.k_max ? v.n : s.k_max);
    v.parent0 = clampi(tr.parent0, 0, s.parents_total - (s.evolution ? 1 : v.k));   // k_max <= parents_total: checked by the host
    v.per = v.n / v.k;                                                    // >= 1
    return v;
}

// the parent map in closed form: (parent row relative to parent0, copied verbatim?) of row i of a trial
//   evolution  _parent_map(True): [mu, elite0 = mu, then children of mu]  ->  row 0, row 1 verbatim, the others mu + noise
//   genetic    _gen_offsprings: block e = i / per starts with elite e verbatim, its children follow
__device__ __forceinline__ int elite_map(const BeliteShape &s, const TrialView &v, int i, bool &verbatim)
{
    if (s.evolution) {
        verbatim = i == 0 || i == 1;
        return 0;
    }
    int e = i / v.per;
    verbatim = i - e * v.per == 0 && e < v.k;
    return e < v.k ? e : v.k - 1;                                         // (e < k for every row of a consistent record)
}

// quad q of row `id` of a trial's population (k_perturb): parents[parent0 + map(id)] verbatim or + sigma * noise
__device__ __forceinline__ void elite_row_quad(const BeliteShape &s, const TrialView &v, const float *__restrict__ parents, int id, int q,
                                               int lim, float sigma, uint64_t seed, uint64_t gen, float row[4])
{
    bool verbatim;
    const int e = elite_map(s, v, id, verbatim);
    const float *src = parents + (size_t)(v.parent0 + e) * s.P + 4 * q;
    if (verbatim) {
        for (int l = 0; l < lim; ++l) row[l] = src[l];
        return;
    }
    float z[4];
    normal4(seed, gen, (uint32_t)id, (uint32_t)q, z);
    for (int l = 0; l < lim; ++l) row[l] = fma_(sigma, z[l], src[l]);
}

// launch 1: one workgroup per trial.  ids / flags: scratch [R][k_max]
__global__ __launch_bounds__(1024) void k_belite_rank_select(BeliteShape s, const float *__restrict__ fitness,
                                                             int32_t *__restrict__ alias_state, float *__restrict__ best,
                                                             int32_t *__restrict__ ids_out, int32_t *__restrict__ flags_out,
                                                             int32_t *__restrict__ elite_ids_out)
{
    __shared__ unsigned long long keys[BELITE_MAX_N];
    __shared__ int32_t ids[BELITE_MAX_N];
    const int r = blockIdx.x, i = threadIdx.x;
    const TrialView v = trial_view(s, s.trials[r]);                     // uniform
    float fi = 0.0f;
    if (i < v.n) {
        fi = fitness[v.row0 + i];
        keys[i] = belite_rank_key(f2u(fi), (uint32_t)i);
    }
    __syncthreads();
    if (i < v.n) {
        const unsigned long long ki = keys[i];
        int rk = 0;
        for (int j = 0; j < v.n; ++j) rk += (keys[j] > ki) ? 1 : 0;
        if (rk == 0 && best) best[r] = fi;                              // max(rewards), loop.py:82-84 `best_reward`
        if (rk < v.k) ids[rk] = i;
    }
    __syncthreads();
    const int first = ids[0];
    const int state = alias_state ? alias_state[r] : 0;
    if (i < v.k) {
        const int id = ids[i];
        ids_out[(size_t)r * s.k_max + i] = id;
        flags_out[(size_t)r * s.k_max + i] =
            (alias_state && i > 0 && state != 0 && (first == 0 || first == 1) && (id == 0 || id == 1) && id != first) ? 1 : 0;
        if (elite_ids_out) elite_ids_out[s.evolution ? (size_t)r * s.k_max + i : (size_t)(v.parent0 + i)] = id;
    }
    __syncthreads();                                            // every thread has read the old state
    if (i == 0 && alias_state) alias_state[r] = (first == 0 || (first == 1 && state != 0)) ? 1 : 0;
}

// launch 2, simple_evolution: k_elite_mean_philox per trial, one thread per (trial, quad): grid (ceil(quads / 64), R)
__global__ __launch_bounds__(64) void k_belite_mean(BeliteShape s, const int32_t *__restrict__ ids, const int32_t *__restrict__ flags,
                                                    const float *__restrict__ parents_in, float *__restrict__ parents_out)
{
    const int r = blockIdx.y, q = blockIdx.x * 64 + threadIdx.x;
    if (q >= s.quads) return;
    const ses_batch_elite_trial tr = s.trials[r];
    const TrialView v = trial_view(s, tr);
    const int lim = s.P - 4 * q < 4 ? s.P - 4 * q : 4;
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = 0; j < v.k; ++j) {
        float row[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        elite_row_quad(s, v, parents_in, ids[(size_t)r * s.k_max + j], q, lim, tr.pop_sigma, tr.seed, tr.gen, row);
        const bool alias = j > 0 && flags[(size_t)r * s.k_max + j];
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const float other = alias ? acc[l] : row[l];
            acc[l] = j == 0 ? row[l] : acc[l] + other;          // offspring_strategies.py:245  mu_param += elite_param
        }
    }
    float *dst = parents_out + (size_t)v.parent0 * s.P + 4 * q;
    for (int l = 0; l < lim; ++l) dst[l] = acc[l] / (float)v.k;          // :248  param /= self.elite_num
}

// launch 2, simple_genetic: one thread per (trial, elite, quad): grid (ceil(k_max quads / 256), R)
__global__ __launch_bounds__(256) void k_belite_gather(BeliteShape s, const int32_t *__restrict__ ids,
                                                       const float *__restrict__ parents_in, float *__restrict__ parents_out)
{
    const int r = blockIdx.y;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const int j = (int)(t / s.quads), q = (int)(t - (long long)j * s.quads);
    const ses_batch_elite_trial tr = s.trials[r];
    const TrialView v = trial_view(s, tr);
    if (j >= v.k) return;
    const int lim = s.P - 4 * q < 4 ? s.P - 4 * q : 4;
    float row[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    elite_row_quad(s, v, parents_in, ids[(size_t)r * s.k_max + j], q, lim, tr.pop_sigma, tr.seed, tr.gen, row);
    float *dst = parents_out + (size_t)(v.parent0 + j) * s.P + 4 * q;
    for (int l = 0; l < lim; ++l) dst[l] = row[l];
}

// launch 3: the next population, one thread per (trial, row < n_max, quad): grid (ceil(n_max quads / 256), R)
__global__ __launch_bounds__(256) void k_belite_population(BeliteShape s, const float *__restrict__ parents_out, float *__restrict__ theta,
                                                           unsigned long long *__restrict__ stamp)
{
    const int r = blockIdx.y;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (stamp && r == 0 && t == 0) *stamp = real_time();                 // ses_set_stamp: the next population is being written
    const int i = (int)(t / s.quads), q = (int)(t - (long long)i * s.quads);
    const ses_batch_elite_trial tr = s.trials[r];
    const TrialView v = trial_view(s, tr);
    if (i >= v.n) return;
    const int lim = s.P - 4 * q < 4 ? s.P - 4 * q : 4;
    float row[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    elite_row_quad(s, v, parents_out, i, q, lim, tr.next_sigma, tr.seed, tr.next_gen, row);
    float *dst = theta + (size_t)(v.row0 + i) * s.P + 4 * q;
    for (int l = 0; l < lim; ++l) dst[l] = row[l];
}

}  // namespace ses

extern "C" {

using namespace ses;

int ses_elite_generation_batch(ses_handle *h, int32_t strategy, const float *fitness, int32_t R, const ses_batch_elite_trial *trials,
                               int32_t n_max, int32_t k_max, int32_t rows_total, int32_t parents_total, const float *parents_in,
                               float *parents_out, int32_t *alias_state, float *theta_next, float *best, int32_t *elite_ids_out)
{
    const char *who = "ses_elite_generation_batch";
    SES_REQUIRE(h && fitness && trials && parents_in && parents_out && theta_next, "%s: null argument", who);
    SES_REQUIRE(strategy == SES_STRATEGY_SIMPLE_EVOLUTION || strategy == SES_STRATEGY_SIMPLE_GENETIC,
                "%s: strategy %d; it serves simple_evolution and simple_genetic", who, strategy);
    const bool evolution = strategy == SES_STRATEGY_SIMPLE_EVOLUTION;
    SES_REQUIRE(parents_in != parents_out, "%s: parents_in and parents_out must be distinct buffers", who);
    SES_REQUIRE(!evolution || alias_state, "%s: simple_evolution needs alias_state[R]", who);
    SES_REQUIRE(evolution || !alias_state, "%s: alias_state is simple_evolution's; pass null for simple_genetic", who);
    SES_REQUIRE(R >= 1, "%s: %d trials; there must be at least 1", who, R);
    SES_REQUIRE(R <= 65535, "%s: %d trials exceed the launch grids (65535)", who, R);
    SES_REQUIRE(n_max >= 2, "%s: n_max = %d rows; a trial has at least 2", who, n_max);
    if (n_max > BELITE_MAX_N)
        return set_error(SES_ERR_UNSUPPORTED, "%s: n_max = %d rows; one workgroup ranks a trial, up to %d rows per trial", who, n_max,
                         BELITE_MAX_N);
    SES_REQUIRE(k_max >= 1 && k_max <= n_max, "%s: k_max = %d elites outside 1 .. n_max = %d", who, k_max, n_max);
    SES_REQUIRE(rows_total <= BELITE_MAX_ROWS, "%s: %d rows in all exceed %lld", who, rows_total, BELITE_MAX_ROWS);
    SES_REQUIRE(rows_total >= n_max && (long long)rows_total >= 2ll * R && (long long)rows_total <= (long long)R * n_max,
                "%s: rows_total = %d does not fit %d trials of 2 .. n_max = %d rows", who, rows_total, R, n_max);
    if (evolution)
        SES_REQUIRE(parents_total == R, "%s: parents_total = %d; simple_evolution keeps one parent row per trial (%d)", who,
                    parents_total, R);
    else
        SES_REQUIRE(parents_total >= k_max && parents_total >= R && (long long)parents_total <= (long long)R * k_max,
                    "%s: parents_total = %d does not fit %d trials of 1 .. k_max = %d elites", who, parents_total, R, k_max);
    const int quads = (h->P + 3) / 4;
    SES_REQUIRE((long long)n_max * quads / 256 < (1ll << 31), "%s: %d rows x %d parameters exceed the launch grids", who, n_max, h->P);
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    // scratch: elite ids [R][k_max] | aliasing flags [R][k_max], at the start of the handle's reduce scratch -- over the rank vector
    // and ticket counters of the other tails' layouts, so both caches are dropped: the next solo or openai_es batch call clears
    // its rank vector itself (tail_rank_take with nothing to clear marks it "not zero")
    const size_t ids_bytes = (sizeof(int32_t) * (size_t)R * k_max + 255) / 256 * 256;
    const int rc = ensure_reduce_scratch(h, 2 * ids_bytes);
    if (rc != SES_OK) return rc;
    int32_t *ids = (int32_t *)h->red_scratch;
    int32_t *flags = (int32_t *)((char *)ids + ids_bytes);
    const int zrc = tail_rank_take(h, ids, 0);
    if (zrc != SES_OK) return zrc;
    h->counter_armed = nullptr;
    const BeliteShape s{trials, evolution ? 1 : 0, n_max, k_max, rows_total, parents_total, h->P, quads};
    hipLaunchKernelGGL(k_belite_rank_select, dim3(R), dim3(1024), 0, h->stream, s, fitness, alias_state, best, ids, flags, elite_ids_out);
    if (evolution)
        hipLaunchKernelGGL(k_belite_mean, dim3(ceil_div(quads, 64), R), dim3(64), 0, h->stream, s, ids, flags, parents_in, parents_out);
    else
        hipLaunchKernelGGL(k_belite_gather, dim3(ceil_div((long long)k_max * quads, 256), R), dim3(256), 0, h->stream, s, ids, parents_in,
                           parents_out);
    hipLaunchKernelGGL(k_belite_population, dim3(ceil_div((long long)n_max * quads, 256), R), dim3(256), 0, h->stream, s, parents_out,
                       theta_next, h->stamp);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

}  // extern "C"
