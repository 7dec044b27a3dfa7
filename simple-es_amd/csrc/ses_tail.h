// ses_tail.h -- where a ranked tail starts: the constants of the rank kernels and the front end that the tails of pgpe, sep_cma_es and
// lm_ma_es share (defined in ses_strategy.hip, next to the rank kernels).  The handle's "this rank vector is known to be zero" cache
// (ses_handle::rank_zeroed, rank_zeroed_n) is kept by ONE pair of helpers, tail_rank_take / tail_rank_cleared, for those tails and for
// openai_generation_impl's own layouts; the ticket-counter cache (counter_armed) stays with each caller: they differ there on purpose.
#pragma once
#include "ses_internal.h"

namespace ses {

constexpr int RANK_TILE = 1024;        // keys per sorted tile (k_rank_tile_sort, k_rank_search)
constexpr int RANK_SORT_MIN = 8192;    // populations above this many rows are ranked by sort + search, the others by counting
constexpr int SEPCMA_CHUNK = 1024;     // rows per workgroup of k_sepcma_sums_partial

// the j-slice of the counting rank: ~2048 workgroups, jt = n^2 / (256 * 2048) rounded up to a multiple of 64, in [64, 8192]
inline int rank_count_slice(int n)
{
    const long long jt = ((long long)n * n / (256ll * 2048ll) + 63) / 64 * 64;
    return (int)(jt < 64 ? 64 : jt > 8192 ? 8192 : jt);
}

// The checks every such tail makes of its population and of the rows it draws next: n >= 4 (and even, where the rows come in
// pairs), the shard [first_row, first_row + n_rows) inside the population, theta_next where there are rows to write.
int tail_check_rows(const char *who, int n, bool even, int64_t first_row, int n_rows, const float *theta_next);

// Ranks fitness[0 .. n) into a zeroed vector of the handle's scratch, laid out  sorted tiles (n > RANK_SORT_MIN only) | rank,
// rounded up to 256 bytes | extra_bytes of the caller's  -- the rank vector sits where ses_openai_generation keeps its own for
// the same n, so one cache serves every tail.  Takes the vector (tail_rank_take) and drops the ticket-counter cache (the caller's
// bytes may lie over another layout's counters).  Rule: rank[i] = #{ j : f[j] > f[i] or (f[j] == f[i] and j > i) }.
int tail_rank_begin(ses_handle *h, const float *fitness, int n, size_t extra_bytes, int32_t **rank, void **extra);
// The "known to be zero" protocol of a rank vector in the handle's scratch.  take: memsets rank[0 .. n) unless the cache says it is
// zero, then marks it "not zero" -- it holds counts from here on, and an early return of the caller leaves it so.  cleared: call
// after the launch that writes the next population and clears rank[0 .. n) again (rank_to_clear, n_clear of the perturb kernels)
int tail_rank_take(ses_handle *h, int32_t *rank, int n);
void tail_rank_cleared(ses_handle *h, int32_t *rank, int n);

// the weighted sums of ses_sepcma.hip, which ses_lmma.hip launches as they are
__global__ void k_sepcma_sums_partial(const int32_t *__restrict__ rank, const float *__restrict__ fitness, int n, int mu,
                                      const float *__restrict__ weights, uint64_t seed, uint64_t gen, int P4, int chunks,
                                      float *__restrict__ partial, float *__restrict__ best);

// the per-trial counting rank of ses_batch.hip (grid (R, ceil(n / 256), ceil(n / jt)), trial r's rows at r n; rank_all zero on
// entry), which ses_batch_sepcma.hip launches as it is
__global__ void k_batch_rank_count(const float *__restrict__ fit_all, int n, int jt, int32_t *__restrict__ rank_all);

// the pair scores of ses_ars.hip (scores[j] = max(fitness[2 j], fitness[2 j + 1]), j < m), which ses_batch_ars.hip launches as it is
// over the R m pairs of a batch
__global__ void k_ars_scores(const float *__restrict__ fitness, int m, float *__restrict__ scores);

}  // namespace ses
