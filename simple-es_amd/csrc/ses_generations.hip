// ses_generations.hip -- k whole generations in ONE call of the C ABI (ses_run_generations).
//
// The reference's generation loop (learning_strategies/evolution/loop.py:61-104) runs one `p.map(RolloutWorker, ...)`
// and one `strategy.evaluate(results)` per generation from Python.  On the device a generation of the reference's own
// configs (96-240 offspring) is 60-120 us of kernels, and the Python host needs ~96 us to enqueue it (ctypes calls,
// tensor bookkeeping): conf/cartpole.yaml and conf/simplespread.yaml ran at half the device's speed.  This file is the
// same sequence of entry points -- resets, fused rollout, episode mean, the strategy's tail, the next population --
// issued from C with the host-side scalars of the strategies (sigma decay, Adam's step scale, generation keys) advanced
// exactly as the Python classes advance them (double arithmetic, same libm pow / sqrt), so a run through this call is
// bit-identical to the per-generation path (tests/test_gpu_host_mirror.py).  No kernel lives here.
//
// How it reads: check_gen_state() validates, make_plan() decides once per call what is fused (LoopPlan), one tail_*() per
// strategy advances that strategy's host scalars and makes its call, and the loop is resets, rollout, exchange, tail, flip.
// What a generation fuses across its entry points travels in ARGUMENTS (RolloutOpts, OpenaiTailOpts: ses_internal.h) and in
// locals of ses_run_generations -- the update a tail leaves to the next rollout among them -- so nothing of one call, or of
// one generation, outlives it in the handle.  The handle fields this file still writes are h->stamp (saved and restored: the
// public ses_set_stamp slot) and the reset buffer it owns (gen_init).
#include <cmath>
#include <cstring>

#include "ses_internal.h"

namespace ses {

// Adam's step scale at update st->adam_t (optimizers.py:43-47 via Adam.next_step_scale())
static double adam_step_scale(const ses_gen_state *st)
{
    const double t = (double)st->adam_t;
    return st->learning_rate * std::sqrt(1.0 - std::pow(0.999, t)) / (1.0 - std::pow(0.99, t));
}

// the strategies whose tail has no multi-GPU form inside this loop
static int one_gpu_only(const char *strategy, const char *entry, int world)
{
    return set_error(SES_ERR_UNSUPPORTED, "ses_run_generations: %s runs on one GPU here (world = %d): call %s per generation on every rank",
                     strategy, world, entry);
}

// everything about `st` that does not depend on the generation: the per-strategy buffers, the shard layout
static int check_gen_state(const ses_handle *h, const ses_gen_state *st)
{
    SES_REQUIRE(st->strategy == SES_STRATEGY_OPENAI_ES || st->strategy == SES_STRATEGY_SIMPLE_EVOLUTION ||
                    st->strategy == SES_STRATEGY_SIMPLE_GENETIC || st->strategy == SES_STRATEGY_PGPE ||
                    st->strategy == SES_STRATEGY_SEP_CMA_ES || st->strategy == SES_STRATEGY_LM_MA_ES ||
                    st->strategy == SES_STRATEGY_MA_ES || st->strategy == SES_STRATEGY_ARS,
                "ses_run_generations: unknown strategy %d", st->strategy);
    SES_REQUIRE(st->n >= 2 && (st->cur == 0 || st->cur == 1), "ses_run_generations: bad population size / buffer index");
    SES_REQUIRE(st->theta[0] && st->theta[1] && st->parents[0] && st->parents[1] && st->fitness && st->init,
                "ses_run_generations: null buffer");
    switch (st->strategy) {
        case SES_STRATEGY_MA_ES:
            SES_REQUIRE(st->ma_ps[0] && st->ma_ps[1] && st->ma_M[0] && st->ma_M[1] && st->ma_step[0] && st->ma_step[1] && st->ma_D[0] &&
                            st->ma_D[1] && st->ma_weights,
                        "ses_run_generations: ma_es needs the path, matrix, step and D buffers and the weight table");
            if (st->world > 1) return one_gpu_only("ma_es", "ses_maes_generation", st->world);
            break;
        case SES_STRATEGY_LM_MA_ES:
            SES_REQUIRE(st->lm_ps[0] && st->lm_ps[1] && st->lm_step[0] && st->lm_step[1] && st->lm_weights &&
                            (st->lm.m == 0 || (st->lm_M[0] && st->lm_M[1])),
                        "ses_run_generations: lm_ma_es needs the path, vector and step buffers and the weight table");
            if (st->world > 1) return one_gpu_only("lm_ma_es", "ses_lmma_generation", st->world);
            break;
        case SES_STRATEGY_SEP_CMA_ES:
            SES_REQUIRE(st->cma_C[0] && st->cma_C[1] && st->cma_ps[0] && st->cma_ps[1] && st->cma_pc[0] && st->cma_pc[1] &&
                            st->cma_step[0] && st->cma_step[1] && st->cma_weights,
                        "ses_run_generations: sep_cma_es needs the variance, path and step buffers and the weight table");
            if (st->world > 1) return one_gpu_only("sep_cma_es", "ses_sepcma_generation", st->world);
            break;
        case SES_STRATEGY_ARS:
            SES_REQUIRE(st->n % 2 == 0 && st->ars_b >= 1 && st->ars_b <= st->n / 2,
                        "ses_run_generations: ars needs an even population and 1 <= ars_b <= n / 2");
            if (st->world > 1) return one_gpu_only("ars", "ses_ars_generation", st->world);
            break;
        case SES_STRATEGY_PGPE:
            SES_REQUIRE(st->adam_m[0] && st->adam_m[1] && st->adam_v[0] && st->adam_v[1] && st->scale[0] && st->scale[1],
                        "ses_run_generations: pgpe needs the Adam and the scale buffers");
            if (st->world > 1) return one_gpu_only("pgpe", "ses_pgpe_generation", st->world);
            break;
        case SES_STRATEGY_OPENAI_ES:
            SES_REQUIRE(st->adam_m[0] && st->adam_m[1] && st->adam_v[0] && st->adam_v[1], "ses_run_generations: openai_es needs the Adam buffers");
            break;
        default:
            SES_REQUIRE(st->elite_num >= 1 && st->elite_num <= st->n && st->elite_num <= 1024 && st->parent_map && st->work_i32 &&
                            st->work_f32, "ses_run_generations: elite strategies need elite_num, parent_map and the work buffers");
            SES_REQUIRE(st->strategy != SES_STRATEGY_SIMPLE_EVOLUTION || st->alias_state, "ses_run_generations: simple_evolution needs alias_state");
            break;
    }
    // sharded run (one process per GPU): this rank rolls out its own rows, the fitness shards are all-gathered INSIDE the loop
    // (both transports of ses_allgather_fitness are plain stream enqueues), the strategy's tail follows
    if (st->world > 1) {
        SES_REQUIRE(st->comm && st->fit_local, "ses_run_generations: a sharded run needs the transport handle and fit_local");
        SES_REQUIRE(st->per_rank >= 1 && (int64_t)st->per_rank * st->world >= st->n && st->first_row >= 0 &&
                        st->first_row % st->per_rank == 0 && st->first_row / st->per_rank < st->world,
                    "ses_run_generations: bad shard layout (%d ranks x %d rows for %d)", st->world, st->per_rank, st->n);
        const int64_t left = (int64_t)st->n - st->first_row;
        SES_REQUIRE(st->n_local == (int32_t)(left <= 0 ? 0 : left < st->per_rank ? left : st->per_rank),
                    "ses_run_generations: n_local %d is not this rank's share of %d rows", st->n_local, st->n);
        SES_REQUIRE(st->comm->stream == h->stream, "ses_run_generations: the transport handle must share the stream");
    }
    return SES_OK;
}

// what one call decides once, for all its generations
struct LoopPlan {
    bool multi;              // one process per GPU: this rank rolls out rows [first, first + n_loc)
    int n_loc;               // rows of theta / init on this rank
    int64_t first;
    bool sharded_tail;       // openai_es in shard form (ses_openai_sharded_ok)
    // ... and then the fitness exchange itself needs no launch: the episode-mean kernel stores every value as a granule into every
    // rank's mailbox, the rank kernel of the tail polls the tiles it sorts (k_fitness_mean_granules, k_rank_sort_search<true>)
    // (up to 8192 rows the counting rank polls them, k_rank_count_granules: also where the tail runs replicated, e.g. 4096 rows in
    //  total over 8 ranks)
    bool fused_fit;
    // one GPU, openai_es, counting rank (up to 8192 rows): the episode mean is formed inside the rank count (k_rank_count_episodes)
    // -- the rollout leaves the per-episode returns, no mean kernel between the rollout and the tail
    bool fused_mean;
    // one GPU, elite strategies, up to 512 rows (the reference's own configs: 97 - 257): mean + rank + best + selection in ONE
    // launch, simple_evolution's elite rows + their mean in a second (elite_tail_small) instead of seven
    bool fused_elite;
    // one GPU, replicated openai_es tail: between two generations of THIS call the launch that applies the update and writes the next
    // population (k_es_apply_perturb) is left to the rollout that runs that population, where its kernel can form its own rows
    // (cartpole_perturb_rollout_ok decides per generation; the call's last generation launches it, so that theta, mu, m and v are
    // complete when the call returns)
    bool defer_perturb;
    // The env resets depend on (env seed, generation key) only: those of all k generations are drawn up front in ONE launch
    // (keyed like ESLoop._init_states), into a buffer the handle owns -- a 4 us kernel per generation less on the
    // critical path (the Python loop hides it on a side stream).  Above 64 MB the chunk is drawn generation by generation
    // into the caller's st->init instead.
    int init_rows;
    size_t slice;            // floats of one generation's resets
    bool ahead;
};

static LoopPlan make_plan(ses_handle *h, const ses_gen_state *st, int k)
{
    LoopPlan p{};
    const int n = st->n;
    const bool openai = st->strategy == SES_STRATEGY_OPENAI_ES;
    const bool elite = st->strategy == SES_STRATEGY_SIMPLE_EVOLUTION || st->strategy == SES_STRATEGY_SIMPLE_GENETIC;
    p.multi = st->world > 1;
    p.n_loc = p.multi ? st->n_local : n;
    p.first = p.multi ? st->first_row : 0;
    p.sharded_tail = p.multi && openai && ses_openai_sharded_ok(h, st->comm, n, st->per_rank, st->world) == 1;
    p.fused_fit = p.multi && openai && openai_fused_fitness_ok(h, n, st->per_rank, p.sharded_tail ? st->per_rank : n) == 1;   // (the slot size, not this rank's rows: a ragged last rank must decide like the others)
    p.fused_mean = !p.multi && openai && h->tune.fused_mean && n <= 8192;
    p.fused_elite = !p.multi && elite && h->tune.fused_elite && n <= 512;   // (one workgroup counts: 512 rows = 8 waves x 512 compares)
    p.defer_perturb = !p.multi && openai && h->tune.fused_perturb_rollout;
    p.init_rows = st->shared_init ? 1 : (p.n_loc > 0 ? p.n_loc : 1);
    p.slice = (size_t)p.init_rows * h->cfg.eval_ep_num * st->init_width;
    p.ahead = p.slice * (size_t)k * sizeof(float) <= (64u << 20);
    return p;
}

// the resets of all k generations in one launch, into the handle's buffer (p.ahead)
static int draw_resets_ahead(ses_handle *h, const ses_gen_state *st, const LoopPlan &p, int k)
{
    if (h->gen_init_cap < p.slice * (size_t)k) {
        if (h->gen_init) { SES_HIP_TRY(hipStreamSynchronize(h->stream)); SES_HIP_TRY(hipFree(h->gen_init)); }
        h->gen_init = nullptr; h->gen_init_cap = 0;
        SES_HIP_TRY(hipMalloc(&h->gen_init, p.slice * (size_t)k * sizeof(float)));
        h->gen_init_cap = p.slice * (size_t)k;
    }
    return ses_init_states_uniform_gens(h, st->env_seed, st->pop_gen, k, st->shared_init ? 0 : p.first, p.init_rows, st->shared_init,
                                        st->init_width, st->init_lo, st->init_hi, h->gen_init);
}

// one generation of the call: the buffer halves it reads and writes, where its best reward and its two time stamps go
struct GenSlot {
    int cur, nxt;
    float *best;
    unsigned long long *rollout_stamp, *tail_stamp;     // end of the rollout phase, end of the tail (or null)
};

// ---- the tails: each advances its strategy's host scalars as the Python class does and makes the strategy's call ------------------
// WHEN the scalars move differs on purpose.  openai_es, pgpe and ars (and the elite strategies) advance adam_t and sigma BEFORE the call,
// as their classes do before they enqueue, and the loop flips the buffers also behind a refused call; sep_cma_es and lm_ma_es
// advance them only once the call was accepted, so that a refused generation leaves counter, sigma and buffer index with the device
// state (advances_when_accepted() is what the loop asks before the flip); ma_es does as they do.
static bool advances_when_accepted(int strategy)
{
    return strategy == SES_STRATEGY_SEP_CMA_ES || strategy == SES_STRATEGY_LM_MA_ES || strategy == SES_STRATEGY_MA_ES;
}

// optimizers.py:43-47 via Adam.next_step_scale(); offspring_strategies.py _evaluate_fused.  fit_view: the granule exchange the
// rollout fed (or null); defer_to: where the update may be left to the next rollout (null in the call's last generation);
// *deferred: it was
static int tail_openai(ses_handle *h, ses_gen_state *st, const LoopPlan &p, const GenSlot &g, const P2pGranuleView *fit_view,
                       PerturbUpdate *defer_to, bool *deferred)
{
    const int cur = g.cur, nxt = g.nxt;
    st->adam_t += 1;
    const double a = adam_step_scale(st);
    const double sigma = st->sigma;
    st->sigma = st->sigma * st->sigma_decay;
    h->stamp = g.tail_stamp;
    OpenaiTailOpts o{};
    if (fit_view) { o.granules = fit_view; o.own_fitness = st->fit_local; o.slot_rows = st->per_rank; }
    if (p.fused_mean) { o.episodes = h->ep_return; o.episodes_stamp = g.rollout_stamp; }
    int rc;
    if (p.sharded_tail) {
        rc = openai_generation_impl(h, st->comm, st->fitness, st->n, st->seed, st->pop_gen, st->learning_rate, sigma, a, st->parents[cur],
                                    st->adam_m[cur], st->adam_v[cur], st->parents[nxt], st->adam_m[nxt], st->adam_v[nxt], (float)st->sigma,
                                    st->pop_gen + 1, p.first, p.n_loc, st->per_rank, st->world, st->theta[nxt], g.best, o, deferred);
    } else {
        o.defer_to = defer_to;
        o.next_mode = st->mode;
        rc = openai_generation_impl(h, nullptr, st->fitness, st->n, st->seed, st->pop_gen, st->learning_rate, sigma, a, st->parents[cur],
                                    st->adam_m[cur], st->adam_v[cur], st->parents[nxt], st->adam_m[nxt], st->adam_v[nxt], (float)st->sigma,
                                    st->pop_gen + 1, p.n_loc > 0 ? p.first : 0, p.n_loc, 0, 1, st->theta[nxt], g.best, o, deferred);
    }
    st->pop_sigma = st->sigma;
    return rc;
}

// Adam's step scale; curr_sigma decays after every evaluate
static int tail_pgpe(ses_handle *h, ses_gen_state *st, const GenSlot &g)
{
    const int cur = g.cur, nxt = g.nxt;
    st->adam_t += 1;
    const double a = adam_step_scale(st);
    const double sigma = st->sigma;
    st->sigma = st->sigma * st->sigma_decay;
    h->stamp = g.tail_stamp;
    const int rc = ses_pgpe_generation(h, st->fitness, st->n, st->seed, st->pop_gen, sigma, a, st->sigma_learning_rate, st->sigma_max_change,
                                       st->scale_lo, st->scale_hi, st->parents[cur], st->adam_m[cur], st->adam_v[cur], st->scale[cur],
                                       st->parents[nxt], st->adam_m[nxt], st->adam_v[nxt], st->scale[nxt], (float)st->sigma,
                                       st->pop_gen + 1, 0, st->n, st->theta[nxt], g.best, nullptr, nullptr);
    st->pop_sigma = st->sigma;
    return rc;
}

// curr_sigma decays after every evaluate; the step (learning_rate / (b sigma_R)) is formed on the device: no scalar comes back
static int tail_ars(ses_handle *h, ses_gen_state *st, const GenSlot &g)
{
    const int cur = g.cur, nxt = g.nxt;
    const double sigma = st->sigma;
    st->sigma = st->sigma * st->sigma_decay;
    h->stamp = g.tail_stamp;
    const int rc = ses_ars_generation(h, st->fitness, st->n, st->ars_b, st->seed, st->pop_gen, sigma, st->learning_rate, st->parents[cur],
                                      st->parents[nxt], (float)st->sigma, st->pop_gen + 1, 0, st->n, st->theta[nxt], g.best, nullptr,
                                      nullptr);
    st->pop_sigma = st->sigma;
    return rc;
}

// the update counter, hsig_scale of this update, curr_sigma
static int tail_sepcma(ses_handle *h, ses_gen_state *st, const GenSlot &g)
{
    const int cur = g.cur, nxt = g.nxt;
    const int64_t t = st->adam_t + 1;
    const double hsig_scale = 1.0 / std::sqrt(1.0 - std::pow(1.0 - st->cma.c_sigma, 2.0 * (double)t));
    const double sigma = st->sigma, next_sigma = st->sigma * st->sigma_decay;
    h->stamp = g.tail_stamp;
    const int rc = ses_sepcma_generation(h, st->fitness, st->n, st->seed, st->pop_gen, sigma, hsig_scale, &st->cma, st->cma_weights,
                                         st->parents[cur], st->cma_C[cur], st->cma_ps[cur], st->cma_pc[cur], st->cma_step[cur],
                                         st->parents[nxt], st->cma_C[nxt], st->cma_ps[nxt], st->cma_pc[nxt], st->cma_step[nxt],
                                         (float)next_sigma, st->pop_gen + 1, 0, st->n, st->theta[nxt], g.best, nullptr, nullptr, nullptr);
    if (rc != SES_OK) return rc;
    st->adam_t = t;
    st->sigma = next_sigma;
    st->pop_sigma = st->sigma;
    return SES_OK;
}

// the update counter (it decides how many direction vectors the evaluated and the next population use) and curr_sigma
static int tail_lmma(ses_handle *h, ses_gen_state *st, const GenSlot &g)
{
    const int cur = g.cur, nxt = g.nxt;
    const int64_t t = st->adam_t;
    const int32_t m_active = (int32_t)(t < st->lm.m ? t : st->lm.m), m_next = (int32_t)(t + 1 < st->lm.m ? t + 1 : st->lm.m);
    const double sigma = st->sigma, next_sigma = st->sigma * st->sigma_decay;
    h->stamp = g.tail_stamp;
    const int rc = ses_lmma_generation(h, st->fitness, st->n, st->seed, st->pop_gen, sigma, &st->lm, st->lm_weights, m_active, m_next,
                                       st->parents[cur], st->lm_ps[cur], st->lm_M[cur], st->lm_step[cur], st->parents[nxt],
                                       st->lm_ps[nxt], st->lm_M[nxt], st->lm_step[nxt], (float)next_sigma, st->pop_gen + 1, 0, st->n,
                                       st->theta[nxt], g.best, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc != SES_OK) return rc;
    st->adam_t = t + 1;
    st->sigma = next_sigma;
    st->pop_sigma = st->sigma;
    return SES_OK;
}

// the update counter and curr_sigma; D of the evaluated population goes in, D of the next one comes out
static int tail_maes(ses_handle *h, ses_gen_state *st, const GenSlot &g)
{
    const int cur = g.cur, nxt = g.nxt;
    const double sigma = st->sigma, next_sigma = st->sigma * st->sigma_decay;
    h->stamp = g.tail_stamp;
    const int rc = ses_maes_generation(h, st->fitness, st->n, st->seed, st->pop_gen, sigma, &st->ma, st->ma_weights, st->parents[cur],
                                       st->ma_ps[cur], st->ma_M[cur], st->ma_step[cur], st->ma_D[cur], st->parents[nxt], st->ma_ps[nxt],
                                       st->ma_M[nxt], st->ma_step[nxt], (float)next_sigma, st->pop_gen + 1, 0, st->n, st->theta[nxt],
                                       st->ma_D[nxt], g.best, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc != SES_OK) return rc;
    st->adam_t += 1;
    st->sigma = next_sigma;
    st->pop_sigma = st->sigma;
    return SES_OK;
}

// simple_evolution and simple_genetic: rank, select the elites, rebuild their rows, draw the next population from them
static int tail_elite(ses_handle *h, ses_gen_state *st, const LoopPlan &p, const GenSlot &g)
{
    const int cur = g.cur, nxt = g.nxt, n = st->n, ke = st->elite_num;
    int32_t *rank = st->work_i32, *ids = rank + n, *pidx = ids + ke, *alias = pidx + ke;
    const bool evo = st->strategy == SES_STRATEGY_SIMPLE_EVOLUTION;
    int rc;
    if (p.fused_elite) {
        rc = elite_tail_small(h, h->ep_return, n, ke, st->parent_map, evo ? st->alias_state : nullptr, rank, st->fitness, g.best,
                              ids, pidx, evo ? alias : nullptr, g.rollout_stamp, st->parents[cur], (float)st->pop_sigma, st->seed,
                              st->pop_gen, evo ? st->parents[nxt] : nullptr);
    } else {
        rc = ses_rank_center(h, st->fitness, n, rank, nullptr, g.best);
        if (rc == SES_OK)
            rc = ses_elite_select(h, rank, n, ke, st->parent_map, evo ? st->alias_state : nullptr, ids, pidx, evo ? alias : nullptr);
    }
    h->stamp = nullptr;                                                         // the elite rows are not "the next population"
    // the elite rows of the CURRENT population, rebuilt from (parents, parent map entry, row id): _select_elites
    float *rows = evo ? st->work_f32 : st->parents[nxt];
    if (rc == SES_OK && !(p.fused_elite && evo))
        rc = ses_perturb(h, st->parents[cur], pidx, ids, (float)st->pop_sigma, st->seed, st->pop_gen, 0, ke, rows);
    if (evo) {
        // mu = elite[0] = the reference's in-place elite sum (offspring_strategies.py:234-248), sigma decays BEFORE the
        // next population is drawn
        if (rc == SES_OK && !p.fused_elite) rc = ses_elite_mean(h, rows, alias, ke, st->parents[nxt]);
        st->sigma = st->sigma * st->sigma_decay;
        st->pop_sigma = st->sigma;
    } else {
        // simple_genetic: the elites are the parents; sigma decays AFTER regeneration (offspring_strategies.py:117-124)
        st->pop_sigma = st->sigma;
        st->sigma = st->sigma * st->sigma_decay;
    }
    h->stamp = g.tail_stamp;
    if (rc == SES_OK && p.n_loc > 0)
        rc = ses_perturb(h, st->parents[nxt], st->parent_map + p.first, nullptr, (float)st->pop_sigma, st->seed, st->pop_gen + 1,
                         p.first, p.n_loc, st->theta[nxt]);
    return rc;
}

}  // namespace ses

extern "C" {

int ses_run_generations(ses_handle *h, ses_gen_state *st, int32_t k, float *best, uint64_t *stamps)
{
    using namespace ses;
    SES_REQUIRE(h && st && best, "ses_run_generations: null argument");
    SES_REQUIRE(k >= 1, "ses_run_generations: k must be >= 1");
    int rc = check_gen_state(h, st);
    if (rc != SES_OK) return rc;
    const LoopPlan p = make_plan(h, st, k);
    unsigned long long *const saved_stamp = h->stamp;
    // The update that the openai_es tail of generation g left to the rollout of generation g + 1 (p.defer_perturb): `carried` points
    // at it from the tail that recorded it to the rollout that took it -- or to the exit below, after an error in between.
    PerturbUpdate update{};
    const PerturbUpdate *carried = nullptr;
    if (p.ahead) rc = draw_resets_ahead(h, st, p, k);
    for (int g = 0; g < k && rc == SES_OK; ++g) {
        const GenSlot slot{st->cur, st->cur ^ 1, best + g, stamps ? (unsigned long long *)(stamps + 2 * g) : nullptr,
                           stamps ? (unsigned long long *)(stamps + 2 * g + 1) : nullptr};
        // resets
        const float *init = st->init;
        if (p.ahead) {
            init = h->gen_init + p.slice * (size_t)g;
        } else {
            rc = ses_init_states_uniform(h, st->env_seed, st->pop_gen, st->shared_init ? 0 : p.first, p.init_rows, st->shared_init,
                                         st->init_width, st->init_lo, st->init_hi, st->init);
            if (rc != SES_OK) break;
        }
        // rollout (+ the episode mean, unless the tail forms it; + the fitness exchange, where the mean kernel feeds it)
        const bool leave_episodes = p.fused_mean || p.fused_elite;
        h->stamp = leave_episodes ? nullptr : slot.rollout_stamp;                       // (the tail's first kernel writes that stamp then)
        P2pGranuleView fit_view;
        bool fused = false;
        if (p.fused_fit) {
            const int grc = comm_p2p_granules_begin(st->comm, st->per_rank, &fit_view);
            if (grc == SES_ERR_COMM) { rc = grc; break; }
            fused = grc == SES_OK;                                                      // (unsupported: RCCL only, or granules switched off)
        }
        if (p.n_loc > 0) {
            RolloutOpts ro{leave_episodes, fused ? &fit_view : nullptr, carried};
            rc = rollout_with(h, st->theta[slot.cur], init, st->shared_init ? 0 : 1, p.n_loc, st->mode,
                              p.multi ? st->fit_local : st->fitness, nullptr, nullptr, ro);
            carried = ro.apply_first;
        }
        if (rc != SES_OK) break;
        // exchange
        if (p.multi && !fused) {
            // loop.py:66-79, the gather half of Pool.map: fitness[r * per_rank + i] = rank r's fit_local[i] (a ragged last
            // shard ends in the -inf the caller put there once)
            rc = ses_allgather_fitness(st->comm, st->fit_local, st->per_rank, st->fitness);
            if (rc != SES_OK) break;
        }
        // tail
        bool deferred = false;
        switch (st->strategy) {
            case SES_STRATEGY_OPENAI_ES:
                rc = tail_openai(h, st, p, slot, fused ? &fit_view : nullptr, p.defer_perturb && g < k - 1 ? &update : nullptr, &deferred);
                if (deferred) carried = &update;
                break;
            case SES_STRATEGY_PGPE: rc = tail_pgpe(h, st, slot); break;
            case SES_STRATEGY_SEP_CMA_ES: rc = tail_sepcma(h, st, slot); break;
            case SES_STRATEGY_LM_MA_ES: rc = tail_lmma(h, st, slot); break;
            case SES_STRATEGY_MA_ES: rc = tail_maes(h, st, slot); break;
            case SES_STRATEGY_ARS: rc = tail_ars(h, st, slot); break;
            default: rc = tail_elite(h, st, p, slot); break;
        }
        if (rc != SES_OK && advances_when_accepted(st->strategy)) break;
        // flip
        st->pop_gen += 1;
        st->cur = slot.nxt;
    }
    if (carried) {                                                     // (only after an error: no rollout took the deferred launch)
        const int frc = launch_apply_perturb(h, *carried);
        if (rc == SES_OK) rc = frc;
    }
    h->stamp = saved_stamp;
    return rc;
}

}  // extern "C"
