// ses_internal.h -- handle layout and error plumbing shared by the translation units of libses_hip.so
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <type_traits>

#include "../../include/ses.h"
#include "ses_rollout_plan.h"

namespace ses {
struct P2pGranuleView;
// What the launch that ends an openai_es generation is given (k_es_apply_perturb): the chunk partials of the gradient, the
// Adam step, the vectors it reads and writes, and the population it draws.  Between two generations of one ses_run_generations call
// the tail hands it to the loop instead of launching it when the NEXT rollout can form its own rows from it (OpenaiTailOpts,
// RolloutOpts below; ses_perturb_prologue.h).
struct PerturbUpdate {
    const float *partial;
    int chunks, P4;
    float update_factor;
    double adam_a;
    const float *mu_in, *m_in, *v_in;
    float *mu_out, *m_out, *v_out;
    float sigma;
    uint64_t seed, gen;
    long long first_row;
    int n_rows, P, quads;
    float *theta;
    unsigned long long *stamp;
    int32_t *rank_to_clear;
    int n_clear;
};
}  // namespace ses
struct ses_handle {
    ses_config cfg;
    hipStream_t stream;
    int P;               // parameters per offspring
    uint32_t obs_mask;   // bit k set: observation component k is zeroed (POMDP wrappers)
    // scratch owned by the handle (grown on demand, never shrunk)
    double *ep_return;   // [rows * E]
    int32_t *ep_steps;   // [rows * E]
    size_t ep_cap;       // capacity in episodes
    void *red_scratch;   // rank keys (u64[n]) followed by es_update partial sums
    size_t red_cap;      // bytes
    float *gen_init;     // ses_run_generations: the env resets of a chunk of generations, drawn in one launch
    size_t gen_init_cap; // floats
    // multi-GPU (ses_comm.hip): RCCL communicator of this rank, null until ses_comm_init
    void *comm;
    int comm_rank, comm_world;
    // peer-store transport of the same exchange (ses_comm_p2p_*): this rank's mailbox and the peers' mapped ones
    struct ses_p2p *p2p;
    ses::Tuning tune;    // the knobs (ses_set_tuning): names, defaults, ranges and comments in ses_tuning.h
    // ses_set_stamp: where the next stamped launch of this handle writes the GPU real-time counter (or null)
    unsigned long long *stamp;
    // ses_openai_generation: the rank vector in red_scratch that is known to be zero (left so by the update kernel)
    int32_t *rank_zeroed;
    int rank_zeroed_n;
    unsigned int *counter_armed;   // the last-block ticket counter in red_scratch that is known to be zero
    int lds_per_cu;                // hipDeviceAttributeMaxSharedMemoryPerMultiprocessor of the handle's device
    int env_step_key[3];           // (block, lds knob, waves knob) the two values below were resolved for
    int env_step_lds_resolved;     // the reservation actually launched with
    int env_step_wpc;              // waves per CU the occupancy calculator gives that shape
    long long count_pair_rollouts;         // launches of the light + heavy pair kernel by this handle, either form ...
    long long count_perturb_rollouts;      // ... those that formed their own rows (the prologue form)
    long long count_apply_perturb;         // launches of k_es_apply_perturb
    // ses_obs_norm_bind: the caller's normaliser state (null: nothing bound) and whether rollouts accumulate and merge into it;
    // the per-env partials of a rollout, float64[2S + 1, episodes], are the handle's own (grown on demand, never shrunk)
    double *obs_norm_stats;
    float *obs_norm_affine;
    int obs_norm_update;
    double *obs_norm_partials;
    size_t obs_norm_cap;                 // capacity in doubles
};

namespace ses {

// the constant-rate (100 MHz) real-time counter shared by the whole GPU: timestamps taken inside kernels are
// comparable across kernels, streams and handles
__device__ __forceinline__ unsigned long long real_time() { return wall_clock64(); }

#define SES_HIP_TRY(expr)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return ::ses::set_error(SES_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                    __FILE__, __LINE__);                                           \
    } while (0)

#define SES_REQUIRE(cond, ...)                                             \
    do {                                                                   \
        if (!(cond)) return ::ses::set_error(SES_ERR_INVALID_ARG, __VA_ARGS__); \
    } while (0)

// ---- runtime value -> template constant, and the launch of a rollout kernel --------------------------------------------
// f is a generic lambda: it gets the value as a std::integral_constant and names the kernel instance with it.
// THE ORDER IN WHICH THESE HELPERS VISIT THEIR CONSTANTS, AND THE ORDER OF THEIR CALLS IN THE HOST CODE, IS LOAD-BEARING.
// hipcc emits implicitly instantiated kernels in the order of their first use in the host code (depth first through the
// host templates that use them), and kernels that read the tanh table or call the Box2D routines reach them PC-relative:
// their machine code holds the distance to .rodata, i.e. depends on every kernel emitted before them.  Swapping two
// constants of a with_lanes<...> list, two branches that name kernels, or two host functions of a unit therefore changes
// kernel hashes (tools/kernel_hash.py) -- the ones profiles/*.json carry, which tests/test_profiles_current.py compares and
// without which bench.py drops its profile-derived fields.  To check a host-side edit: the FUNC symbols of the unit's code
// object sorted by address (tools/kernel_hash.py _code_objects(), or llvm-objdump -d --mcpu=gfx950 on it) must list the
// kernels in the order they had before, and the sha256 of the code object must not move.
template <int L>
using lanes_c = std::integral_constant<int, L>;

// mode -> FIXED_LENGTH: true is visited before false
template <class F>
inline void with_fixed_length(int mode, F &&f)
{
    if (mode == SES_MODE_FIXED_LENGTH) f(std::true_type{});
    else f(std::false_type{});
}

// lanes per env -> LPE: calls f(lanes_c<L>) for the L of Ls... that equals `lanes` (visited in the order listed); false,
// and nothing called, when none does
template <int... Ls, class F>
inline bool with_lanes(int lanes, F &&f)
{
    return (... || (lanes == Ls && (f(lanes_c<Ls>{}), true)));      // a LEFT fold: the compiler expands a right fold last constant first
}

// (num_state, num_action) -> the <S, A> of a policy-forward kernel: as with_lanes, over the pairs listed
template <int S_, int A_>
struct PolicyShape {
    static constexpr int S = S_, A = A_;
};
template <class... Shapes, class F>
inline bool with_policy_shape(int S, int A, F &&f)
{
    return (... || (S == Shapes::S && A == Shapes::A && (f(Shapes{}), true)));
}

// what every fused rollout kernel takes, built once per ses_rollout call
struct RolloutArgs {
    const float *theta, *init;
    int per;             // init_per_offspring
    int n_rows, E, P, max_step;
    uint32_t obs_mask;
    double *epr;
    int32_t *ep_steps;
    const PerturbUpdate *prologue;   // the pair kernel forms its own rows from this first (rollout_with decided that it may); else null
    const float *norm_affine;        // the float64 envs' MLP rollout normalises its observations with this (ses_obs_norm_bind); else null
    double *norm_partials;           // ... and leaves the per-env statistics of the raw observations here (update on); else null
    long long episodes() const { return (long long)n_rows * E; }
};

// launches `kernel` on the handle's stream with the common arguments (a.prologue is not one: only the prologue form of the pair
// kernel takes it, launch_cartpole_mlp_pairs_perturb); the kernel's own (`extra`: waves_light, epw, ...) go
// where the kernels declare them, between obs_mask and the two output arrays
template <class K, class... X>
inline void launch_rollout_kernel(const ses_handle *h, K kernel, dim3 grid, dim3 block, const RolloutArgs &a, X... extra)
{
    hipLaunchKernelGGL(kernel, grid, block, 0, h->stream, a.theta, a.init, a.per, a.n_rows, a.E, a.P, a.max_step, a.obs_mask,
                       extra..., a.epr, a.ep_steps);
}

// A view of the peer-store mailboxes for kernels that exchange 8-byte {sequence, value} GRANULES themselves (the shard form
// of the openai_es tail: the gradient kernel stores its chunk partials straight into every rank's mailbox, the update
// kernel polls them -- the data is the flag, no exchange launch, no fence).  One aligned 8-byte store carries both words.
constexpr int P2P_GRANULE_MAX_WORLD = 16;
struct P2pGranuleView {
    unsigned long long *dst[P2P_GRANULE_MAX_WORLD];   // dst[r]: where THIS rank's granules go in rank r's mailbox (r = own rank included)
    const unsigned long long *src;                    // this rank's mailbox, the slot of this exchange: rank s's granules at src + s * section
    int section;                                      // granules per (slot, source rank) section
    int rank, world;
    uint32_t seq;                                     // the tag of this exchange
    unsigned long long timeout_ticks;
    uint32_t *err, *err_seen;                         // as k_allgather_p2p: host-visible mask, its copy in device memory
};
// reserves the next exchange of `comm`'s peer-store transport for a granule exchange of `granules` per rank; SES_ERR_UNSUPPORTED
// when the transport is not attached or a section cannot hold them, SES_ERR_COMM after an unrecovered time-out
int comm_p2p_granules_begin(ses_handle *comm, int granules, P2pGranuleView *view);

#if defined(__HIPCC__)
__device__ __forceinline__ void granule_store(unsigned long long *dst, uint32_t seq, uint32_t value_bits)
{
    // ONE aligned 8-byte store carries the value and the tag of the exchange it belongs to: whoever reads the tag it waits
    // for has the value (no flag, no fence); system scope: the mailbox may be another GPU's memory
    __hip_atomic_store(dst, ((unsigned long long)value_bits << 32) | (unsigned long long)seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// waits for the granule of exchange v.seq at `src` (a section of THIS rank's mailbox written by rank `from`): its value bits,
// or NaN after the time-out / when the word already carries a LATER exchange's tag (the peer gave up on this rank and moved
// on) -- with rank `from`'s bit set in the error words, as k_allgather_p2p does
__device__ __forceinline__ uint32_t granule_wait(const unsigned long long *src, const P2pGranuleView &v, int from)
{
    const unsigned long long t0 = real_time();
    unsigned long long limit = v.timeout_ticks;
    bool known_late = false;
    for (;;) {
        const unsigned long long g = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        const uint32_t tag = (uint32_t)g;
        if (tag == v.seq) return (uint32_t)(g >> 32);
        if (!known_late) {                                            // (read once, on the slow path only)
            known_late = true;
            const uint32_t seen = __hip_atomic_load(v.err_seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (((seen >> (from & 31)) & 1u) && limit > 200000ull) limit = 200000ull;      // 2 ms for a peer that was late before
        }
        if ((int32_t)(tag - v.seq) > 0 || real_time() - t0 > limit) {
            atomicOr_system(v.err, 1u << (from & 31));
            atomicOr(v.err_seen, 1u << (from & 31));
            return 0x7FC00000u;
        }
        __builtin_amdgcn_s_sleep(2);
    }
}

#endif

int openai_fused_fitness_ok(const ses_handle *h, int32_t n, int32_t per_rank, int32_t n_ranked);     // ses_strategy.hip
int elite_tail_small(ses_handle *h, const double *ep_return, int32_t n, int32_t k, const int32_t *parent_map, int32_t *alias_state,
                     int32_t *rank, float *fitness, float *best, int32_t *ids, int32_t *pidx, int32_t *alias,
                     unsigned long long *stamp, const float *parents, float sigma, uint64_t seed, uint64_t gen, float *mean_out);

// The eight float64 control envs (ses_f64_envs.hip): the env entry functions are the table rows' (ses_env_table.h)
int f64_obs_norm_merge(const ses_handle *h, const double *partials, int n_env, double *stats, float *affine);
// ses_policy_forward for these envs' shapes -- (num_state, num_action) = (6, 3), (2, 3), (3, 1), (2, 1), (5, 1), (9, 1), (9, 2) --
// MLP or GRU
inline bool is_f64_policy_shape(int S, int A)
{
    return (A == 3 && (S == 6 || S == 2)) || (A == 1 && (S == 3 || S == 2 || S == 5 || S == 9)) || (A == 2 && S == 9);
}
int f64_policy_forward(ses_handle *h, const float *theta, const float *obs, float *hidden, int n, float *logits, float *act,
                       int32_t *action);

// simple_spread with the GRU policy (ses_spread_gru.hip): the fused rollout, and ses_policy_forward for (num_state, num_action) =
// (12, 5), (18, 5) with gru = 1
int spread_gru_rollout(const ses_handle *h, const RolloutArgs &a);
inline bool is_spread_policy_shape(int S, int A) { return A == 5 && (S == 12 || S == 18); }
int spread_gru_policy_forward(ses_handle *h, const float *theta, const float *obs, float *hidden, int n, float *logits, float *act,
                              int32_t *action);

// waterworld (ses_waterworld.hip; its env entry functions: ses_env_table.h): ses_policy_forward for (num_state, num_action) = (242, 2)
int waterworld_policy_forward(ses_handle *h, const float *theta, const float *obs, int n, float *logits, float *act, int32_t *action);

// pursuit (ses_pursuit.hip; its env entry functions: ses_env_table.h): ses_policy_forward for (num_state, num_action) = (147, 5)
int pursuit_policy_forward(ses_handle *h, const float *theta, const float *obs, int n, float *logits, float *act, int32_t *action);

// HopperBulletEnv-v0 (ses_hopper.hip; its env entry functions: ses_env_table.h): ses_policy_forward for (num_state, num_action) = (15, 3),
// MLP or GRU
int hopper_policy_forward(ses_handle *h, const float *theta, const float *obs, float *hidden, int n, float *logits, float *act,
                          int32_t *action);

// Walker2DBulletEnv-v0 (ses_walker2d.hip; its env entry functions: ses_env_table.h): ses_policy_forward for (num_state, num_action) =
// (22, 6), MLP or GRU
int walker2d_policy_forward(ses_handle *h, const float *theta, const float *obs, float *hidden, int n, float *logits, float *act,
                            int32_t *action);

// BipedalWalkerHardcore-v3 (ses_walker_hardcore.hip; its env entry functions: ses_env_table.h): ses_policy_forward for a GRU policy of
// (num_state, num_action) = (24, 4); the MLP instance of that shape is ses_rollout.hip's
int walker_hardcore_policy_forward(ses_handle *h, const float *theta, const float *obs, float *hidden, int n, float *logits, float *act,
                                   int32_t *action);

// LunarLander-v2, the discrete four-action lander (ses_lander_discrete.hip): the fused rollout in the form and wave shape that
// the plan chose by the continuous env's rules (ses_rollout_plan.h; form: GRU policies; lpe lanes per env, epw envs per wave:
// MLP policies), and the step-wise env's transition with int32[n] actions (a value outside 0 .. 3 is the no-op)
int lander_discrete_rollout(const ses_handle *h, const RolloutArgs &a, GruForm form, int lpe, int epw);
int lander_discrete_env_step(ses_handle *h, void *state, const int32_t *action, int n, float *obs, float *reward, int32_t *done);

// ---- what ses_run_generations fuses across the entry points of one generation: said in arguments, never kept in the handle -------
// The rollout (ses_rollout.hip).  ses_rollout is rollout_with and empty options.
struct RolloutOpts {
    bool leave_episodes;               // leave the episode returns in the handle's ep_return, launch no episode-mean kernel (the tail
                                       // forms the means: k_rank_count_episodes, elite_tail_small)
    const P2pGranuleView *granules;    // the episode-mean kernel also stores every value as a granule into every rank's mailbox
                                       // (k_fitness_mean_granules): the fitness exchange of a sharded run without a launch of its own
    const PerturbUpdate *apply_first;  // the previous generation's update, which has to be applied before these rows run: in the pair
                                       // kernel's prologue when cartpole_perturb_rollout_ok holds for these rows and mode and theta is
                                       // what it writes, by a k_es_apply_perturb launch first otherwise.  Null again on return once either
                                       // was enqueued; a call refused before that leaves it to the caller.
};
int rollout_with(ses_handle *h, const float *theta, const float *init, int32_t init_per_offspring, int32_t n_rows, int32_t mode,
                 float *fitness, double *ep_return, int32_t *ep_steps, RolloutOpts &o);
bool cartpole_perturb_rollout_ok(const ses_handle *h, int n_rows, int mode);   // the rollout of n_rows can form its own rows

// The openai_es tail (ses_strategy.hip), replicated (comm == null; per_rank, world unused) or in shard form.
// ses_openai_generation[_sharded] are this function and empty options; the argument checks and their texts are in it.
struct OpenaiTailOpts {
    // the granule view of a fitness exchange that the episode-mean kernel fed and the rank kernel consumes (k_rank_sort_search<true>
    // polls the tiles it sorts, k_rank_count_granules the values it counts); own_fitness: this rank's own values, slot_rows: rows
    // per rank slot of the exchange.  No gathered vector exists then (the replicated counting rank writes `fitness`).
    const P2pGranuleView *granules;
    const float *own_fitness;
    int slot_rows;
    // the counting rank forms the episode means itself from episodes[n, eval_ep_num] and writes fitness[] (k_rank_count_episodes);
    // episodes_stamp: where it writes the end-of-rollout time stamp
    const double *episodes;
    unsigned long long *episodes_stamp;
    // where the replicated tail may record its last launch (k_es_apply_perturb) instead of making it, when the rollout of
    // next_mode that runs the whole next population can form its own rows (cartpole_perturb_rollout_ok); null: always launch
    PerturbUpdate *defer_to;
    int next_mode;
};
int openai_generation_impl(ses_handle *h, ses_handle *comm, const float *fitness, int32_t n, uint64_t seed, uint64_t gen, double lr,
                           double sigma, double adam_a, const float *mu_in, const float *m_in, const float *v_in, float *mu_out,
                           float *m_out, float *v_out, float next_sigma, uint64_t next_gen, int64_t first_row, int32_t n_rows,
                           int32_t per_rank, int32_t world, float *theta_next, float *best, const OpenaiTailOpts &o, bool *deferred);
int launch_apply_perturb(ses_handle *h, const PerturbUpdate &u);               // k_es_apply_perturb for this update

int ensure_episode_scratch(ses_handle *h, size_t episodes);
int ensure_obs_norm_scratch(ses_handle *h, size_t doubles);
int ensure_reduce_scratch(ses_handle *h, size_t bytes);
int comm_release(ses_handle *h);
void comm_p2p_set_timeout(ses_handle *h);


}  // namespace ses
