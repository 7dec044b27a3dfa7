// ses_rollout.hip -- the rollout side of the hot path:
//   k_rollout_cartpole_mlp : RolloutWorker (loop.py:108-125) for a whole shard, one kernel
//   k_fitness_mean         : total_reward / eval_ep_num (loop.py:124)
//   k_env_step_cartpole    : standalone SoA env.step (gym_wrapper.py:32-45), the HBM-roofline kernel
//   k_policy_forward_mlp   : standalone population-batched GymEnvModel.forward (neural_network.py:20-36), ses_policy_forward.h
#include "ses_cartpole.h"
#include "ses_gru.h"
#include "ses_gru_lockstep.h"
#include "ses_gru_mfma.h"
#include "ses_gru_mfma4.h"
#include "ses_lander.h"
#include "ses_walker.h"
#include "ses_env_table.h"
#include "ses_policy.h"
#include "ses_policy_pk.h"
#include "ses_policy_forward.h"
#include "ses_rollout_bodies.h"
#include "ses_perturb_prologue.h"
#include "ses_spread.h"

namespace ses {

// ------------------------------------------------------------------------------------------------
// Fused rollout.  Thread layout: LPE adjacent lanes share one env; envs are numbered
// env = row * E + episode, so the E episodes of an offspring sit next to each other and their weight
// loads hit the same cache lines.  Each wave is its own 64-thread workgroup: 20 480 envs x LPE=4 gives
// 1280 independent workgroups that the dispatcher spreads over the 8 XCDs / 256 CUs; nothing is shared
// between workgroups, so no XCD-aware remap is needed.
// All state (4 floats of physics, the lane's slice of the weights, step counter) stays in VGPRs for
// the whole episode; HBM is touched once at the start (theta row, initial state) and once at the end.
// fp32 (default, folded constants) or gym-order float64 dynamics behind one interface
template <bool PHYS64>
struct CartPoleSim;

template <>
struct CartPoleSim<false> {
    CartPoleState st;
    CartPolePre pre;
    float th_clamp, lim_clamp;
    __device__ __forceinline__ void init(const float *s0)
    {
        st = CartPoleState{s0[0], s0[1], s0[2], s0[3]};
        th_clamp = register_constant(CP_TH_CLAMP);
        lim_clamp = register_constant(CP_CLAMP);
    }
    __device__ __forceinline__ void observe(float (&o)[4]) const { o[0] = st.x; o[1] = st.xd; o[2] = st.th; o[3] = st.thd; }
    // |pole angle| <= SINCOS_SMALL_MAX for this lane now -- and then for the whole episode (CP_TH_CLAMP)
    __device__ __forceinline__ bool small_angle() const { return __builtin_fabsf(st.th) <= SINCOS_SMALL_MAX; }
    template <bool SMALL>
    __device__ __forceinline__ void prepare()                               // action-independent half
    {
        pre = SMALL ? cartpole_pre_small(st) : cartpole_pre(st);
    }
    // wave mask of the lanes whose CURRENT state is terminal (== what advance() just returned when nothing was
    // frozen); two ballots of plain compares so that the mask is formed in SGPRs without a detour through a VGPR
    __device__ __forceinline__ unsigned long long terminal_mask() const
    {
        return __builtin_amdgcn_ballot_w64(__builtin_fabsf(st.x) > CP_X_LIMIT) |
               __builtin_amdgcn_ballot_w64(__builtin_fabsf(st.th) > CP_THETA_LIMIT);
    }
    __device__ __forceinline__ bool advance(int action, bool keep_old)
    {
        CartPoleState ns = st;
        const bool term = cartpole_post(ns, pre, action, th_clamp, lim_clamp);
        st.x = keep_old ? st.x : ns.x;
        st.xd = keep_old ? st.xd : ns.xd;
        st.th = keep_old ? st.th : ns.th;
        st.thd = keep_old ? st.thd : ns.thd;
        return term;
    }
};

template <>
struct CartPoleSim<true> {
    CartPoleState64 st;
    __device__ __forceinline__ void init(const float *s0) { st = CartPoleState64{s0[0], s0[1], s0[2], s0[3]}; }
    __device__ __forceinline__ void observe(float (&o)[4]) const
    {
        o[0] = (float)st.x; o[1] = (float)st.xd; o[2] = (float)st.th; o[3] = (float)st.thd;   // neural_network.py:22
    }
    __device__ __forceinline__ bool small_angle() const { return false; }
    template <bool SMALL>
    __device__ __forceinline__ void prepare() {}
    __device__ __forceinline__ unsigned long long terminal_mask() const
    {
        const double thr = 12 * 2 * 3.141592653589793 / 360;
        return __builtin_amdgcn_ballot_w64(__builtin_fabs(st.x) > 2.4) |
               __builtin_amdgcn_ballot_w64(__builtin_fabs(st.th) > thr);
    }
    __device__ __forceinline__ bool advance(int action, bool keep_old)
    {
        CartPoleState64 ns = st;
        const bool term = cartpole_step64(ns, action);
        st.x = keep_old ? st.x : ns.x;
        st.xd = keep_old ? st.xd : ns.xd;
        st.th = keep_old ? st.th : ns.th;
        st.thd = keep_old ? st.thd : ns.thd;
        return term;
    }
};

// The step loop of one wave.  MASKED: some observation components are zeroed (POMDP).  SMALL: every lane's pole
// angle is inside |th| <= SINCOS_SMALL_MAX, so the sin/cos argument reduction is skipped (ses_cartpole.h).
// Fixed length: alive_mask holds the wave's live lanes on entry and on exit, so that a run may stop after some steps and be
// continued by another wave (k_rollout_cartpole_mlp_handover); episodic runs start every env afresh.
template <int LPE, bool FIXED_LENGTH, bool PHYS64, bool MASKED, bool SMALL, class PADS = NoLoopPads>
__device__ __forceinline__ void rollout_cartpole_mlp_loop(const TanhEntry *tanh_tab, const MlpSlice<4, 2, LPE> &net,
                                                          CartPoleSim<PHYS64> &sim, int max_step, uint32_t obs_mask,
                                                          int &steps, unsigned long long &alive_mask)
{
    bool alive = true;
    place_loop<PADS::loop(LPE, false, MASKED, SMALL)>();
    for (int t = 0; t < max_step; ++t) {
        if constexpr (!FIXED_LENGTH) {
            if (__ballot(alive) == 0ull) break;  // wave-uniform: every env of this wave is done
        }
        float obs[4];
        sim.observe(obs);
        if constexpr (MASKED) {
#pragma unroll
            for (int k = 0; k < 4; ++k) obs[k] = ((obs_mask >> k) & 1u) ? 0.0f : obs[k];
        }
        float logits[2];
        typename MlpSlice<4, 2, LPE>::Pending pending;
        net.template begin<true>(tanh_tab, obs, pending);  // fc1 + tanh table reads (by byte offset) in flight ...
        sim.template prepare<SMALL>();                     // ... next to the action-independent half of the physics
        net.finish(pending, logits);
        const int action = argmax_first<2>(logits);
        const bool term = sim.advance(action, FIXED_LENGTH ? false : !alive);  // episodic: a finished env is frozen
        // (the horizon needs no test here: a live env reaches max_step exactly when the loop ends)
        if constexpr (FIXED_LENGTH) {                      // the flag lives in SGPRs as a wave mask
            steps = add_mask_bit(steps, alive_mask);
            alive_mask &= ~sim.terminal_mask();
        } else {                                           // per-lane flag: it also freezes the env
            steps += (int)alive;
            alive = alive & !term;
        }
    }
}

// the loop variant for the wave: fully observed envs skip the masking selects, SMALL the sin/cos argument reduction
template <int LPE, bool FIXED_LENGTH, bool PHYS64, class PADS = NoLoopPads>
__device__ __forceinline__ void rollout_cartpole_mlp_run(const TanhEntry *tanh_tab, const MlpSlice<4, 2, LPE> &net,
                                                         CartPoleSim<PHYS64> &sim, int n_steps, uint32_t obs_mask, bool small,
                                                         int &steps, unsigned long long &alive_mask)
{
    if (obs_mask == 0u && small)
        rollout_cartpole_mlp_loop<LPE, FIXED_LENGTH, PHYS64, false, true, PADS>(tanh_tab, net, sim, n_steps, obs_mask, steps, alive_mask);
    else if (small)
        rollout_cartpole_mlp_loop<LPE, FIXED_LENGTH, PHYS64, true, true, PADS>(tanh_tab, net, sim, n_steps, obs_mask, steps, alive_mask);
    else
        rollout_cartpole_mlp_loop<LPE, FIXED_LENGTH, PHYS64, true, false, PADS>(tanh_tab, net, sim, n_steps, obs_mask, steps, alive_mask);
}

// One wave's share of the rollout: envs [env0 + wave_local_index ...), LPE lanes per env.
// theta holds the population from row row_base on (0: the whole population in global memory; a workgroup that formed its own
// rows in LDS passes those and their first row).
// PK: the packed form of the step for a wave that has its SIMD to itself (ses_policy_pk.h; LPE 8 or 16, fp32 dynamics; the heavy
// wave of the pair kernel takes it at LPE 4 in rollout_cartpole_mlp_pairs).
template <int LPE, bool FIXED_LENGTH, bool PHYS64 = false, bool PK = false, class PADS = NoLoopPads>
__device__ __forceinline__ void rollout_cartpole_mlp_body(const TanhEntry *tanh_tab, long long lane_index, int env0,
                                                          const float *__restrict__ theta,
                                                          const float *__restrict__ init, int init_per_offspring,
                                                          int n_env, int E, int P, int max_step, uint32_t obs_mask,
                                                          double *__restrict__ ep_return,
                                                          int32_t *__restrict__ ep_steps, int row_base = 0)
{
    static_assert(!PK || (!PHYS64 && (LPE == 8 || LPE == 16)), "the packed step exists for 8 / 16 lanes per env, fp32 dynamics");
    int env = env0 + (int)(lane_index / LPE);
    const int sub = (int)(lane_index % LPE);
    const bool valid = env < n_env;
    env = valid ? env : n_env - 1;  // keep every lane active (DPP needs full waves); only valid lanes store
    const int row = env / E;
    const int ep = env - row * E;
    const float *s0 = init + ((size_t)(init_per_offspring ? row : 0) * E + ep) * 4;
    int steps = 0;
    // Loop variants, chosen once per wave (both conditions are wave-uniform):
    //  * fully observed envs (obs_mask == 0, a kernel argument) skip the four masking selects per step;
    //  * when every lane starts inside |th| <= 0.78 -- resets are U(-0.05, 0.05) -- the angle stays there for the
    //    whole episode (CP_TH_CLAMP) and the sin/cos argument reduction is skipped, bit-identically (sincos_small_);
    //    a caller-supplied initial state outside that range runs the general loop.
    const bool small = !PHYS64 && __ballot(!(__builtin_fabsf(s0[2]) <= SINCOS_SMALL_MAX)) == 0ull;
    bool done = false;
    if constexpr (PK) {
        if (small) {
            MlpSlicePk<LPE> netp;
            netp.load(theta + (size_t)(row - row_base) * P, sub);
            CartPoleSimPk simp;
            simp.init(s0);
            unsigned long long alive_mask = ~0ull;
            if (obs_mask == 0u)
                rollout_cartpole_mlp_loop_pk<LPE, FIXED_LENGTH, false>(tanh_tab, netp, simp, max_step, obs_mask, steps, alive_mask);
            else
                rollout_cartpole_mlp_loop_pk<LPE, FIXED_LENGTH, true>(tanh_tab, netp, simp, max_step, obs_mask, steps, alive_mask);
            done = true;
        }
    }
    if (!done) {
        MlpSlice<4, 2, LPE> net;
        net.load(theta + (size_t)(row - row_base) * P, sub);
        CartPoleSim<PHYS64> sim;
        sim.init(s0);
        unsigned long long alive_mask = ~0ull;
        rollout_cartpole_mlp_run<LPE, FIXED_LENGTH, PHYS64, PADS>(tanh_tab, net, sim, max_step, obs_mask, small, steps, alive_mask);
    }
    if (valid && sub == 0) {
        if (ep_return) ep_return[env] = (double)steps;  // CartPole reward is 1 per step incl. the terminal one
        if (ep_steps) ep_steps[env] = steps;
    }
}

template <int LPE, bool FIXED_LENGTH, int BLOCK, bool PHYS64 = false, bool PK = false>
__global__ __launch_bounds__(BLOCK) void k_rollout_cartpole_mlp(const float *__restrict__ theta,
                                                             const float *__restrict__ init, int init_per_offspring,
                                                             int n_rows, int E, int P, int max_step,
                                                             uint32_t obs_mask, double *__restrict__ ep_return,
                                                             int32_t *__restrict__ ep_steps)
{
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    stage_tanh_table(tanh_tab);
    rollout_cartpole_mlp_body<LPE, FIXED_LENGTH, PHYS64, PK>(tanh_tab, (long long)blockIdx.x * BLOCK + threadIdx.x, 0, theta, init,
                                                 init_per_offspring, n_rows * E, E, P, max_step, obs_mask, ep_return,
                                                 ep_steps);
}

// Mixed split for mid-sized populations.  A lone wave issues one VALU instruction per 4 cycles, so a SIMD
// holding a single wave runs at half its issue rate, and with 20 480 envs neither split fills the 1024 SIMDs
// evenly (LPE 4: 1280 waves, a quarter of the SIMDs carry two; LPE 8: 2560 waves, half carry three).
// Here the first `waves8` single-wave workgroups take 8 envs each at 8 lanes per env -- the dispatcher deals
// them one per SIMD -- and the remaining envs follow at 4 lanes per env, so every SIMD ends up with one light
// wave (151 instructions per step) and at most one heavy wave (218).  Results do not depend on the split:
// every LPE variant evaluates the same canonical arithmetic.
// Round 3: the light wave may also run at 16 lanes per env (LIGHT = 16: 4 envs, 83 instructions per step).  At the
// benchmark population -- 20 480 envs -- 1024 such waves + 1024 waves at 4 lanes per env put exactly one light and one
// heavy wave, 20 envs and 243 instructions per step on EVERY SIMD (LIGHT = 8: 264 on three quarters of them, a lone
// light wave on the rest).  launch_cartpole_mlp picks the split whose busiest SIMD has the least to issue.
// Round 6: the second kind of wave is a template argument too.  REST = 4: as above.  (FIRST, REST) = (8, 16): populations between
// one and one and a half waves per SIMD at 8 lanes per env (8192 < envs <= 12 288: the 2048 offspring per GPU of the strong line at
// two GPUs) -- 1024 waves of 8 envs, one per SIMD, then the remaining envs four to a wave: a doubled SIMD issues 104 + 83 instructions
// per step where the pure split gave a quarter of the SIMDs 2 x 104.
template <bool FIXED_LENGTH, int LIGHT, int REST = 4>
__global__ __launch_bounds__(64) void k_rollout_cartpole_mlp_mix(const float *__restrict__ theta,
                                                                 const float *__restrict__ init,
                                                                 int init_per_offspring, int n_rows, int E, int P,
                                                                 int max_step, uint32_t obs_mask, int waves_light,
                                                                 double *__restrict__ ep_return,
                                                                 int32_t *__restrict__ ep_steps)
{
    constexpr int EPW = 64 / LIGHT;                    // envs of a wave of the first kind
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    stage_tanh_table(tanh_tab);
    const int n_env = n_rows * E;
    if ((int)blockIdx.x < waves_light) {
        rollout_cartpole_mlp_body<LIGHT, FIXED_LENGTH>(tanh_tab, (long long)blockIdx.x * 64 + threadIdx.x, 0, theta, init,
                                                       init_per_offspring, n_env < waves_light * EPW ? n_env : waves_light * EPW,
                                                       E, P, max_step, obs_mask, ep_return, ep_steps);
    } else {
        rollout_cartpole_mlp_body<REST, FIXED_LENGTH>(tanh_tab, (long long)(blockIdx.x - waves_light) * 64 + threadIdx.x,
                                                      waves_light * EPW, theta, init, init_per_offspring, n_env, E, P, max_step,
                                                      obs_mask, ep_return, ep_steps);
    }
}

// Round 7: the (16, 4) mix as light + heavy wave pairs (fixed-length mode).  Inferred from the round-6 SQ counters, not
// stamped: on a SIMD holding one light and one heavy wave of the mix the light wave (dispatched first, so older) wins VALU
// arbitration, ends its 500 x 83 instructions early, and the heavy wave (500 x 160) runs the rest alone at the lone-wave
// cadence.  One 512-thread workgroup per CU: waves 0-3 are the light waves, waves 4-7 the heavy ones, and wave w and wave
// w + 4 form pair 4 * block + w % 4.  They are meant to share SIMD w % 4 -- what the dispatcher was seen to do with the
// waves of a 512-thread workgroup (NOTES, "MFMA and VALU do not overlap": HW_ID) -- but nothing depends on it except speed.
// The pair's envs are numbered as in k_rollout_cartpole_mlp_mix: the light wave takes envs [4p, 4p + 4), the heavy wave
// [4 L + 16p, 4 L + 16p + 16) with L light waves.
//  * prio_steps (default: all): the heavy wave runs its first prio_steps steps at s_setprio 1, so that it is served before
//    the light wave, which fills its dependency stalls.  This is what pays: 196 -> 180 us at 4096 x 5 x 500, no
//    instruction added.  The same s_setprio in the heavy single-wave workgroups of k_rollout_cartpole_mlp_mix gets 4/5 of
//    that: 0.2008 against 0.1977 ms per generation, ranges apart (profiles/r07_handover_sweep.txt).
//  * handover < max_step (default: off): the heavy wave stops at that step, the state of its 16 envs crosses through LDS as
//    raw bits (x, xd, th, thd, steps, alive) and both waves run 8 of them at 8 lanes per env (104 instructions per step) to
//    max_step.  Measured slower than the priority alone: 16 envs cost 2 x 104 instructions per step against 160.  The
//    phase-2 loop takes the sin/cos shortcut only if the heavy wave did, i.e. if it held for all 16 envs.
//  * HEAVY_PK (round 9; knob "rollout_heavy_packed", default on): the heavy wave runs the packed form of the step
//    (ses_policy_pk.h, MlpSlicePk<4>): 132 VALU instructions per step for 160, 153 instructions of every kind for 175.  Served
//    first, the heavy wave pays for its instructions one by one (16 extra moves per step cost it 12.8 us, the light wave 4.1).
//    Measured: 0.1924 -> 0.1894 ms per generation (profiles/r09_heavy_stream.txt); the rest of the heavy wave's step is its own
//    dependence stalls.  A wave with an env outside the small-angle range keeps the scalar loop.  Round 10: 148 instructions of every
//    kind -- the loop waits for its table reads three times, not seven, and no longer for the fc2 bias (ses_policy_pk.h): 0.1889 ->
//    0.1791 ms per generation (profiles/r10_action_speculated.txt).
// Every lanes-per-env form evaluates the same canonical arithmetic, so the results are the bits of the unsplit schedule.
// The pairs of one workgroup are a device function of the workgroup's LDS and of where its rows are: OWN_ROWS false -- theta is
// the population in global memory; true -- the workgroup formed the rows of its light envs (rows_l, from row row0_l) and of its
// heavy envs (rows_h, from row0_h) in LDS itself (perturb_prologue), theta is not read.
// no-op counts of the prologue form's step loops (place_loop, ses_policy.h), per instance
template <bool HEAVY_PK>
struct PrologueLoopPads {
    static constexpr int seg = HEAVY_PK ? 4 : 3;
    static constexpr int loop(int lpe, bool pk, bool masked, bool small)
    {
        if (lpe == 16) return !small ? 2 : masked ? 5 : 4;                      // the light wave
        if (lpe == 8) return HEAVY_PK ? 3 : 7;                                  // behind the hand-over
        if (pk) return masked ? 0 : 5;                                          // the heavy wave, packed
        return HEAVY_PK ? 7 : -1;       // ... scalar: <true, false> runs these inside its segment loop, which is placed as a whole
    }
};
struct HandoverSlot {
    float x, xd, th, thd;
    int steps, alive;
};
template <bool FIXED_LENGTH, bool OWN_ROWS, bool HEAVY_PK>
__device__ __forceinline__ void rollout_cartpole_mlp_pairs(
    const TanhEntry *tanh_tab, HandoverSlot (*slots)[64 / 4], int *small_of, const float *__restrict__ theta,
    const float *__restrict__ init, int init_per_offspring, int n_rows, int E, int P, int max_step, uint32_t obs_mask,
    int waves_light, int waves_heavy, int handover, int prio_steps, double *__restrict__ ep_return,
    int32_t *__restrict__ ep_steps, const float *rows_l = nullptr, int row0_l = 0, const float *rows_h = nullptr, int row0_h = 0)
{
    static_assert(FIXED_LENGTH, "the hand-over needs every env to run max_step steps");
    constexpr int LIGHT = 16, HEAVY = 4, SPLIT = 8;
    using PADS = std::conditional_t<OWN_ROWS, PrologueLoopPads<HEAVY_PK>, NoLoopPads>;   // only the prologue form was measured placed
    constexpr int EPW_L = 64 / LIGHT, EPW_H = 64 / HEAVY, EPW_S = 64 / SPLIT;
    static_assert(EPW_H == 2 * EPW_S, "the heavy wave's envs are split evenly");
    using Slot = HandoverSlot;
    const int wave = (int)threadIdx.x / 64, lane = (int)threadIdx.x % 64;
    const int slot = wave % HANDOVER_PAIRS;
    const int pair = (int)blockIdx.x * HANDOVER_PAIRS + slot;
    const bool heavy = wave >= HANDOVER_PAIRS;
    const int n_env = n_rows * E;
    const int n_light = n_env < waves_light * EPW_L ? n_env : waves_light * EPW_L;
    const int env0_h = waves_light * EPW_L + pair * EPW_H;           // the heavy wave's first env
    const bool has_heavy = pair < waves_heavy && env0_h < n_env;    // wave-uniform, and the same in both waves of a pair
    const bool split = handover < max_step;                          // kernel arguments: workgroup-uniform
    const int n_heavy = split ? handover : max_step;                 // steps the heavy wave runs on its 16 envs
    if (!heavy) {                                                    // phase 1 of the light wave: its own envs, to the end
        if (pair * EPW_L < n_light)
            rollout_cartpole_mlp_body<LIGHT, FIXED_LENGTH, false, false, PADS>(tanh_tab, (long long)pair * 64 + lane, 0, OWN_ROWS ? rows_l : theta, init,
                                                           init_per_offspring, n_light, E, P, max_step, obs_mask, ep_return,
                                                           ep_steps, OWN_ROWS ? row0_l : 0);
    } else if (has_heavy) {                                          // phase 1 of the heavy wave: steps [0, handover)
        int env = env0_h + lane / HEAVY;
        const int sub = lane % HEAVY;
        const bool valid = env < n_env;
        env = valid ? env : n_env - 1;                               // as in rollout_cartpole_mlp_body
        const int row = env / E;
        const int ep = env - row * E;
        const float *s0 = init + ((size_t)(init_per_offspring ? row : 0) * E + ep) * 4;
        const bool small = __ballot(!(__builtin_fabsf(s0[2]) <= SINCOS_SMALL_MAX)) == 0ull;
        const float *const row_theta = OWN_ROWS ? rows_h + (size_t)(row - row0_h) * P : theta + (size_t)row * P;
        CartPoleSim<false> sim;
        sim.init(s0);
        int steps = 0;
        unsigned long long alive_mask = ~0ull;
        // the first prio_steps steps at s_setprio 1: VALU arbitration goes by priority before age, so the (younger) heavy
        // wave is served first
        const int n1 = prio_steps < n_heavy ? prio_steps : n_heavy;
        bool done = false;
        if constexpr (HEAVY_PK) if (small) {
            // the packed form of the step (ses_policy_pk.h): the wave served first issues at its own cadence, one interval per
            // instruction whatever it is, so fewer instructions are less time
            MlpSlicePk<HEAVY> netp;
            netp.load(row_theta, sub);
            CartPoleSimPk simp;
            simp.init(s0);
            place_loop<PADS::seg>();
#pragma unroll 1
            for (int seg = 0; seg < 2; ++seg) {
                if (seg == 0) __builtin_amdgcn_s_setprio(1);
                else __builtin_amdgcn_s_setprio(0);
                const int n_seg = seg == 0 ? n1 : n_heavy - n1;
                if (obs_mask == 0u)
                    rollout_cartpole_mlp_loop_pk<HEAVY, FIXED_LENGTH, false, PADS>(tanh_tab, netp, simp, n_seg, obs_mask, steps, alive_mask);
                else
                    rollout_cartpole_mlp_loop_pk<HEAVY, FIXED_LENGTH, true, PADS>(tanh_tab, netp, simp, n_seg, obs_mask, steps, alive_mask);
            }
            sim.st = CartPoleState{simp.P.x, simp.V.x, simp.P.y, simp.V.y};
            done = true;
        }
        if (!done) {
            MlpSlice<4, 2, HEAVY> net;
            net.load(row_theta, sub);
            place_loop<PADS::seg>();
#pragma unroll 1
            for (int seg = 0; seg < 2; ++seg) {
                if (seg == 0) __builtin_amdgcn_s_setprio(1);
                else __builtin_amdgcn_s_setprio(0);
                rollout_cartpole_mlp_run<HEAVY, FIXED_LENGTH, false, PADS>(tanh_tab, net, sim, seg == 0 ? n1 : n_heavy - n1, obs_mask,
                                                                     small, steps, alive_mask);
            }
        }
        if (!split) {
            if (valid && sub == 0) {
                if (ep_return) ep_return[env] = (double)steps;
                if (ep_steps) ep_steps[env] = steps;
            }
        } else if (sub == 0) {
            slots[slot][lane / HEAVY] = Slot{sim.st.x, sim.st.xd, sim.st.th, sim.st.thd, steps, (int)((alive_mask >> lane) & 1ull)};
            if (lane == 0) small_of[slot] = small ? 1 : 0;
        }
    }
    if (!split) return;                                              // workgroup-uniform
    __syncthreads();                                                 // every wave of the workgroup gets here
    if (!has_heavy) return;
    // phase 2, steps [handover, max_step): the heavy wave keeps the first half of its envs, the light wave takes the rest
    const int k = (heavy ? 0 : EPW_S) + lane / SPLIT;
    const int sub = lane % SPLIT;
    int env = env0_h + k;
    const bool valid = env < n_env;
    env = valid ? env : n_env - 1;
    const int row = env / E;
    const Slot st = slots[slot][k];
    const bool small = small_of[slot] != 0;
    MlpSlice<4, 2, SPLIT> net;
    net.load(OWN_ROWS ? rows_h + (size_t)(row - row0_h) * P : theta + (size_t)row * P, sub);
    const float s1[4] = {st.x, st.xd, st.th, st.thd};
    CartPoleSim<false> sim;
    sim.init(s1);
    int steps = st.steps;
    unsigned long long alive_mask = __ballot(st.alive != 0);
    rollout_cartpole_mlp_run<SPLIT, FIXED_LENGTH, false, PADS>(tanh_tab, net, sim, max_step - handover, obs_mask, small, steps,
                                                         alive_mask);
    if (valid && sub == 0) {
        if (ep_return) ep_return[env] = (double)steps;
        if (ep_steps) ep_steps[env] = steps;
    }
}

template <bool FIXED_LENGTH, bool HEAVY_PK = false>
__global__ __launch_bounds__(64 * 2 * HANDOVER_PAIRS) void k_rollout_cartpole_mlp_handover(
    const float *__restrict__ theta, const float *__restrict__ init, int init_per_offspring, int n_rows, int E, int P,
    int max_step, uint32_t obs_mask, int waves_light, int waves_heavy, int handover, int prio_steps,
    double *__restrict__ ep_return, int32_t *__restrict__ ep_steps)
{
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ HandoverSlot slots[HANDOVER_PAIRS][64 / 4];
    __shared__ int small_of[HANDOVER_PAIRS];
    stage_tanh_table(tanh_tab);
    rollout_cartpole_mlp_pairs<FIXED_LENGTH, false, HEAVY_PK>(tanh_tab, slots, small_of, theta, init, init_per_offspring, n_rows, E, P,
                                                              max_step, obs_mask, waves_light, waves_heavy, handover, prio_steps,
                                                              ep_return, ep_steps);
}

// The pair kernel behind an openai_es generation of the same ses_run_generations call: the population it runs does not exist yet.
// Every workgroup applies the previous generation's update to the mean and draws the rows of ITS envs -- light envs [16 b, 16 b + 16),
// heavy envs [4 L + 64 b, 4 L + 64 b + 64) of workgroup b, clipped to the envs there are; a lane past the last env runs the last
// env, whose row is among them -- into LDS and into u.theta (perturb_prologue: what k_es_apply_perturb would have launched for,
// bit for bit).  Dynamic LDS: the mean (u.P4 floats) and pair_own_rows(E) rows of u.P floats.
template <bool FIXED_LENGTH, bool HEAVY_PK = false>
__global__ __launch_bounds__(64 * 2 * HANDOVER_PAIRS) void k_rollout_cartpole_mlp_handover_perturb(
    const float *__restrict__ init, int init_per_offspring, int n_rows, int E, int P, int max_step, uint32_t obs_mask,
    int waves_light, int waves_heavy, int handover, int prio_steps, double *__restrict__ ep_return,
    int32_t *__restrict__ ep_steps, PerturbUpdate u)
{
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ HandoverSlot slots[HANDOVER_PAIRS][64 / 4];
    __shared__ int small_of[HANDOVER_PAIRS];
    extern __shared__ __attribute__((aligned(16))) float own_rows_lds[];     // (the mean is read 16 bytes at a time)
    constexpr int ENVS_L = HANDOVER_PAIRS * (64 / 16), ENVS_H = HANDOVER_PAIRS * (64 / 4);      // envs of a workgroup's waves
    const int n_env = n_rows * E;
    const int n_light = n_env < waves_light * (64 / 16) ? n_env : waves_light * (64 / 16);
    const int l0 = (int)blockIdx.x * ENVS_L, h0 = waves_light * (64 / 16) + (int)blockIdx.x * ENVS_H;
    const RowSpan span_l = rows_of_envs(l0, l0 + ENVS_L < n_light ? l0 + ENVS_L : n_light, E);
    const RowSpan span_h = rows_of_envs(h0, h0 + ENVS_H < n_env ? h0 + ENVS_H : n_env, E);
    float *const mu_new = own_rows_lds, *const rows = own_rows_lds + u.P4;
    // (stages the tanh table too; the constant: where this instance's step loops were measured, perturb_prologue's last comment)
    perturb_prologue<HEAVY_PK ? 33 : 41>(u, span_l, span_h, mu_new, rows, tanh_tab);
    rollout_cartpole_mlp_pairs<FIXED_LENGTH, true, HEAVY_PK>(tanh_tab, slots, small_of, nullptr, init, init_per_offspring, n_rows, E, P,
                                                             max_step, obs_mask, waves_light, waves_heavy, handover, prio_steps, ep_return,
                                                             ep_steps, rows, span_l.row0, rows + (size_t)span_l.rows * P, span_h.row0);
}

// GRU policy: one offspring per wavefront (ses_gru.h), its E episodes run one after the other so the
// 6 x 16 + ... weights per lane stay in VGPRs across all of them.  4 offspring per 256-thread workgroup
// share one copy of the tanh table; the waves never synchronise with each other (episode lengths differ).
template <bool FIXED_LENGTH>
__global__ __launch_bounds__(256) void k_rollout_cartpole_gru(const float *__restrict__ theta,
                                                              const float *__restrict__ init, int init_per_offspring,
                                                              int n_rows, int E, int P, int max_step,
                                                              uint32_t obs_mask, double *__restrict__ ep_return,
                                                              int32_t *__restrict__ ep_steps, int ep_parallel)
{
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ __attribute__((aligned(16))) float vecs[4][64];
    stage_tanh_table(tanh_tab);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // ep_parallel: one wave per (offspring, episode) instead of one per offspring -- for populations too small to
    // fill the chip the E episodes of an offspring run side by side and the rollout takes one episode's time
    const int unit = blockIdx.x * 4 + wave, n_units = ep_parallel ? n_rows * E : n_rows;
    const bool valid = unit < n_units;
    const int u = valid ? unit : n_units - 1;
    const int row = ep_parallel ? u / E : u;
    const int ep_begin = ep_parallel ? u - row * E : 0, ep_end = ep_parallel ? ep_begin + 1 : E;
    GruSlice<4, 2> net;
    net.load(theta + (size_t)row * P, lane);
    float *vec = vecs[wave];
    for (int ep = ep_begin; ep < ep_end; ++ep) {
        const float *s0 = init + ((size_t)(init_per_offspring ? row : 0) * E + ep) * 4;
        CartPoleState st{s0[0], s0[1], s0[2], s0[3]};
        float h = 0.0f;                                   // GymEnvModel.reset(), neural_network.py:38-40
        wave_lds_sync();
        if (lane < 32) vec[2 * lane + 1] = 0.0f;
        wave_lds_sync();
        int steps = 0;
        bool alive = true;
        for (int t = 0; t < max_step; ++t) {
            if constexpr (!FIXED_LENGTH) {
                if (__builtin_amdgcn_readfirstlane((int)alive) == 0) break;   // one env per wave: uniform
            }
            float obs[4];
            obs[0] = (obs_mask & 1u) ? 0.0f : st.x;
            obs[1] = (obs_mask & 2u) ? 0.0f : st.xd;
            obs[2] = (obs_mask & 4u) ? 0.0f : st.th;
            obs[3] = (obs_mask & 8u) ? 0.0f : st.thd;
            float logits[2];
            net.forward(tanh_tab, obs, h, vec, lane, logits);
            const int action = argmax_first<2>(logits);
            CartPoleState ns = st;
            const bool term = cartpole_step_general(ns, action);
            const bool advance = FIXED_LENGTH ? true : alive;
            st.x = advance ? ns.x : st.x;
            st.xd = advance ? ns.xd : st.xd;
            st.th = advance ? ns.th : st.th;
            st.thd = advance ? ns.thd : st.thd;
            const int nsteps = steps + 1;
            const bool finished = term | (nsteps >= max_step);
            steps = alive ? nsteps : steps;
            alive = alive & !finished;
        }
        if (valid && lane == 0) {
            if (ep_return) ep_return[(size_t)row * E + ep] = (double)steps;
            if (ep_steps) ep_steps[(size_t)row * E + ep] = steps;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Lockstep GRU rollout (ses_gru_lockstep.h): one offspring per wave, up to 8 episodes advance together,
// lane l owns the env of episode (l & 7).  EnvT adapts an env to the kernel.
struct CartPoleLs {
    static constexpr int S = 4, A = 2, INIT_W = 4;
    struct State {
        CartPoleState st;
    };
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u, int)
    {
        s.st = CartPoleState{u[0], u[1], u[2], u[3]};
    }
    __device__ static __forceinline__ void observe(const State &s, float (&obs)[S])
    {
        obs[0] = s.st.x; obs[1] = s.st.xd; obs[2] = s.st.th; obs[3] = s.st.thd;
    }
    // advance with the policy output; returns the reward, sets done.  `freeze`: keep the old state (finished env)
    __device__ static __forceinline__ float step(State &s, const float (&logits)[A], const TanhEntry *, bool freeze,
                                                 bool &done)
    {
        const int action = argmax_first<A>(logits);
        CartPoleState ns = s.st;
        done = cartpole_step_general(ns, action);
        s.st.x = freeze ? s.st.x : ns.x;
        s.st.xd = freeze ? s.st.xd : ns.xd;
        s.st.th = freeze ? s.st.th : ns.th;
        s.st.thd = freeze ? s.st.thd : ns.thd;
        return 1.0f;
    }
};

struct CartPoleLs64 {
    static constexpr int S = 4, A = 2, INIT_W = 4;
    struct State {
        CartPoleState64 st;
    };
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u, int)
    {
        s.st = CartPoleState64{u[0], u[1], u[2], u[3]};
    }
    __device__ static __forceinline__ void observe(const State &s, float (&obs)[S])
    {
        obs[0] = (float)s.st.x; obs[1] = (float)s.st.xd; obs[2] = (float)s.st.th; obs[3] = (float)s.st.thd;
    }
    __device__ static __forceinline__ float step(State &s, const float (&logits)[A], const TanhEntry *, bool freeze,
                                                 bool &done)
    {
        const int action = argmax_first<A>(logits);
        CartPoleState64 ns = s.st;
        done = cartpole_step64(ns, action);
        s.st.x = freeze ? s.st.x : ns.x;
        s.st.xd = freeze ? s.st.xd : ns.xd;
        s.st.th = freeze ? s.st.th : ns.th;
        s.st.thd = freeze ? s.st.thd : ns.thd;
        return 1.0f;
    }
};

struct LanderLs {
    static constexpr int S = 8, A = 4, INIT_W = 16;
    struct State {
        LanderState st;
    };
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u, int slot)
    {
        __shared__ float terrain[4][32][LL_TERRAIN_ROW];       // one terrain row per (wave, env slot); slot < 32
        ll_reset(s.st, u, terrain[threadIdx.x >> 6][slot]);
    }
    __device__ static __forceinline__ void observe(const State &s, float (&obs)[S]) { ll_obs(s.st, obs); }
    __device__ static __forceinline__ float step(State &s, const float (&logits)[A], const TanhEntry *tab, bool freeze,
                                                 bool &done)
    {
        const float a0 = tanh_(tab, logits[0]), a1 = tanh_(tab, logits[1]);
        float r = 0.0f;
        done = true;
        if (!freeze) r = ll_step(s.st, a0, a1, done);          // a finished env is frozen (the env code has no wave votes)
        return r;
    }
};

// ------------------------------------------------------------------------------------------------
// The lockstep GRU rollout with the policy step on v_mfma_f32_4x4x1_16b_f32 (ses_gru_mfma4.h, round 6): one offspring per
// wave, up to 8 episodes, lane l owns the env of episode (l & 7) exactly as in gru_lockstep_batch; only the policy differs.
template <typename EnvT, bool FIXED_LENGTH>
__device__ __forceinline__ void gru_mfma4_batch(const TanhEntry *tanh_tab, GruMfma4Lds<EnvT::S, EnvT::A> &lds,
                                                const GruMfma4<EnvT::S, EnvT::A> &net, int lane, int nb,
                                                const float *__restrict__ init_rows, int max_step, uint32_t obs_mask,
                                                double *__restrict__ ret_out, int32_t *__restrict__ steps_out, bool valid_row)
{
    constexpr int S = EnvT::S, A = EnvT::A;
    const int slot = lane & 7;
    const bool owner_valid = slot < nb;
    typename EnvT::State st;
    EnvT::reset(st, init_rows + (size_t)(owner_valid ? slot : 0) * EnvT::INIT_W, slot);   // padding slots replay episode 0
    float hreg[4] = {0.0f, 0.0f, 0.0f, 0.0f};                                     // GymEnvModel.reset()
    wave_lds_sync();
    if (lane < 32) {
#pragma unroll
        for (int e = 0; e < G4_EB; ++e) lds.ah[e][lane][1] = 0.0f;
    }
    double ret = 0.0;
    int steps = 0;
    bool alive = true;
    for (int t = 0; t < max_step; ++t) {
        if constexpr (!FIXED_LENGTH) {
            if (__ballot(alive & owner_valid) == 0ull) break;
        }
        float obs[S];
        EnvT::observe(st, obs);
        if (lane < G4_EB) {
#pragma unroll
            for (int k = 0; k < S; ++k) lds.obs[lane][k] = ((obs_mask >> k) & 1u) ? 0.0f : obs[k];
        }
        wave_lds_sync();
        net.step(tanh_tab, lds, hreg, lane);
        float logits[A];
        GruMfma4<S, A>::logits_of(lds, lane, logits);
        bool term;
        const bool freeze = FIXED_LENGTH ? false : !alive;
        const float r = EnvT::step(st, logits, tanh_tab, freeze, term);
        const int nsteps = steps + 1;
        const bool finished = term | (nsteps >= max_step);
        ret = alive ? ret + (double)r : ret;
        steps = alive ? nsteps : steps;
        alive = alive & !finished;
    }
    if (valid_row && lane < G4_EB && owner_valid) {
        if (ret_out) ret_out[slot] = ret;
        if (steps_out) steps_out[slot] = steps;
    }
}

// 4 offspring per 256-thread workgroup (one copy of the tanh table), two waves per SIMD: W_hh (96 values per lane) in registers,
// W_ih in the wave's LDS block (13.5 KB; two workgroups = 8 waves fill 158 of the CU's 160 KB).  With all 192 gate weights in
// registers the kernel needed 360 of them, i.e. one wave per SIMD, and a lone wave ran the step's ~550 non-MFMA instructions
// with every stall exposed: 4.01 ms against this form's -- see DESIGN.md section 4.
template <typename EnvT, bool FIXED_LENGTH>
__global__ __launch_bounds__(256, 2) void k_rollout_gru_mfma4(const float *__restrict__ theta, const float *__restrict__ init,
                                                              int init_per_offspring, int n_rows, int E, int P, int max_step,
                                                              uint32_t obs_mask, double *__restrict__ ep_return,
                                                              int32_t *__restrict__ ep_steps)
{
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ __attribute__((aligned(16))) GruMfma4Lds<EnvT::S, EnvT::A> ldsv[4];
    stage_tanh_table(tanh_tab);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int row = blockIdx.x * 4 + wave;
    const bool valid = row < n_rows;
    row = valid ? row : n_rows - 1;
    GruMfma4Lds<EnvT::S, EnvT::A> &lds = ldsv[wave];
    GruMfma4<EnvT::S, EnvT::A> net;
    net.load(theta + (size_t)row * P, lane, lds);
    wave_lds_sync();
    for (int e0 = 0; e0 < E; e0 += G4_EB) {
        const int nb = E - e0 < G4_EB ? E - e0 : G4_EB;
        const float *rows = init + ((size_t)(init_per_offspring ? row : 0) * E + e0) * EnvT::INIT_W;
        double *ro = ep_return ? ep_return + (size_t)row * E + e0 : nullptr;
        int32_t *so = ep_steps ? ep_steps + (size_t)row * E + e0 : nullptr;
        gru_mfma4_batch<EnvT, FIXED_LENGTH>(tanh_tab, lds, net, lane, nb, rows, max_step, obs_mask, ro, so, valid);
    }
}

// ------------------------------------------------------------------------------------------------
// Lockstep GRU rollout with G offspring per wave (gru_lockstep_multi_batch, ses_rollout_bodies.h): four waves per workgroup,
// each with its own G blocks of LDS.
template <typename EnvT, int G>
__global__ __launch_bounds__(256, 2) void k_rollout_gru_lockstep_multi(const float *__restrict__ theta,
                                                                    const float *__restrict__ init, int init_per_offspring,
                                                                    int n_rows, int E, int P, int max_step,
                                                                    uint32_t obs_mask, double *__restrict__ ep_return,
                                                                    int32_t *__restrict__ ep_steps)
{
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ __attribute__((aligned(16))) GruLockstepLds<EnvT::S, EnvT::A> ldsv[4][G];
    stage_tanh_table(tanh_tab);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row0 = (blockIdx.x * 4 + wave) * G;
    if (row0 >= n_rows) return;                       // (no workgroup-level synchronisation after the table staging)
#define SES_LSM_CASE(NP_, ODD_)                                                                                          \
    gru_lockstep_multi_batch<EnvT, G, NP_, ODD_>(tanh_tab, ldsv[wave], theta, P, row0, n_rows, lane, E, init,              \
                                                 init_per_offspring, E, max_step, obs_mask, ep_return, ep_steps)
    switch (E) {                                      // E <= GL_EB (the launcher checks)
        case 1: SES_LSM_CASE(1, true); break;
        case 2: SES_LSM_CASE(1, false); break;
        case 3: SES_LSM_CASE(2, true); break;
        case 4: SES_LSM_CASE(2, false); break;
        case 5: SES_LSM_CASE(3, true); break;
        case 6: SES_LSM_CASE(3, false); break;
        case 7: SES_LSM_CASE(4, true); break;
        default: SES_LSM_CASE(4, false); break;
    }
#undef SES_LSM_CASE
}

// ------------------------------------------------------------------------------------------------
// MFMA GRU rollout (gru_mfma_batch, ses_rollout_bodies.h): 4 offspring per 256-thread workgroup.
template <typename EnvT, bool FIXED_LENGTH>
__global__ __launch_bounds__(256, 2) void k_rollout_gru_mfma(const float *__restrict__ theta,
                                                          const float *__restrict__ init, int init_per_offspring,
                                                          int n_rows, int E, int P, int max_step, uint32_t obs_mask,
                                                          double *__restrict__ ep_return,
                                                          int32_t *__restrict__ ep_steps)
{
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ __attribute__((aligned(16))) GruMfmaLds<EnvT::S, EnvT::A> ldsv[4];
    stage_tanh_table(tanh_tab);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int row = blockIdx.x * 4 + wave;
    const bool valid = row < n_rows;
    row = valid ? row : n_rows - 1;
    GruMfmaLds<EnvT::S, EnvT::A> &lds = ldsv[wave];
    GruMfma<EnvT::S, EnvT::A> net;
    net.load(theta + (size_t)row * P, lane, lds);
    wave_lds_sync();
    for (int e0 = 0; e0 < E; e0 += GM_EB) {
        const int nb = E - e0 < GM_EB ? E - e0 : GM_EB;
        const float *rows = init + ((size_t)(init_per_offspring ? row : 0) * E + e0) * EnvT::INIT_W;
        double *ro = ep_return ? ep_return + (size_t)row * E + e0 : nullptr;
        int32_t *so = ep_steps ? ep_steps + (size_t)row * E + e0 : nullptr;
        gru_mfma_batch<EnvT, FIXED_LENGTH>(tanh_tab, lds, net, lane, nb, rows, max_step, obs_mask, ro, so, valid);
    }
}

// LunarLanderContinuous-v2 (ses_lander.h): continuous control (tanh head, the env uses outputs 0 and 1 -- SURVEY 3.4-12), float
// rewards accumulated in float64 like the reference's python sum (loop.py:123).  GRU policy, one offspring (or one
// episode of it, ep_parallel) per wave, episodes one after the other; the MLP policies run in k_rollout_box2d_mlp.
__global__ __launch_bounds__(256, 2) void k_rollout_lander_gru(const float *__restrict__ theta,
                                                        const float *__restrict__ init, int init_per_offspring,
                                                        int n_rows, int E, int P, int max_step, uint32_t obs_mask,
                                                        double *__restrict__ ep_return, int32_t *__restrict__ ep_steps,
                                                        int ep_parallel)
{
    constexpr int S = 8, A = 4;
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ __attribute__((aligned(16))) float vecs[4][64];
    __shared__ float terrain[4][LL_TERRAIN_ROW];                  // one terrain row per wave
    stage_tanh_table(tanh_tab);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    {
        const int unit = blockIdx.x * 4 + wave, n_units = ep_parallel ? n_rows * E : n_rows;   // see k_rollout_cartpole_gru
        const bool valid = unit < n_units;
        const int u = valid ? unit : n_units - 1;
        const int row = ep_parallel ? u / E : u;
        const int ep_begin = ep_parallel ? u - row * E : 0, ep_end = ep_parallel ? ep_begin + 1 : E;
        GruSlice<S, A> net;
        net.load(theta + (size_t)row * P, lane);
        float *vec = vecs[wave];
        for (int ep = ep_begin; ep < ep_end; ++ep) {
            LanderState st;
            ll_reset(st, init + ((size_t)(init_per_offspring ? row : 0) * E + ep) * 16, terrain[wave]);
            float h = 0.0f;
            wave_lds_sync();
            if (lane < 32) vec[2 * lane + 1] = 0.0f;
            wave_lds_sync();
            double ret = 0.0;
            int steps = 0;
            bool done = false;
            while (steps < max_step) {
                if (__builtin_amdgcn_readfirstlane((int)done)) break;
                float obs[S], logits[A];
                ll_obs(st, obs);
#pragma unroll
                for (int k = 0; k < S; ++k) obs[k] = ((obs_mask >> k) & 1u) ? 0.0f : obs[k];
                net.forward(tanh_tab, obs, h, vec, lane, logits);
                const float a0 = tanh_(tanh_tab, logits[0]), a1 = tanh_(tanh_tab, logits[1]);
                ret += (double)ll_step(st, a0, a1, done);
                steps += 1;
            }
            if (valid && lane == 0) {
                ep_return[(size_t)row * E + ep] = ret;
                if (ep_steps) ep_steps[(size_t)row * E + ep] = steps;
            }
        }
    }
}

// MLP policies on the Box2D-style envs (LunarLander: conf/lunarlander.yaml, BipedalWalker: conf/bipedalwalker.yaml):
// LPE lanes per env (LPE <= 8: 32 / LPE hidden units each for the forward; above: the forward on every 16-lane row), every
// lane of a group carries the env.  A wave-step costs a + b x (different envs in the wave) with a large a -- the solver's
// sequential iterations, whatever the number of lanes that carry an env -- so box2d_wave_shape() spreads the population
// over every wave slot of the chip with as few envs per wave as that allows (envs_per_wave), LPE follows from it, and
// the lane groups past the last env shadow it (same env, same path).
// Single-wave workgroups (they spread over all SIMDs and retire independently).  EnvB adapts an env.
struct LanderMlpEnv {
    static constexpr int S = 8, A = 4, INIT_W = 16, ROW = LL_TERRAIN_ROW;
    static constexpr int WAVES_PER_SIMD = LANDER_MLP_WAVES_PER_SIMD;   // 256 registers for the kernel and for ll_step: enough
    using State = LanderState;
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u, float *row) { ll_reset(s, u, row); }
    __device__ static __forceinline__ void observe(const State &s, float (&obs)[S]) { ll_obs(s, obs); }
    __device__ static __forceinline__ float step(State &s, const float (&act)[A], bool &done) { return ll_step(s, act[0], act[1], done); }
};

struct WalkerMlpEnv {
    static constexpr int S = 24, A = 4, INIT_W = 4, ROW = BW_TERRAIN_ROW;
    // one wave per SIMD: bw_step (compiled for its callers' budget) may then use all 512 registers -- the walker's
    // world does not fit 256, and what spills goes to AGPRs (one v_accvgpr move) instead of scratch memory (a trip
    // to L2 or HBM inside the 180-iteration solver loop)
    static constexpr int WAVES_PER_SIMD = WALKER_MLP_WAVES_PER_SIMD;
    using State = WalkerState;
    __device__ static __forceinline__ void reset(State &s, const float *__restrict__ u, float *row) { bw_reset(s, u, row); }
    __device__ static __forceinline__ void observe(const State &s, float (&obs)[S]) { bw_obs(s, obs); }
    __device__ static __forceinline__ float step(State &s, const float (&act)[A], bool &done)
    {
        return bw_step(s, act[0], act[1], act[2], act[3], done);
    }
};

template <class EnvB, int LPE>
__global__ __launch_bounds__(64, EnvB::WAVES_PER_SIMD) void k_rollout_box2d_mlp(const float *__restrict__ theta,
                                                           const float *__restrict__ init, int init_per_offspring,
                                                           int n_rows, int E, int P, int max_step, uint32_t obs_mask,
                                                           int envs_per_wave, double *__restrict__ ep_return,
                                                           int32_t *__restrict__ ep_steps)
{
    constexpr int S = EnvB::S, A = EnvB::A;
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ float terrain[64 / LPE][EnvB::ROW];                // one terrain row per env
    stage_tanh_table(tanh_tab);
    // envs_per_wave <= 64 / LPE envs in this wave; the lane groups past the last one shadow it (same env, same path:
    // they add nothing to what the wave executes) -- a wave-step costs about as much as it carries DIFFERENT envs
    const int n_env = n_rows * E;
    const int group = (int)threadIdx.x / LPE;
    const int slot = group < envs_per_wave ? group : envs_per_wave - 1;
    int env = (int)blockIdx.x * envs_per_wave + slot;
    const int sub = (int)(threadIdx.x % LPE);
    const bool valid = env < n_env && group < envs_per_wave;
    env = env < n_env ? env : n_env - 1;
    const int row = env / E, ep = env - row * E;
    typename EnvB::State st;
    EnvB::reset(st, init + ((size_t)(init_per_offspring ? row : 0) * E + ep) * EnvB::INIT_W, terrain[slot]);
#ifdef SES_PHASE_TIMERS
    phase_mark(-1);
#endif
    double ret = 0.0;
    int steps = 0;
    bool done = false;
    for (int t = 0; t < max_step; ++t) {
        if (__ballot(!done) == 0ull) break;
        // the lane's weight slice is re-read from the (L2-resident) row every step: a few dozen loads next to a
        // 20 000-instruction world step, and nothing of the policy has to stay in registers across it
        float obs[S], logits[A], act[A];
#ifdef SES_PHASE_TIMERS
        phase_mark(10);
#endif
        EnvB::observe(st, obs);
#pragma unroll
        for (int k = 0; k < S; ++k) obs[k] = ((obs_mask >> k) & 1u) ? 0.0f : obs[k];
        if constexpr (LPE > 8) {
            // 16, 32 or 64 lanes per env: small populations, where an env that has a wave (or a good part of one) to itself
            // pays for its own contacts, impacts and position iterations only, not for the union over its wave-mates'.
            // The policy runs on each 16-lane row of the env's lanes (2 hidden units per lane, MlpSlice<.., 16>: ~90
            // instructions and 30 weight loads per step; round 2 had every lane evaluate the whole policy from streamed
            // weights: ~930 instructions and 420 dependent-ish loads, a tenth of a lander step)
            MlpSlice<S, A, 16> net;
            net.load(theta + (size_t)row * P, (int)(threadIdx.x & 15));
            net.forward(tanh_tab, obs, logits);
        } else if constexpr (LPE >= 4) {
            MlpSlice<S, A, LPE> net;
            net.load(theta + (size_t)row * P, sub);
            net.forward(tanh_tab, obs, logits);
        } else {
            mlp_forward_streamed<S, A, LPE>(theta + (size_t)row * P, sub, tanh_tab, obs, logits);
        }
#pragma unroll
        for (int k = 0; k < A; ++k) act[k] = tanh_(tanh_tab, logits[k]);
#ifdef SES_PHASE_TIMERS
#pragma unroll
        for (int k = 0; k < A; ++k) asm volatile("" : "+v"(act[k]));   // the policy is done before the mark
        phase_mark(11);
#endif
        if (!done) {                                               // a finished env is frozen
            ret += (double)EnvB::step(st, act, done);
            steps += 1;
        }
    }
    if (valid && sub == 0) {
        ep_return[env] = ret;
        if (ep_steps) ep_steps[env] = steps;
    }
#ifdef SES_PHASE_TIMERS
    phase_flush();
#endif
}

// simple_spread: NA agents per env share the offspring's MLP (utils.py:4-8: one deepcopy per agent, same
// weights); per cycle every agent is evaluated on its own observation, then the world steps once
// (pettingzoo_wrapper.py:36-52).  8 lanes per env: with S = 6*NA inputs the lane's weight slice is
// 4 x (S + 1 + 5) registers.  Episodes last max_cycles (25) steps, so this kernel is short and dominated by
// the one-time weight load; nothing is early-exited (all agents finish together).
template <int NA>
__global__ __launch_bounds__(64) void k_rollout_spread_mlp(const float *__restrict__ theta,
                                                           const float *__restrict__ init, int init_per_offspring,
                                                           int n_rows, int E, int P, int max_cycles,
                                                           double *__restrict__ ep_return)
{
    constexpr int LPE = 8, S = 6 * NA, A = 5;
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    stage_tanh_table(tanh_tab);
    const long long gtid = (long long)blockIdx.x * 64 + threadIdx.x;
    const int n_env = n_rows * E;
    int env = (int)(gtid / LPE);
    const int sub = (int)(threadIdx.x % LPE);
    const bool valid = env < n_env;
    env = valid ? env : n_env - 1;
    const int row = env / E;
    const int ep = env - row * E;
    MlpSlice<S, A, LPE> net;
    net.load(theta + (size_t)row * P, sub);
    const float *s0 = init + ((size_t)(init_per_offspring ? row : 0) * E + ep) * (4 * NA);
    SpreadState<NA> st;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        st.ax[i] = s0[2 * i]; st.ay[i] = s0[2 * i + 1];
        st.vx[i] = 0.0f; st.vy[i] = 0.0f;
        st.lx[i] = s0[2 * NA + 2 * i]; st.ly[i] = s0[2 * NA + 2 * i + 1];
    }
    double ret = 0.0;
    for (int t = 0; t < max_cycles; ++t) {
        int action[NA];
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            float obs[S], logits[A];
            spread_obs<NA>(st, a, obs);
            net.forward(tanh_tab, obs, logits);
            action[a] = argmax_first<A>(logits);
        }
        ret += (double)spread_step<NA, true>(st, action, sub & 3);
    }
    if (valid && sub == 0) ep_return[env] = ret;
}

__global__ void k_fitness_mean(const double *__restrict__ ep_return, int n_rows, int E, float *__restrict__ fitness,
                               unsigned long long *__restrict__ stamp)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (stamp && i == 0) *stamp = real_time();                          // end of the rollout phase (ses_set_stamp)
    if (i >= n_rows) return;
    double total = 0.0;
    for (int e = 0; e < E; ++e) total += ep_return[(size_t)i * E + e];
    fitness[i] = (float)(total / (double)E);
}

// The same mean, and the fitness exchange of a sharded run in the same launch (ses_run_generations, "fused_fitness_exchange"):
// every thread also stores its value as an 8-byte {exchange number, value} granule into the mailbox of EVERY rank (its own
// included) -- one store per rank, the data is its own flag -- where the ranks' rank kernels poll the tiles they sort
// (k_rank_sort_search).  No exchange launch between the rollout and the tail.
__global__ void k_fitness_mean_granules(const double *__restrict__ ep_return, int n_rows, int E, float *__restrict__ fitness,
                                        unsigned long long *__restrict__ stamp, P2pGranuleView gv)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (stamp && i == 0) *stamp = real_time();
    if (i >= n_rows) return;
    double total = 0.0;
    for (int e = 0; e < E; ++e) total += ep_return[(size_t)i * E + e];
    const float f = (float)(total / (double)E);
    fitness[i] = f;
    for (int r = 0; r < gv.world; ++r) granule_store(gv.dst[r] + i, gv.seq, f2u(f));
}

// ------------------------------------------------------------------------------------------------
// Standalone SoA env step: pure streaming, 16 B per lane per array (7 loads + 6 stores = 52 B/env).
template <bool FIXED_LENGTH>
__device__ __forceinline__ void env_step_one(float &x, float &xd, float &th, float &thd, int action, float &ret,
                                             uint32_t &status, int max_step)
{
    const bool done = (status >> 31) != 0u;
    const uint32_t steps = status & 0x7fffffffu;
    CartPoleState s{x, xd, th, thd};
    const bool term = cartpole_step(s, action);
    const bool advance = FIXED_LENGTH ? true : !done;
    x = advance ? s.x : x;
    xd = advance ? s.xd : xd;
    th = advance ? s.th : th;
    thd = advance ? s.thd : thd;
    const uint32_t nsteps = steps + 1u;
    const bool now_done = term | (max_step > 0 && (int)nsteps >= max_step);
    ret = done ? ret : ret + 1.0f;
    status = done ? status : (nsteps | ((uint32_t)now_done << 31));
}

// 16-byte non-temporal accesses: the state is streamed once per step and never re-read by this kernel,
// so it should not displace anything in L2 / Infinity Cache (measured +7 % over plain loads/stores).
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

template <bool FIXED_LENGTH>
__global__ __launch_bounds__(256) void k_env_step_cartpole_v4(int n4, int max_step, f32x4 *__restrict__ x,
                                                              f32x4 *__restrict__ xd, f32x4 *__restrict__ th,
                                                              f32x4 *__restrict__ thd,
                                                              const i32x4 *__restrict__ action,
                                                              f32x4 *__restrict__ ret, u32x4 *__restrict__ status)
{
    const int stride = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        f32x4 vx = __builtin_nontemporal_load(x + i), vxd = __builtin_nontemporal_load(xd + i),
              vth = __builtin_nontemporal_load(th + i), vthd = __builtin_nontemporal_load(thd + i),
              vr = __builtin_nontemporal_load(ret + i);
        const i32x4 va = __builtin_nontemporal_load(action + i);
        u32x4 vs = __builtin_nontemporal_load(status + i);
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            float ex = vx[l], exd = vxd[l], eth = vth[l], ethd = vthd[l], er = vr[l];
            uint32_t es = vs[l];
            env_step_one<FIXED_LENGTH>(ex, exd, eth, ethd, va[l], er, es, max_step);
            vx[l] = ex; vxd[l] = exd; vth[l] = eth; vthd[l] = ethd; vr[l] = er; vs[l] = es;
        }
        __builtin_nontemporal_store(vx, x + i);
        __builtin_nontemporal_store(vxd, xd + i);
        __builtin_nontemporal_store(vth, th + i);
        __builtin_nontemporal_store(vthd, thd + i);
        __builtin_nontemporal_store(vr, ret + i);
        __builtin_nontemporal_store(vs, status + i);
    }
}

// The env-step kernel's 13 streams with no arithmetic in between (7 x 16-B non-temporal loads, 6 x 16-B non-temporal
// stores per lane, same grid): what the memory system of THIS box gives this access pattern -- the ceiling bench.py
// prints next to the env-step kernel (ses_stream_probe).  Every loaded vector passes through an empty asm statement, so
// that neither a load nor a store-back of an unchanged value can be dropped (tests/test_profiles_current.py counts them).
__global__ __launch_bounds__(256) void k_stream_probe13(int n4, f32x4 *__restrict__ x, f32x4 *__restrict__ xd,
                                                        f32x4 *__restrict__ th, f32x4 *__restrict__ thd,
                                                        const i32x4 *__restrict__ action, f32x4 *__restrict__ ret,
                                                        u32x4 *__restrict__ status)
{
    const int stride = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        f32x4 vx = __builtin_nontemporal_load(x + i);
        const f32x4 vxd = __builtin_nontemporal_load(xd + i), vth = __builtin_nontemporal_load(th + i),
                    vthd = __builtin_nontemporal_load(thd + i), vr = __builtin_nontemporal_load(ret + i);
        const i32x4 va = __builtin_nontemporal_load(action + i);
        const u32x4 vs = __builtin_nontemporal_load(status + i);
        asm volatile("" ::"v"(va));                               // the action stream is loaded (and consumed here), never stored
        // opaque to the optimiser: without this, storing a value back to the address it was loaded from is dropped
        f32x4 wxd = vxd, wth = vth, wthd = vthd, wr = vr;
        u32x4 ws = vs;
        asm volatile("" : "+v"(vx), "+v"(wxd), "+v"(wth), "+v"(wthd), "+v"(wr), "+v"(ws));
        __builtin_nontemporal_store(vx, x + i);
        __builtin_nontemporal_store(wxd, xd + i);
        __builtin_nontemporal_store(wth, th + i);
        __builtin_nontemporal_store(wthd, thd + i);
        __builtin_nontemporal_store(wr, ret + i);
        __builtin_nontemporal_store(ws, status + i);
    }
}

template <bool FIXED_LENGTH>
__global__ void k_env_step_cartpole_scalar(int first, int n, int max_step, float *x, float *xd, float *th, float *thd,
                                           const int32_t *action, float *ret, uint32_t *status)
{
    const int i = first + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float vx = x[i], vxd = xd[i], vth = th[i], vthd = thd[i], vr = ret[i];
    uint32_t vs = status[i];
    env_step_one<FIXED_LENGTH>(vx, vxd, vth, vthd, action[i], vr, vs, max_step);
    x[i] = vx; xd[i] = vxd; th[i] = vth; thd[i] = vthd; ret[i] = vr; status[i] = vs;
}

// k_rollout_cartpole_mlp is named HERE ONLY.  First-use order of its instances (see ses_internal.h, "load-bearing"):
// FIXED_LENGTH true before false.
template <int LPE, int BLOCK, bool PK = false, bool PHYS64 = false>
static void launch_rollout_b(const ses_handle *h, const RolloutArgs &a, int mode)
{
    const dim3 grid(ceil_div(a.episodes() * LPE, BLOCK)), block(BLOCK);
    with_fixed_length(mode, [&](auto fixed) {
        launch_rollout_kernel(h, k_rollout_cartpole_mlp<LPE, fixed(), BLOCK, PHYS64, PK>, grid, block, a);
    });
}

// (first-use order: the packed form where it exists, then BLOCK 256, then 64)
template <int LPE>
static void launch_rollout(const ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode)
{
    if constexpr (LPE == 8 || LPE == 16) {
        if (plan.packed) {
            launch_rollout_b<LPE, 64, true>(h, a, mode);
            return;
        }
    }
    if (plan.block == 256) launch_rollout_b<LPE, 256>(h, a, mode);
    else launch_rollout_b<LPE, 64>(h, a, mode);
}

// (first-use order of the instances: 64 lanes per env down to 1)
template <class EnvB>
static void launch_box2d_mlp(const ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan)
{
    const int lpe = plan.box2d_lpe, epw = plan.box2d_epw;
    const dim3 grid(ceil_div(a.episodes(), epw)), block(64);
    const auto launch = [&](auto lanes) { launch_rollout_kernel(h, k_rollout_box2d_mlp<EnvB, lanes()>, grid, block, a, epw); };
    if (!with_lanes<64, 32, 16, 8, 4, 2, 1>(lpe, launch)) with_lanes<1>(1, launch);      // any other value: one lane per env
}

// the handle's env is the one whose row runs rollout_cartpole (ses_env_table.h)
static bool runs_cartpole(const ses_handle *h)
{
    const EnvDesc *d = env_desc(h);
    return d && d->rollout == rollout_cartpole;
}

// what the tail asks about the NEXT rollout (ses_strategy.hip); the rule is the plan's, and rollout_with reads the plan it formed
bool cartpole_perturb_rollout_ok(const ses_handle *h, int n_rows, int mode)
{
    return n_rows >= 1 && plan_rollout(h->cfg, h->tune, h->P, n_rows, mode).own_rows_ok;
}

static void launch_cartpole_mlp_pairs_perturb(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan);   // (defined last: emission order)
static void launch_cartpole_mlp_pairs_packed(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan);    // (likewise)

// (first-use order: the handover kernel, the mixes with FIXED_LENGTH true then false, the pure splits 1, 2, 4, 16, 32, 8; the
//  prologue form of the handover kernel comes behind ses_policy_forward's kernels, the HEAVY_PK instances of both last in the unit)
static void launch_cartpole_mlp(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode)
{
    if (plan.lanes_light) {
        // one wave of the first kind per SIMD (the dispatcher deals the first workgroups one per SIMD) + the rest
        const int waves_light = plan.waves_light, waves_rest = plan.waves_rest, handover = plan.handover;
        const dim3 grid(waves_light + waves_rest), block(64);
        if (plan.family == RolloutFamily::CartPoleMlpPair) {
            // one light and one heavy wave per SIMD, swapping work at step `handover` (k_rollout_cartpole_mlp_handover)
            h->count_pair_rollouts += 1;
            if (a.prologue) {                                            // ... which forms its own rows first (rollout_with checked that it may)
                launch_cartpole_mlp_pairs_perturb(h, a, plan);
                return;
            }
            if (plan.heavy_packed) {
                launch_cartpole_mlp_pairs_packed(h, a, plan);
                return;
            }
            launch_rollout_kernel(h, k_rollout_cartpole_mlp_handover<true>, dim3(ceil_div(waves_light, HANDOVER_PAIRS)),
                                  dim3(64 * 2 * HANDOVER_PAIRS), a, waves_light, waves_rest, handover, h->tune.rollout_heavy_prio_steps);
            return;
        }
        with_fixed_length(mode, [&](auto fixed) {
            constexpr bool FIXED = fixed();
            const auto mix = [&](auto light, auto rest) {
                launch_rollout_kernel(h, k_rollout_cartpole_mlp_mix<FIXED, light(), rest()>, grid, block, a, waves_light);
            };
            if (plan.lanes_rest == 16) mix(lanes_c<8>{}, lanes_c<16>{});
            else if (plan.lanes_light == 16) mix(lanes_c<16>{}, lanes_c<4>{});
            else mix(lanes_c<8>{}, lanes_c<4>{});
        });
        return;
    }
    const auto launch = [&](auto lanes) { launch_rollout<lanes()>(h, a, plan, mode); };
    if (!with_lanes<1, 2, 4, 16, 32, 8>(plan.lanes_rest, launch)) with_lanes<8>(8, launch);          // any other value: 8 lanes per env
}

// launch shape of the standalone env-step kernel (and of the probe that has to match it): see ses_env_step
struct EnvStepShape {
    int blocks, block, lds;
};
// The LDS reservation that limits the waves in flight.  Knob "env_step_lds_bytes" >= 0: taken as given.  -1 (default):
// derived from the device -- its LDS per CU divided by the workgroups per CU that make "env_step_waves_per_cu" (7) waves,
// rounded down to 256 bytes and checked against the occupancy calculator (the allocation granule is the hardware's
// business: if the rounded figure still lets one more workgroup in, or one fewer, it is moved by 256 bytes until the
// calculator agrees).  Resolved once per (block, knobs); env_step_wpc is what the calculator says in the end.
static void env_step_resolve(ses_handle *h)
{
    const int block = h->tune.env_step_block;
    if (h->env_step_key[0] == block && h->env_step_key[1] == h->tune.env_step_lds && h->env_step_key[2] == h->tune.env_step_waves) return;
    auto occupancy = [&](int lds) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_env_step_cartpole_v4<true>, block, (size_t)lds) != hipSuccess) {
            (void)hipGetLastError();
            nb = 0;
        }
        return nb;
    };
    int lds = h->tune.env_step_lds;
    if (lds < 0) {
        int wgs = h->tune.env_step_waves * 64 / block;                     // workgroups per CU that make the wanted waves
        if (wgs < 1) wgs = 1;
        lds = h->lds_per_cu > 0 ? h->lds_per_cu / wgs / 256 * 256 : 0;
        if (lds > 65536) lds = 65536;                                       // what one workgroup may ask for
        for (int tries = 0; tries < 16 && lds > 256; ++tries) {
            const int nb = occupancy(lds);
            if (nb == 0 || nb == wgs) break;                                // (0: no calculator -- keep the arithmetic figure)
            if (nb < wgs) lds -= 256;                                       // a granule rounded it up past the share
            else if (lds + 256 <= 65536 && occupancy(lds + 256) >= wgs) lds += 256;
            else break;
        }
    }
    h->env_step_lds_resolved = lds;
    h->env_step_wpc = occupancy(lds) * block / 64;
    h->env_step_key[0] = block; h->env_step_key[1] = h->tune.env_step_lds; h->env_step_key[2] = h->tune.env_step_waves;
}

static EnvStepShape env_step_shape(ses_handle *h, int n4)
{
    EnvStepShape sh;
    env_step_resolve(h);
    sh.block = h->tune.env_step_block;
    sh.lds = h->env_step_lds_resolved;
    const long long want = ceil_div((long long)n4, sh.block);
    sh.blocks = want < (1 << 20) ? (int)want : (1 << 20);                   // beyond that the kernel strides
    return sh;
}

// ---- one rollout_<env>() per env family (ses_rollout).  Their order in this file and the order of the kernels inside
// them is the first-use order that ses_internal.h ("load-bearing") speaks of: LunarLander, BipedalWalker, simple_spread,
// CartPole float64, CartPole GRU -- behind launch_cartpole_mlp and env_step_resolve above.
int rollout_lander(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode)
{
    SES_REQUIRE(mode == SES_MODE_EPISODIC, "ses_rollout: LunarLander has no fixed-length mode");
    if (h->cfg.discrete_action) {
        // LunarLander-v2: the same forms and wave shapes under the kernels of ses_lander_discrete.hip
        return lander_discrete_rollout(h, a, plan.gru_form, plan.box2d_lpe, plan.box2d_epw);
    }
    const dim3 block(256);                                              // the GRU kernels: four waves per workgroup
    if (h->cfg.gru) {
        switch (const GruForm form = plan.gru_form) {
            case GruForm::EpisodeParallel:
            case GruForm::Sequential: {                                     // one wave per (offspring, episode) / per offspring
                const bool epp = form == GruForm::EpisodeParallel;
                hipLaunchKernelGGL(k_rollout_lander_gru, dim3(ceil_div(epp ? a.episodes() : a.n_rows, 4)), block, 0, h->stream, a.theta,
                                   a.init, a.per, a.n_rows, a.E, a.P, a.max_step, a.obs_mask, a.epr, a.ep_steps, epp ? 1 : 0);
                break;
            }
            case GruForm::Mfma:
                launch_rollout_kernel(h, k_rollout_gru_mfma<LanderLs, false>, dim3(ceil_div(a.n_rows, 4)), block, a);
                break;
            case GruForm::LockstepMulti4:
                launch_rollout_kernel(h, k_rollout_gru_lockstep_multi<LanderLs, 4>, dim3(ceil_div(a.n_rows, 16)), block, a);
                break;
            case GruForm::LockstepMulti2:
                launch_rollout_kernel(h, k_rollout_gru_lockstep_multi<LanderLs, 2>, dim3(ceil_div(a.n_rows, 8)), block, a);
                break;
            default:
                launch_rollout_kernel(h, k_rollout_gru_lockstep<LanderLs, false, 1>, dim3(a.n_rows), dim3(64), a);
                break;
        }
    } else {
        launch_box2d_mlp<LanderMlpEnv>(h, a, plan);
    }
    return SES_OK;
}

int rollout_walker(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode)
{
    SES_REQUIRE(mode == SES_MODE_EPISODIC, "ses_rollout: BipedalWalker has no fixed-length mode");
    SES_REQUIRE(!h->cfg.gru, "ses_rollout: BipedalWalker has an MLP-policy kernel only (conf/bipedalwalker.yaml: gru False)");
    launch_box2d_mlp<WalkerMlpEnv>(h, a, plan);
    return SES_OK;
}

int rollout_spread(ses_handle *h, const RolloutArgs &a, const RolloutPlan &, int)                 // (either mode: every episode is 25 cycles)
{
    SES_REQUIRE(a.ep_steps == nullptr, "ses_rollout: simple_spread episodes have a fixed length, no ep_steps");
    if (h->cfg.gru) return spread_gru_rollout(h, a);                   // ses_spread_gru.hip
    const dim3 grid(ceil_div(a.episodes() * 8, 64)), block(64);
    with_lanes<2, 3>(h->cfg.n_agents == 2 ? 2 : 3, [&](auto agents) {
        hipLaunchKernelGGL(k_rollout_spread_mlp<agents()>, grid, block, 0, h->stream, a.theta, a.init, a.per, a.n_rows, a.E, a.P,
                           a.max_step, a.epr);
    });
    return SES_OK;
}

int rollout_cartpole(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode)
{
    const dim3 rows4(ceil_div(a.n_rows, 4)), block(256);                // the GRU kernels: four offspring (waves) per workgroup
    if (h->cfg.physics64) {
        // gym-order float64 dynamics: GRU lockstep or MLP at 4 / 8 lanes per env (parity option, not the bench path)
        if (h->cfg.gru)
            with_fixed_length(mode, [&](auto fixed) {
                launch_rollout_kernel(h, k_rollout_gru_lockstep<CartPoleLs64, fixed(), 4>, rows4, block, a);
            });
        else if (plan.lanes_rest >= 8) launch_rollout_b<8, 64, false, true>(h, a, mode);
        else launch_rollout_b<4, 64, false, true>(h, a, mode);
    } else if (h->cfg.gru) {
        switch (const GruForm form = plan.gru_form) {
            case GruForm::EpisodeParallel:
            case GruForm::Sequential: {                                     // one wave per (offspring, episode) / per offspring
                const bool epp = form == GruForm::EpisodeParallel;
                const dim3 grid(ceil_div(epp ? a.episodes() : a.n_rows, 4));
                with_fixed_length(mode, [&](auto fixed) {
                    hipLaunchKernelGGL(k_rollout_cartpole_gru<fixed()>, grid, block, 0, h->stream, a.theta, a.init, a.per, a.n_rows, a.E,
                                       a.P, a.max_step, a.obs_mask, a.epr, a.ep_steps, epp ? 1 : 0);
                });
                break;
            }
            case GruForm::Mfma4:    // 4x4x1 MFMA blocks (ses_gru_mfma4.h): the policy step costs the same for any eval_ep_num up to 8
                with_fixed_length(mode, [&](auto fixed) {
                    launch_rollout_kernel(h, k_rollout_gru_mfma4<CartPoleLs, fixed()>, rows4, block, a);
                });
                break;
            case GruForm::Mfma:
                with_fixed_length(mode, [&](auto fixed) {
                    launch_rollout_kernel(h, k_rollout_gru_mfma<CartPoleLs, fixed()>, rows4, block, a);
                });
                break;
            default:
                with_fixed_length(mode, [&](auto fixed) {
                    launch_rollout_kernel(h, k_rollout_gru_lockstep<CartPoleLs, fixed(), 4>, rows4, block, a);
                });
                break;
        }
    } else {
        launch_cartpole_mlp(h, a, plan, mode);
    }
    return SES_OK;
}

// ses_rollout with what ses_run_generations fuses into it (RolloutOpts, ses_internal.h)
int rollout_with(ses_handle *h, const float *theta, const float *init, int32_t init_per_offspring, int32_t n_rows, int32_t mode,
                 float *fitness, double *ep_return, int32_t *ep_steps, RolloutOpts &o)
{
    SES_REQUIRE(h && theta && init && fitness, "ses_rollout: null argument");
    SES_REQUIRE(n_rows >= 1, "ses_rollout: n_rows must be >= 1");
    SES_REQUIRE(mode == SES_MODE_EPISODIC || mode == SES_MODE_FIXED_LENGTH, "ses_rollout: bad mode %d", mode);
    SES_REQUIRE((long long)n_rows * h->cfg.eval_ep_num * 16 < (1ll << 31), "ses_rollout: shard too large");
    const EnvDesc *env = env_desc(h);
    SES_REQUIRE(env, "ses_rollout: handle has no env");
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    const size_t episodes = (size_t)n_rows * h->cfg.eval_ep_num;
    double *epr = ep_return;
    if (!epr) {
        int rc = ensure_episode_scratch(h, episodes);
        if (rc != SES_OK) return rc;
        epr = h->ep_return;
    }
    RolloutArgs a{theta, init, init_per_offspring, n_rows, h->cfg.eval_ep_num, h->P, h->cfg.max_step, h->obs_mask, epr, ep_steps, nullptr};
    const RolloutPlan plan = plan_rollout(h->cfg, h->tune, h->P, n_rows, mode);   // the launch form, decided once (ses_rollout_plan.h)
    int rc;
    // A normaliser bound to the handle (ses_obs_norm_bind; float64 envs, MLP): the rollout normalises with its affine and, update
    // on, leaves per-env statistics in the handle's scratch, which a merge launch between the rollout and the episode mean folds in.
    const bool norm_update = h->obs_norm_stats && h->obs_norm_update;
    if (h->obs_norm_stats) {
        if (h->comm && h->comm_world > 1)
            return set_error(SES_ERR_UNSUPPORTED, "ses_rollout: an observation normaliser is bound and the handle has a communicator of "
                                                  "world %d; one GPU only: the statistics would need an exchange", h->comm_world);
        a.norm_affine = h->obs_norm_affine;
        if (norm_update) {
            rc = ensure_obs_norm_scratch(h, (size_t)(2 * h->cfg.num_state + 1) * episodes);
            if (rc != SES_OK) return rc;
            a.norm_partials = h->obs_norm_partials;
        }
    }
    // The previous generation's tail left its last launch to this rollout: it is taken if this is the rollout the tail decided
    // for -- these rows, the whole population, the pair kernel -- and launched first otherwise.
    if (const PerturbUpdate *u = o.apply_first) {
        o.apply_first = nullptr;
        // (the prologue stores its rows 8 bytes at a time: an even P -- own_rows_ok -- and a population that starts
        //  on an 8-byte boundary, as every device allocation does; a view that does not takes the launch)
        if (theta == u->theta && n_rows == u->n_rows && (uintptr_t)u->theta % 8 == 0 && plan.own_rows_ok) {
            a.prologue = u;
        } else {
            rc = launch_apply_perturb(h, *u);
            if (rc != SES_OK) return rc;
        }
    }
    rc = env->rollout(h, a, plan, mode);
    if (rc != SES_OK) return rc;
    if (norm_update) {
        rc = f64_obs_norm_merge(h, h->obs_norm_partials, (int)episodes, h->obs_norm_stats, h->obs_norm_affine);
        if (rc != SES_OK) return rc;
    }
    if (o.leave_episodes) {
        // (ses_run_generations on one GPU: the tail forms the means itself, k_rank_count_episodes / k_elite_rank_select_small)
        SES_REQUIRE(epr == h->ep_return, "ses_rollout: the fused episode mean works on the handle's own episode scratch");
    } else if (o.granules)
        hipLaunchKernelGGL(k_fitness_mean_granules, dim3(ceil_div(n_rows, 256)), dim3(256), 0, h->stream, epr, n_rows,
                           h->cfg.eval_ep_num, fitness, h->stamp, *o.granules);
    else
        hipLaunchKernelGGL(k_fitness_mean, dim3(ceil_div(n_rows, 256)), dim3(256), 0, h->stream, epr, n_rows,
                           h->cfg.eval_ep_num, fitness, h->stamp);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

}  // namespace ses

extern "C" {

int ses_rollout(ses_handle *h, const float *theta, const float *init, int32_t init_per_offspring, int32_t n_rows,
                int32_t mode, float *fitness, double *ep_return, int32_t *ep_steps)
{
    ses::RolloutOpts none{};
    return ses::rollout_with(h, theta, init, init_per_offspring, n_rows, mode, fitness, ep_return, ep_steps, none);
}

int ses_env_step(ses_handle *h, int32_t n, int32_t mode, float *x, float *xd, float *th, float *thd,
                 const int32_t *action, float *ret, uint32_t *status)
{
    using namespace ses;
    SES_REQUIRE(h && x && xd && th && thd && action && ret && status, "ses_env_step: null argument");
    SES_REQUIRE(n >= 1, "ses_env_step: n must be >= 1");
    SES_REQUIRE(mode == SES_MODE_EPISODIC || mode == SES_MODE_FIXED_LENGTH, "ses_env_step: bad mode %d", mode);
    SES_REQUIRE(runs_cartpole(h), "ses_env_step: handle has no env");
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    const uintptr_t align = (uintptr_t)x | (uintptr_t)xd | (uintptr_t)th | (uintptr_t)thd | (uintptr_t)action |
                            (uintptr_t)ret | (uintptr_t)status;
    const int n4 = (align & 15u) ? 0 : n / 4;  // unaligned arrays take the scalar path entirely
    const int max_step = h->cfg.max_step;
    if (n4 > 0) {
        // One float4 group per thread, a one-shot grid -- and FEW WAVES IN FLIGHT: single-wave workgroups that each reserve
        // a seventh of the CU's LDS (22.5 KB of 160 on gfx950; derived from the device, env_step_resolve) without touching
        // it, so that a CU holds 7 of them instead of 32 waves.  Thirteen streams from 8192
        // resident waves thrash the memory system's open pages; from 1792 they do not: 2^24 envs, same box, interleaved
        // (tools/envstep_ab.hip): 256 threads / no limit 152.5 us = 0.715 of 8 TB/s; 5 / 6 / 7 / 8 / 10 / 12 / 16 waves per CU
        // 148.0 / 132.1 / 132.1 / 133.9 / 134.4 / 141.1 / 151.1 us -- 0.826 at 6-7, above a plain two-stream copy (0.805).
        // ses_set_tuning "env_step_block" / "env_step_waves_per_cu" / "env_step_lds_bytes" (-1 = derive; 0 with block 256 = the
        // old shape: no reservation).
        const EnvStepShape sh = env_step_shape(h, n4);
        with_fixed_length(mode, [&](auto fixed) {
            hipLaunchKernelGGL(k_env_step_cartpole_v4<fixed()>, dim3(sh.blocks), dim3(sh.block), sh.lds, h->stream, n4, max_step,
                               (f32x4 *)x, (f32x4 *)xd, (f32x4 *)th, (f32x4 *)thd, (const i32x4 *)action, (f32x4 *)ret,
                               (u32x4 *)status);
        });
    }
    const int first = n4 * 4;
    if (first < n) {
        const int blocks = ceil_div(n - first, 256);
        with_fixed_length(mode, [&](auto fixed) {
            hipLaunchKernelGGL(k_env_step_cartpole_scalar<fixed()>, dim3(blocks), dim3(256), 0, h->stream, first, n, max_step, x, xd,
                               th, thd, action, ret, status);
        });
    }
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int ses_env_step_shape(ses_handle *h, int32_t *block, int32_t *lds_bytes, int32_t *waves_per_cu, int32_t *lds_per_cu)
{
    using namespace ses;
    SES_REQUIRE(h, "ses_env_step_shape: null handle");
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    env_step_resolve(h);
    if (block) *block = h->tune.env_step_block;
    if (lds_bytes) *lds_bytes = h->env_step_lds_resolved;
    if (waves_per_cu) *waves_per_cu = h->env_step_wpc;
    if (lds_per_cu) *lds_per_cu = h->lds_per_cu;
    return SES_OK;
}

int ses_stream_probe(ses_handle *h, int32_t n, float *x, float *xd, float *th, float *thd, const int32_t *action, float *ret,
                     uint32_t *status)
{
    using namespace ses;
    SES_REQUIRE(h && x && xd && th && thd && action && ret && status, "ses_stream_probe: null argument");
    const uintptr_t align = (uintptr_t)x | (uintptr_t)xd | (uintptr_t)th | (uintptr_t)thd | (uintptr_t)action |
                            (uintptr_t)ret | (uintptr_t)status;
    SES_REQUIRE(n >= 4 && (n & 3) == 0 && (align & 15u) == 0, "ses_stream_probe: n must be a multiple of 4 and the arrays 16-byte aligned");
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    const int n4 = n / 4;
    const EnvStepShape sh = env_step_shape(h, n4);                                       // the env-step kernel's launch shape
    hipLaunchKernelGGL(k_stream_probe13, dim3(sh.blocks), dim3(sh.block), sh.lds, h->stream, n4, (f32x4 *)x, (f32x4 *)xd, (f32x4 *)th,
                       (f32x4 *)thd, (const i32x4 *)action, (f32x4 *)ret, (u32x4 *)status);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int ses_policy_forward(ses_handle *h, const float *theta, const float *obs, float *hidden, int32_t n, float *logits,
                       float *act, int32_t *action)
{
    using namespace ses;
    SES_REQUIRE(h && theta && obs && logits && action, "ses_policy_forward: null argument");
    SES_REQUIRE(n >= 1 && (long long)n * 4 < (1ll << 31), "ses_policy_forward: n out of range");
    SES_HIP_TRY(hipSetDevice(h->cfg.device));
    const int S = h->cfg.num_state, A = h->cfg.num_action;
    bool known;                                                  // (first-use order: the GRU instances, then the MLP ones, as listed)
    if (h->cfg.gru) {
        SES_REQUIRE(hidden, "ses_policy_forward: GRU policy needs the hidden-state array");
        known = with_policy_shape<PolicyShape<4, 2>, PolicyShape<8, 4>>(S, A, [&](auto sh) {
            hipLaunchKernelGGL((k_policy_forward_gru<sh.S, sh.A>), dim3(ceil_div(n, 4)), dim3(256), 0, h->stream, theta, obs, hidden, n,
                               h->P, logits, act, action);
        });
    } else {
        known = with_policy_shape<PolicyShape<4, 2>, PolicyShape<8, 4>, PolicyShape<12, 5>, PolicyShape<18, 5>, PolicyShape<24, 4>>(
            S, A, [&](auto sh) {
                hipLaunchKernelGGL((k_policy_forward_mlp<sh.S, sh.A>), dim3(ceil_div((long long)n * 4, 64)), dim3(64), 0, h->stream,
                                   theta, obs, n, h->P, logits, act, action);
            });
    }
    if (known) {
        SES_HIP_TRY(hipGetLastError());
        return SES_OK;
    }
    if (!h->cfg.gru && S == 242 && A == 2) return waterworld_policy_forward(h, theta, obs, n, logits, act, action);   // ses_waterworld.hip
    if (!h->cfg.gru && S == 147 && A == 5) return pursuit_policy_forward(h, theta, obs, n, logits, act, action);      // ses_pursuit.hip
    if (is_f64_policy_shape(S, A)) return f64_policy_forward(h, theta, obs, hidden, n, logits, act, action);          // ses_f64_envs.hip
    if (S == 15 && A == 3) return hopper_policy_forward(h, theta, obs, hidden, n, logits, act, action);               // ses_hopper.hip
    if (S == 22 && A == 6) return walker2d_policy_forward(h, theta, obs, hidden, n, logits, act, action);             // ses_walker2d.hip
    if (h->cfg.gru && S == 24 && A == 4)
        return walker_hardcore_policy_forward(h, theta, obs, hidden, n, logits, act, action);                         // ses_walker_hardcore.hip
    if (h->cfg.gru && is_spread_policy_shape(S, A))
        return spread_gru_policy_forward(h, theta, obs, hidden, n, logits, act, action);                              // ses_spread_gru.hip
    if (h->cfg.gru) return set_error(SES_ERR_UNSUPPORTED, "ses_policy_forward: no GRU kernel instance for num_state=%d num_action=%d", S, A);
    return set_error(SES_ERR_UNSUPPORTED, "ses_policy_forward: no kernel instance for num_state=%d num_action=%d", S, A);
}

}  // extern "C"

namespace ses {

// (the last kernel instances of the unit, in this order: the prologue form, then the HEAVY_PK instances of both pair kernels; nothing
//  that was emitted before them moves)
static void launch_cartpole_mlp_pairs_perturb(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan)
{
    h->count_perturb_rollouts += 1;
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(ceil_div(plan.waves_light, HANDOVER_PAIRS)), dim3(64 * 2 * HANDOVER_PAIRS),
                           perturb_rollout_lds(a.P, a.E), h->stream, a.init, a.per, a.n_rows, a.E, a.P, a.max_step, a.obs_mask,
                           plan.waves_light, plan.waves_rest, plan.handover, h->tune.rollout_heavy_prio_steps, a.epr, a.ep_steps, *a.prologue);
    };
    if (!plan.heavy_packed) launch(k_rollout_cartpole_mlp_handover_perturb<true>);
    else launch(k_rollout_cartpole_mlp_handover_perturb<true, true>);
}

static void launch_cartpole_mlp_pairs_packed(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan)
{
    launch_rollout_kernel(h, k_rollout_cartpole_mlp_handover<true, true>, dim3(ceil_div(plan.waves_light, HANDOVER_PAIRS)),
                          dim3(64 * 2 * HANDOVER_PAIRS), a, plan.waves_light, plan.waves_rest, plan.handover, h->tune.rollout_heavy_prio_steps);
}

}  // namespace ses

#ifdef SES_PHASE_TIMERS
// development build only (tools/walker_phases.py): the phase totals of ses_lander.h's phase_mark, read and optionally cleared
extern "C" int ses_debug_phase_totals(unsigned long long *out24, int reset)
{
    if (hipMemcpyFromSymbol(out24, HIP_SYMBOL(ses::phase_total), ses::PHASE_SLOTS * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[ses::PHASE_SLOTS] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(ses::phase_total), z, sizeof z) != hipSuccess) return -1;
    }
    return 0;
}
#endif
