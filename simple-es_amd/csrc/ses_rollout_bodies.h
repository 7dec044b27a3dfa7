// ses_rollout_bodies.h -- the env-generic batch bodies of the GRU rollouts that more than one unit wraps in kernels:
// ses_rollout.hip (CartPole, LunarLanderContinuous-v2) and ses_lander_discrete.hip (LunarLander-v2).
//   gru_lockstep_multi_batch : lockstep GRU rollout with G offspring per wave
//   gru_mfma_batch           : GRU rollout on v_mfma_f32_16x16x4_f32 tiles, up to 16 episodes per batch
// (gru_lockstep_batch, the one-offspring lockstep body, lives in ses_gru_lockstep.h.)  Both are forceinline: a kernel that
// calls one is the body's code under the kernel's own name and launch bounds.  EnvT adapts an env and decides what the
// policy's outputs mean (tanh head, argmax head); the bodies hand them over as they come.
// The MLP body of k_rollout_box2d_mlp and the sequential GRU body of k_rollout_lander_gru are NOT here: as functions called
// from their kernels they compile to other machine code than inside them, which would move the hashes of ses_rollout.hip's
// kernels (ses_internal.h, "load-bearing"); ses_lander_discrete.hip has kernels of its own for those two forms.
#pragma once
#include "ses_gru.h"
#include "ses_gru_lockstep.h"
#include "ses_gru_mfma.h"
#include "ses_policy.h"
#ifdef SES_PHASE_TIMERS
#include "ses_lander.h"   // phase_mark / phase_flush of the development build
#endif

namespace ses {

// ------------------------------------------------------------------------------------------------
// Lockstep GRU rollout with G offspring per wave, for envs whose step dwarfs the policy (the Box2D-style lander: ~20 000
// instructions per world step against ~600 for the GRU step of five episodes).  An env step costs a wave the same
// number of issue slots whether 5 or 40 of its lanes carry a live env, so the wave takes the envs of G offspring:
// lane l owns env (offspring (l >> 3) % G, episode l & 7), one call of the env step serves G x E envs.  The policy is
// evaluated offspring after offspring by all 64 lanes as in the one-offspring kernel (same arithmetic, same lane roles);
// the weights cannot all stay in registers, so each offspring's slice (~110 floats per lane) is re-read from its theta
// row (L2) before its GRU step -- ~27 KB per offspring and time step, 11 GB per C3 generation, next to 20 000
// instructions of solver per step.  Hidden states stay in registers (G x NP) and in the per-offspring LDS block.
// Measured (C3, 4096 offspring x 5 episodes): see DESIGN.md section 4.
template <typename EnvT, int G, int NP, bool ODD>
__device__ __forceinline__ void gru_lockstep_multi_batch(const TanhEntry *tanh_tab, GruLockstepLds<EnvT::S, EnvT::A> *lds,
                                                         const float *__restrict__ theta, int P, int row0, int n_rows,
                                                         int lane, int nb, const float *__restrict__ init,
                                                         int init_per_offspring, int E, int max_step, uint32_t obs_mask,
                                                         double *__restrict__ ep_return, int32_t *__restrict__ ep_steps)
{
    constexpr int S = EnvT::S, A = EnvT::A;
    const int slot = lane & 7, rep = lane >> 3, gl = rep % G;
    const int my_row_raw = row0 + gl;
    const bool row_valid = my_row_raw < n_rows;
    const int my_row = row_valid ? my_row_raw : n_rows - 1;
    const bool owner_valid = slot < nb && row_valid;
    typename EnvT::State st;
    EnvT::reset(st, init + ((size_t)(init_per_offspring ? my_row : 0) * E + (slot < nb ? slot : 0)) * EnvT::INIT_W, gl * 8 + slot);
    float hreg[G][NP];
#pragma unroll
    for (int g = 0; g < G; ++g) {
#pragma unroll
        for (int p = 0; p < NP; ++p) hreg[g][p] = 0.0f;                           // GymEnvModel.reset()
        const int row_g = row0 + g < n_rows ? row0 + g : n_rows - 1;
        GruLockstep<S, A> net;
        net.template load<true>(theta + (size_t)row_g * P, lane, lds[g]);         // W2 / b2 -> LDS (the registers are dropped)
        if (lane < 32) {
#pragma unroll
            for (int e = 0; e < GL_EB; ++e) lds[g].ah[e][lane][1] = 0.0f;
        }
    }
    wave_lds_sync();
#ifdef SES_PHASE_TIMERS
    phase_mark(-1);
#endif
    double ret = 0.0;
    int steps = 0;
    bool alive = true;
    for (int t = 0; t < max_step; ++t) {
        if (__ballot(alive & owner_valid) == 0ull) break;
#ifdef SES_PHASE_TIMERS
        phase_mark(10);
#endif
        float obs[S];
        EnvT::observe(st, obs);
        float logits[A];
#pragma unroll
        for (int o = 0; o < A; ++o) logits[o] = 0.0f;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            // an offspring all of whose episodes are over needs no policy step any more (wave-uniform test): in the last
            // two thirds of a C3 rollout most waves carry ONE offspring with a long episode, and the other one's weight
            // re-read + GRU step was a tenth of their step
            if (__ballot(alive & owner_valid & (gl == g)) == 0ull) continue;
            const int row_g = row0 + g < n_rows ? row0 + g : n_rows - 1;
            GruLockstep<S, A> net;
            net.template load<false>(theta + (size_t)row_g * P, lane, lds[g]);
            if (rep == g) {                                                       // the first replica group of offspring g
#pragma unroll
                for (int k = 0; k < S; ++k) lds[g].obs[slot][k] = ((obs_mask >> k) & 1u) ? 0.0f : obs[k];
            }
            wave_lds_sync();
            net.template step<NP, ODD>(tanh_tab, lds[g], hreg[g], lane);
            float lg[A];
            net.logits_of(lds[g], lane, lg);
#pragma unroll
            for (int o = 0; o < A; ++o) logits[o] = gl == g ? lg[o] : logits[o];
        }
#ifdef SES_PHASE_TIMERS
#pragma unroll
        for (int o = 0; o < A; ++o) asm volatile("" : "+v"(logits[o]));
        phase_mark(11);
#endif
        bool term;
        const bool freeze = !(alive & owner_valid);
        const float r = EnvT::step(st, logits, tanh_tab, freeze, term);
        const int nsteps = steps + 1;
        const bool finished = term | (nsteps >= max_step);
        ret = alive ? ret + (double)r : ret;
        steps = alive ? nsteps : steps;
        alive = alive & !finished;
    }
    if (owner_valid && rep < G) {
        if (ep_return) ep_return[(size_t)my_row * E + slot] = ret;
        if (ep_steps) ep_steps[(size_t)my_row * E + slot] = steps;
    }
#ifdef SES_PHASE_TIMERS
    phase_flush();
#endif
}

// ------------------------------------------------------------------------------------------------
// MFMA GRU rollout (ses_gru_mfma.h): one offspring per wave, up to 16 episodes are the columns of the
// v_mfma_f32_16x16x4_f32 tiles; lane l simulates the env of episode (l & 15) (four identical replicas, so no lane
// diverges).  Used for eval_ep_num >= 12.  launch_bounds(256, 2): 256 registers, two waves per SIMD.
// SQ counters at E = 16 (tools/prof_mfma.sh): 106 MFMAs + ~600 VALU instructions per step; the matrix pipe is busy 56 %
// of the kernel (MfmaUtil) and SQ_WAIT_INST_ANY is 54 % of the wave cycles: fp32 MFMA executes on the vector lanes
// (its peak IS the vector peak), so the contraction and the VALU phases of the two resident waves take turns instead
// of overlapping -- staggering the waves by a VALU phase changed nothing.
template <typename EnvT, bool FIXED_LENGTH>
__device__ __forceinline__ void gru_mfma_batch(const TanhEntry *tanh_tab, GruMfmaLds<EnvT::S, EnvT::A> &lds,
                                               const GruMfma<EnvT::S, EnvT::A> &net, int lane, int nb,
                                               const float *__restrict__ init_rows, int max_step, uint32_t obs_mask,
                                               double *__restrict__ ret_out, int32_t *__restrict__ steps_out,
                                               bool valid_row)
{
    constexpr int S = EnvT::S, A = EnvT::A;
    const int slot = lane & 15;
    const bool owner_valid = slot < nb;
    typename EnvT::State st;
    EnvT::reset(st, init_rows + (size_t)(owner_valid ? slot : 0) * EnvT::INIT_W, slot);   // padding columns replay episode 0
    float hreg[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) hreg[t][r] = 0.0f;                           // GymEnvModel.reset()
    wave_lds_sync();
    for (int i = lane; i < 32 * GM_EB; i += 64) (&lds.hT[0][0])[i] = 0.0f;
    double ret = 0.0;
    int steps = 0;
    bool alive = true;
    for (int t = 0; t < max_step; ++t) {
        if constexpr (!FIXED_LENGTH) {
            if (__ballot(alive & owner_valid) == 0ull) break;
        }
        float obs[S];
        EnvT::observe(st, obs);
        if (lane < GM_EB) {
#pragma unroll
            for (int k = 0; k < S; ++k) lds.obsT[k][lane] = ((obs_mask >> k) & 1u) ? 0.0f : obs[k];
        }
        wave_lds_sync();
        net.step(tanh_tab, lds, hreg, lane);
        const float4 lg4 = *reinterpret_cast<const float4 *>(&lds.logit[slot][0]);
        const float all[4] = {lg4.x, lg4.y, lg4.z, lg4.w};
        float logits[A];
#pragma unroll
        for (int o = 0; o < A; ++o) logits[o] = all[o];
        bool term;
        const bool freeze = FIXED_LENGTH ? false : !alive;
        const float r = EnvT::step(st, logits, tanh_tab, freeze, term);
        const int nsteps = steps + 1;
        const bool finished = term | (nsteps >= max_step);
        ret = alive ? ret + (double)r : ret;
        steps = alive ? nsteps : steps;
        alive = alive & !finished;
    }
    if (valid_row && lane < GM_EB && owner_valid) {
        if (ret_out) ret_out[slot] = ret;
        if (steps_out) steps_out[slot] = steps;
    }
}

}  // namespace ses
