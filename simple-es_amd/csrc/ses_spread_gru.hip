// ses_spread_gru.hip -- simple_spread with the GRU policy: the recurrent multi-agent rollout and the standalone GRU forward of
// its two shapes, (12, 5) and (18, 5).  A unit of its own, so that the other units keep their machine code.
//
// The reference runs network.gru: True on simple_spread by giving every agent its own deep copy of the offspring's
// GymEnvModel (utils.py:4-8), hence its own hidden state, all of them reset at each episode start (loop.py RolloutWorker).
// Per cycle every agent is evaluated on its own observation of the state BEFORE the step, then the world steps once.
//
// Kernel shape: the lockstep GRU step of ses_gru_lockstep.h -- one offspring's gate weights in the wave's registers, up to 8
// COLUMNS advanced per policy step, the pair cross-over by v_permlane32_swap -- with a column being an (episode, agent) pair:
// column c = NA * env + agent, so a batch is 4 envs at two agents and 2 envs (6 columns) at three; the agents of an env always
// sit in one batch.  Lane l finishes with the logits of column (l & 7) (GruLockstep::logits_of), takes the argmax, and fetches
// the NA actions of its env from the neighbouring lanes of its 8-lane group with ds_bpermute; every lane carries a copy of
// its column's env and steps it with the plain spread_step<NA> (the quad-split form wants four ADJACENT lanes on one env;
// here adjacent lanes are different columns).  Same canonical arithmetic as ses_gru.h / oracle/ses_oracle.c.
#include "ses_gru_lockstep.h"
#include "ses_internal.h"
#include "ses_policy_forward.h"
#include "ses_spread.h"

namespace ses {

// wave-private LDS block: GruLockstepLds with observation rows of S = 12 / 18 floats, padded to a multiple of four so that
// every row -- and every wave's copy of the block -- stays 16-byte aligned (see the note in ses_gru_lockstep.h)
template <int S>
struct alignas(16) SpreadGruLds {
    float ah[GL_EB][32][2];
    float y[GL_EB][36];
    float obs[GL_EB][(S + 3) / 4 * 4];
    float w2[5][32];
    float b2[5];
};

// One batch: the envs [0, nb) of init_rows, columns [0, NA * nb) = [0, 2 NP) (ODD: the last pair holds one real column).
template <int NA, int NP, bool ODD>
__device__ __forceinline__ void spread_gru_batch(const TanhEntry *tanh_tab, SpreadGruLds<6 * NA> &lds, const GruLockstep<6 * NA, 5> &net,
                                                 int lane, int nb, const float *__restrict__ init_rows, int max_cycles,
                                                 double *__restrict__ ret_out, bool valid_row)
{
    constexpr int S = 6 * NA, A = 5, COLS = GL_EB / NA * NA;
    const int slot = lane & 7;
    const int col = slot < COLS ? slot : 0;                 // three agents: slots 6 and 7 replay column 0
    const int e = col / NA, agent = col - e * NA;
    const bool env_valid = e < nb;                          // padding envs replay env 0 (their columns are never read)
    const float *s0 = init_rows + (size_t)(env_valid ? e : 0) * (4 * NA);
    SpreadState<NA> st;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        st.ax[i] = s0[2 * i]; st.ay[i] = s0[2 * i + 1];
        st.vx[i] = 0.0f; st.vy[i] = 0.0f;
        st.lx[i] = s0[2 * NA + 2 * i]; st.ly[i] = s0[2 * NA + 2 * i + 1];
    }
    float hreg[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) hreg[p] = 0.0f;            // every agent's GymEnvModel.reset()
    wave_lds_sync();
    if (lane < 32) {
#pragma unroll
        for (int c = 0; c < GL_EB; ++c) lds.ah[c][lane][1] = 0.0f;
    }
    const int env_lane = (lane & ~7) + e * NA;              // the lane of my 8-lane group that holds my env's agent 0
    double ret = 0.0;
    for (int t = 0; t < max_cycles; ++t) {
        // my agent's observation: the NA candidates have compile-time agent indices (the state stays in registers)
        float obs[S];
        spread_obs<NA>(st, 0, obs);
        if constexpr (NA > 1) {
            float o[S];
            spread_obs<NA>(st, 1, o);
#pragma unroll
            for (int k = 0; k < S; ++k) obs[k] = agent == 1 ? o[k] : obs[k];
        }
        if constexpr (NA > 2) {
            float o[S];
            spread_obs<NA>(st, 2, o);
#pragma unroll
            for (int k = 0; k < S; ++k) obs[k] = agent == 2 ? o[k] : obs[k];
        }
        if (lane < GL_EB) {
#pragma unroll
            for (int k = 0; k < S; ++k) lds.obs[lane][k] = obs[k];
        }
        wave_lds_sync();
        net.template step<NP, ODD>(tanh_tab, lds, hreg, lane);
        float logits[A];
        net.logits_of(lds, lane, logits);
        const int mine = argmax_first<A>(logits);
        int action[NA];
#pragma unroll
        for (int i = 0; i < NA; ++i) action[i] = __shfl(mine, env_lane + i);
        ret += (double)spread_step<NA>(st, action);
    }
    if (valid_row && lane < COLS && env_valid && agent == 0) ret_out[e] = ret;
}

// Four waves per workgroup (they share one copy of the tanh table and never synchronise).  wave_per_batch = 0: a wave plays
// the batches of its offspring one after the other (weights loaded once); 1: one wave per (offspring, batch) -- the weights
// are read once per batch (from L2 after the first), the rollout ends in one batch's time.  Same bits either way.
template <int NA>
__global__ __launch_bounds__(256, 2) void k_rollout_spread_gru(const float *__restrict__ theta, const float *__restrict__ init,
                                                               int init_per_offspring, int n_rows, int E, int P, int max_cycles,
                                                               int wave_per_batch, double *__restrict__ ep_return)
{
    constexpr int S = 6 * NA, EPB = GL_EB / NA, WAVES = 4;
    static_assert(NA == 2 || NA == 3, "a batch is 4 envs of two agents or 2 envs of three");
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ __attribute__((aligned(16))) SpreadGruLds<S> ldsv[WAVES];
    stage_tanh_table(tanh_tab);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int batches = (E + EPB - 1) / EPB;
    const int n_units = wave_per_batch ? n_rows * batches : n_rows;
    int unit = blockIdx.x * WAVES + wave;
    const bool valid = unit < n_units;
    unit = valid ? unit : n_units - 1;
    const int row = wave_per_batch ? unit / batches : unit;
    const int b_first = wave_per_batch ? unit - row * batches : 0;
    const int b_end = wave_per_batch ? b_first + 1 : batches;
    SpreadGruLds<S> &lds = ldsv[wave];
    GruLockstep<S, 5> net;
    net.load(theta + (size_t)row * P, lane, lds);
    wave_lds_sync();
    for (int b = b_first; b < b_end; ++b) {
        const int e0 = b * EPB;
        const int nb = E - e0 < EPB ? E - e0 : EPB;
        const float *rows = init + ((size_t)(init_per_offspring ? row : 0) * E + e0) * (4 * NA);
        double *ro = ep_return + (size_t)row * E + e0;
#define SES_SG_CASE(NP_, ODD_) spread_gru_batch<NA, NP_, ODD_>(tanh_tab, lds, net, lane, nb, rows, max_cycles, ro, valid)
        if constexpr (NA == 2) {
            switch (nb) {
                case 1: SES_SG_CASE(1, false); break;
                case 2: SES_SG_CASE(2, false); break;
                case 3: SES_SG_CASE(3, false); break;
                default: SES_SG_CASE(4, false); break;
            }
        } else {
            if (nb == 1) SES_SG_CASE(2, true);              // three columns: the odd case
            else SES_SG_CASE(3, false);
        }
#undef SES_SG_CASE
    }
}

// (offspring x batch) waves up to which the default runs one wave per (offspring, batch).  Measured crossover at 5 episodes
// (profiles/spread_gru_timing.txt): that form wins at 2048 (two agents) and 3072 (three) waves, loses at 4096 and 6144 -- the
// device holds 2048 of these waves at a time (1024 SIMDs x 2), beyond ~1.5 rounds the repeated weight load costs more than
// the shorter tail saves.
constexpr long long SPREAD_GRU_WAVE_PER_BATCH_MAX = 3072;

int spread_gru_rollout(const ses_handle *h, const RolloutArgs &a)
{
    const int NA = h->cfg.n_agents;
    const int batches = ceil_div(a.E, GL_EB / NA);
    int wpb = h->tune.spread_gru_wave_per_batch;
    if (wpb < 0) wpb = batches > 1 && (long long)a.n_rows * batches <= SPREAD_GRU_WAVE_PER_BATCH_MAX;
    const dim3 grid(ceil_div(wpb ? (long long)a.n_rows * batches : a.n_rows, 4)), block(256);
    with_lanes<2, 3>(NA == 2 ? 2 : 3, [&](auto agents) {
        hipLaunchKernelGGL(k_rollout_spread_gru<agents()>, grid, block, 0, h->stream, a.theta, a.init, a.per, a.n_rows, a.E, a.P,
                           a.max_step, wpb, a.epr);
    });
    return SES_OK;
}

// ses_policy_forward, GRU policy, for the two simple_spread shapes; the caller has checked that (num_state, num_action) is one
int spread_gru_policy_forward(ses_handle *h, const float *theta, const float *obs, float *hidden, int n, float *logits, float *act,
                              int32_t *action)
{
    with_policy_shape<PolicyShape<12, 5>, PolicyShape<18, 5>>(h->cfg.num_state, h->cfg.num_action, [&](auto sh) {
        hipLaunchKernelGGL((k_policy_forward_gru<sh.S, sh.A>), dim3(ceil_div(n, 4)), dim3(256), 0, h->stream, theta, obs, hidden, n,
                           h->P, logits, act, action);
    });
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

}  // namespace ses
