// ses_pursuit.hip -- pursuit (csrc/ses_pursuit.h) on the device, through every path the other envs have:
//   k_envs_reset_pursuit / k_envs_step_pursuit : env.reset() / env.step(a) for n independent envs, one lane per env
//                                                (ses_env_reset / ses_env_step_generic); action int32[n, 8], obs [n, 8, 147],
//                                                the team reward rounded to float, done = no evader is left
//   k_rollout_pursuit_mlp<MFMA>                : RolloutWorker (loop.py:108-125) for one offspring's episodes x 8 pursuers
//                                                with the MLP policy 147 -> 32 -> 5, the whole episode loop in the kernel
//   k_policy_forward_pursuit                   : ses_policy_forward for (num_state, num_action) = (147, 5)
// A unit of its own: the kernels of the other units keep their machine code byte for byte.
//
// The fused rollout, modelled on k_rollout_waterworld_mlp.  One wave plays one TILE of one offspring: up to PU_TILE_E = 4
// episodes, i.e. up to 32 (episode, pursuer) rows of 147 observations that all meet the offspring's one 147 x 32 fc1 matrix --
// a full tile fills the 32 rows of v_mfma_f32_32x32x2_f32 exactly.  eval_ep_num that is no multiple of 4 leaves the
// offspring's LAST tile partial: its rows past 8 * (episodes left) stay zero observations whose results nobody reads.
// fc1: rows = (episode, pursuer), columns = the 32 hidden units, C = b1 in every row, then the k-blocks in ascending order -- an
// MFMA adds its two products one after the other with one rounding each, so the run IS the canonical bias-first k-ascending
// fmaf chain (ses_gru_mfma.h, tools/mfma_exact.hip).  K = 147 is padded to 148 = 74 k-blocks.  THE PAD: observation row 147
// is +0 and the pad weight is -0, so the pad's product is -0, and x + (-0) = x for EVERY x under round to nearest -- a -0
// accumulator (b1 = -0, all products -0) stays -0, where a +0 pad product would have made it +0.  The pad is the last term, so it
// meets the finished chain and changes no bit of it.  The W1 fragments (B operand: lane l holds W1[l & 31][2 kb + (l >> 5)])
// stay in 74 VGPRs for the whole rollout.  Observations live in a wave-private LDS block k-major ([k][row], 32 rows) as BYTES --
// they are counts 0 .. 30 and flags, so the conversion to float at the read is exact, and the block is 4.7 KB instead of 18.9:
// the kernel's LDS drops to 18 KB, which lets eight waves share a CU where the float block allowed four.  The A fragment of
// k-block kb is the 64 consecutive bytes from 64 kb (ds_read_u8 + v_cvt_f32_ubyte0).  The VALU form (MFMA = false;
// "pursuit_fc1_mfma" = 0) keeps all 147 weights of the lane's unit in VGPRs and runs the same chain with v_fma_f32 for the 16
// rows the MFMA form would leave in that lane, with no pad: identical bits, for A/B timing (tools/time_pursuit.py).
// tanh, fc2 (lane = (row, outputs of one parity): the canonical groups of 4, balanced tree, bias last; W2 read from LDS, one
// address per half-wave) and the first-maximum argmax run on the VALU.  The env's cycle is spread over the lanes where the
// definition allows: lanes 0 .. 31 move the pursuers while lanes 32 .. 63 draw and move the evaders, a quad each; every (episode,
// evader) decides its catch on a lane of its own; every (episode, pursuer) row counts its reward; one lane per env adds the
// eight in order, removes the caught and decides done; the occupancy grids and the 7 x 7 x 3 windows are again spread over
// all lanes.  An episode that ends (no evader left) is frozen -- its state, return and step count stand still, its rows keep
// riding through fc1 unread -- while its tile-mates run on; the wave leaves the loop when all its episodes are done.
#include "ses_gru.h"
#include "ses_env_table.h"
#include "ses_policy.h"
#include "ses_pursuit.h"

namespace ses {

constexpr int PU_TILE_E = 4;                  // episodes per wave: all 32 rows of the tile
constexpr int PU_ROWS = 32;
constexpr int PU_KPAD = PU_OBS + 1;           // 148
constexpr int PU_KB = PU_KPAD / 2;            // 74 k-blocks of 2
constexpr int PU_A = 5;
constexpr int PU_P = H * PU_OBS + H + PU_A * H + PU_A;
static_assert(PU_KPAD % 2 == 0 && PU_TILE_E * PU_NP == PU_ROWS, "the tile holds whole episodes and K is a whole number of k-blocks");

typedef float pu_f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(64) void k_envs_reset_pursuit(const float *__restrict__ init, int n, PursuitState *__restrict__ state,
                                                           float *__restrict__ obs)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    PursuitState s;
    pu_reset(s, init + (size_t)i * PU_INIT_W);
    state[i] = s;
    for (int a = 0; a < PU_NP; ++a) pu_observe(s, a, obs + ((size_t)i * PU_NP + a) * PU_OBS);
}

__global__ __launch_bounds__(64) void k_envs_step_pursuit(PursuitState *__restrict__ state, const int32_t *__restrict__ action, int n,
                                                          float *__restrict__ obs, float *__restrict__ reward, int32_t *__restrict__ done)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    PursuitState s = state[i];
    int32_t act[PU_NP];
    for (int a = 0; a < PU_NP; ++a) act[a] = action[(size_t)i * PU_NP + a];
    bool d;
    const double r = pu_step(s, act, d);
    state[i] = s;
    for (int a = 0; a < PU_NP; ++a) pu_observe(s, a, obs + ((size_t)i * PU_NP + a) * PU_OBS);
    reward[i] = (float)r;
    done[i] = d ? 1 : 0;
}

// ---- the fused rollout -----------------------------------------------------------------------------------------------------
struct alignas(16) PursuitLds {
    uint8_t obsT[PU_KPAD][PU_ROWS];   // observations, [component][row], ONE BYTE each (they are counts 0 .. 30 and flags: the
                                      // conversion to float at the read is exact); rows past the tile's last and component 147 stay 0
    float act[PU_ROWS][H + 1];        // tanh(fc1), [row][unit]; the pad keeps a row's 32 reads and a unit's stores off one bank
    float w2[PU_A][H];                // fc2 of the offspring
    float b2[8];
    float logit[PU_ROWS][PU_A];
    double r[PU_ROWS];                // per row: the pursuer's own reward of the cycle
    uint32_t pc[PU_TILE_E][PU_GRID * PU_GRID / 4];   // pursuers per cell, one byte a cell (x * 16 + y)
    uint32_t ec[PU_TILE_E][PU_GRID * PU_GRID / 4];   // live evaders per cell
    uint32_t caught[PU_TILE_E];       // the evaders caught in this cycle
    int32_t done[PU_TILE_E];
    PursuitState st[PU_TILE_E];
};

// counts the actors of the live episodes into the grids (lanes 0 .. 31: the row's pursuer, lanes 32 .. 63: a quad of evaders) and
// writes the rows' windows.  The grids of a finished episode are left alone, and so are its observations.
__device__ __forceinline__ void pu_observe_tile(PursuitLds &lds, int lane, int n_ep)
{
    const int ep = (lane & 31) >> 3;
    const bool live = ep < n_ep && !lds.done[ep];
    if (live) {
        for (int i = lane & 7; i < PU_GRID * PU_GRID / 4; i += 8) (lane < 32 ? lds.pc : lds.ec)[ep][i] = 0u;
    }
    wave_lds_sync();
    if (live) {
        const PursuitState &s = lds.st[ep];
        if (lane < 32) {
            const int c = (int)s.px[lane & 7] * PU_GRID + (int)s.py[lane & 7];
            atomicAdd(&lds.pc[ep][c >> 2], 1u << (8 * (c & 3)));
        } else {
            const int q = lane & 7;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = 4 * q + j;
                if (e < PU_NE && ((s.alive >> e) & 1u)) {
                    const int c = (int)s.ex[e] * PU_GRID + (int)s.ey[e];
                    atomicAdd(&lds.ec[ep][c >> 2], 1u << (8 * (c & 3)));
                }
            }
        }
    }
    wave_lds_sync();
    if (live) {
        const int row = lane & 31;
        const int x = lds.st[ep].px[row & 7], y = lds.st[ep].py[row & 7];
        const uint8_t *pc = reinterpret_cast<const uint8_t *>(lds.pc[ep]);
        const uint8_t *ec = reinterpret_cast<const uint8_t *>(lds.ec[ep]);
        for (int c = lane >> 5; c < PU_RANGE * PU_RANGE; c += 2) {
            int cx, cy;
            const bool wall = pu_window_cell(x, y, c / PU_RANGE, c % PU_RANGE, cx, cy);
            const int cell = pu_on_grid(cx, cy) ? cx * PU_GRID + cy : 0;           // (a cell off the grid reads cell 0 and drops it)
            const uint8_t np = pc[cell], ne = ec[cell];
            lds.obsT[3 * c][row] = wall ? 1 : 0;
            lds.obsT[3 * c + 1][row] = pu_on_grid(cx, cy) ? np : 0;
            lds.obsT[3 * c + 2][row] = pu_on_grid(cx, cy) ? ne : 0;
        }
    }
}

template <bool MFMA>
__global__ __launch_bounds__(64) void k_rollout_pursuit_mlp(const float *__restrict__ theta, const float *__restrict__ init,
                                                            int init_per_offspring, int n_rows, int E, int P, int max_step, int tiles,
                                                            double *__restrict__ ep_return, int32_t *__restrict__ ep_steps)
{
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ PursuitLds lds;
    stage_tanh_table(tanh_tab);
    const int lane = threadIdx.x;
    const int row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    const int e0 = tile * PU_TILE_E;
    const int n_ep = E - e0 < PU_TILE_E ? E - e0 : PU_TILE_E;
    const int horizon = max_step < PU_MAX_CYCLES ? max_step : PU_MAX_CYCLES;
    const float *th = theta + (size_t)row * P;
    const int unit = lane & 31, half = lane >> 5;

    // the policy: fc1 weights of this lane's unit (a k-block's half in the MFMA form -- the pad weight is -0, see the head of the
    // file -- all of them in the VALU form); fc2 goes to LDS
    constexpr int NW1 = MFMA ? PU_KB : PU_OBS;
    float w1[NW1];
#pragma unroll
    for (int i = 0; i < NW1; ++i) {
        if constexpr (MFMA) w1[i] = 2 * i + half < PU_OBS ? th[unit * PU_OBS + 2 * i + half] : -0.0f;
        else w1[i] = th[unit * PU_OBS + i];
    }
    const float b1 = th[H * PU_OBS + unit];
    for (int i = lane; i < PU_A * H; i += 64) (&lds.w2[0][0])[i] = th[H * PU_OBS + H + i];
    if (lane < PU_A) lds.b2[lane] = th[H * PU_OBS + H + PU_A * H + lane];

    for (int i = lane; i < PU_KPAD * PU_ROWS / 4; i += 64) reinterpret_cast<uint32_t *>(&lds.obsT[0][0])[i] = 0u;
    if (lane < PU_TILE_E) lds.done[lane] = lane < n_ep ? 0 : 1;
    if (lane < n_ep) pu_reset(lds.st[lane], init + ((size_t)(init_per_offspring ? row : 0) * E + e0 + lane) * PU_INIT_W);
    wave_lds_sync();
    pu_observe_tile(lds, lane, n_ep);
    wave_lds_sync();

    // lane & 31 is this lane's row in every phase after fc1: episode (lane & 31) >> 3, pursuer lane & 7 (lanes 0 .. 31) or
    // evader quad lane & 7 (lanes 32 .. 63)
    const int frow = lane & 31, fep = frow >> 3, sub = lane & 7;
    double ret = 0.0;
    int steps = 0;
    for (int t = 0; t < horizon; ++t) {
        const bool live = fep < n_ep && !lds.done[fep];
        if (__ballot(live) == 0ull) break;
        // ---- fc1: acc[r] = the pre-activation of (row (r & 3) + 8 (r >> 2) + 4 half, this lane's unit)
        pu_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = b1;
        if constexpr (MFMA) {
            const uint8_t *frag = &lds.obsT[0][0] + lane;
#pragma unroll
            for (int kb = 0; kb < PU_KB; ++kb) acc = __builtin_amdgcn_mfma_f32_32x32x2f32((float)frag[64 * kb], w1[kb], acc, 0, 0, 0);
        } else {
#pragma unroll
            for (int k = 0; k < PU_OBS; ++k) {
                const uint32_t *o = reinterpret_cast<const uint32_t *>(&lds.obsT[k][4 * half]);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const uint32_t x = o[2 * g];                                 // rows 8 g + 4 half .. + 3, a byte each
                    acc[4 * g] = fma_(w1[k], (float)(x & 0xFFu), acc[4 * g]);
                    acc[4 * g + 1] = fma_(w1[k], (float)((x >> 8) & 0xFFu), acc[4 * g + 1]);
                    acc[4 * g + 2] = fma_(w1[k], (float)((x >> 16) & 0xFFu), acc[4 * g + 2]);
                    acc[4 * g + 3] = fma_(w1[k], (float)(x >> 24), acc[4 * g + 3]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) lds.act[(r & 3) + 8 * (r >> 2) + 4 * half][unit] = tanh_(tanh_tab, acc[r]);
        wave_lds_sync();
        // ---- fc2: lanes 0 .. 31 hold outputs 0, 2, 4 of their row, lanes 32 .. 63 outputs 1, 3 (and 4 once more)
        {
            float a[H];
#pragma unroll
            for (int j = 0; j < H; ++j) a[j] = lds.act[frow][j];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int o = half + 2 * q < PU_A ? half + 2 * q : PU_A - 1;
                const float4 *w = reinterpret_cast<const float4 *>(&lds.w2[o][0]);
                float p[8];
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    const float4 wg = w[g];
                    float s = wg.x * a[4 * g];
                    s = fma_(wg.y, a[4 * g + 1], s);
                    s = fma_(wg.z, a[4 * g + 2], s);
                    s = fma_(wg.w, a[4 * g + 3], s);
                    p[g] = s;
                }
                lds.logit[frow][o] = (((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))) + lds.b2[o];
            }
        }
        if (lane < PU_TILE_E) lds.caught[lane] = 0u;
        wave_lds_sync();
        // ---- the envs' cycle.  Moves: no actor's move reads another actor
        if (live) {
            PursuitState &s = lds.st[fep];
            if (lane < 32) {
                float lg[PU_A];
#pragma unroll
                for (int o = 0; o < PU_A; ++o) lg[o] = lds.logit[frow][o];
                pu_move(s.px[sub], s.py[sub], argmax_first<PU_A>(lg));
            } else {
                pu_move_evaders(s, sub);
            }
        }
        wave_lds_sync();
        // catches: (episode, evader) items, on the positions after all moves
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            const int ep = 2 * pass + half, e = lane & 31;
            if (ep < n_ep && !lds.done[ep] && e < PU_NE && ((lds.st[ep].alive >> e) & 1u) && pu_caught(lds.st[ep], e))
                atomicOr(&lds.caught[ep], 1u << e);
        }
        wave_lds_sync();
        if (live && lane < 32) lds.r[frow] = pu_pursuer_reward(lds.st[fep], sub, lds.st[fep].alive, lds.caught[fep]);
        wave_lds_sync();
        if (lane < n_ep && !lds.done[lane]) {
            double r[PU_NP];
#pragma unroll
            for (int i = 0; i < PU_NP; ++i) r[i] = lds.r[lane * PU_NP + i];
            ret += pu_team_reward(r);
            steps = t + 1;
            const bool d = pu_settle(lds.st[lane], lds.caught[lane]);
            if (d) lds.done[lane] = 1;
        }
        wave_lds_sync();
        pu_observe_tile(lds, lane, n_ep);
        wave_lds_sync();
    }
    if (lane < n_ep) {
        ep_return[(size_t)row * E + e0 + lane] = ret;
        if (ep_steps) ep_steps[(size_t)row * E + e0 + lane] = steps;
    }
}

// ---- ses_policy_forward for (147, 5): one wave per (row, obs) pair, lane & 31 = the hidden unit ---------------------------------
__global__ __launch_bounds__(64) void k_policy_forward_pursuit(const float *__restrict__ theta, const float *__restrict__ obs_in, int n,
                                                               int P, float *__restrict__ logits_out, float *__restrict__ act_out,
                                                               int32_t *__restrict__ action_out)
{
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ float hid[H];
    __shared__ float lg[PU_A];
    stage_tanh_table(tanh_tab);
    const int i = blockIdx.x, lane = threadIdx.x, unit = lane & 31;
    const float *th = theta + (size_t)i * P;
    const float *obs = obs_in + (size_t)i * PU_OBS;
    float acc = th[H * PU_OBS + unit];
    for (int k = 0; k < PU_OBS; ++k) acc = fma_(th[unit * PU_OBS + k], obs[k], acc);
    if (lane < H) hid[lane] = tanh_(tanh_tab, acc);
    __syncthreads();
    if (lane < PU_A) {
        const float *w2 = th + H * PU_OBS + H + lane * H;
        float p[8];
        for (int g = 0; g < 8; ++g) {
            float q = w2[4 * g] * hid[4 * g];
            q = fma_(w2[4 * g + 1], hid[4 * g + 1], q);
            q = fma_(w2[4 * g + 2], hid[4 * g + 2], q);
            q = fma_(w2[4 * g + 3], hid[4 * g + 3], q);
            p[g] = q;
        }
        const float logit = (((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))) + th[H * PU_OBS + H + PU_A * H + lane];
        logits_out[(size_t)i * PU_A + lane] = logit;
        if (act_out) act_out[(size_t)i * PU_A + lane] = tanh_(tanh_tab, logit);
        lg[lane] = logit;
    }
    __syncthreads();
    if (lane == 0) {
        float all[PU_A];
        for (int o = 0; o < PU_A; ++o) all[o] = lg[o];
        action_out[i] = argmax_first<PU_A>(all);                              // first maximum wins
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
int pursuit_env_state_bytes(const ses_config *) { return (int)sizeof(PursuitState); }

int pursuit_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs)
{
    hipLaunchKernelGGL(k_envs_reset_pursuit, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, init, n, (PursuitState *)state, obs);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int pursuit_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done)
{
    hipLaunchKernelGGL(k_envs_step_pursuit, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, (PursuitState *)state, (const int32_t *)action, n, obs,
                       reward, done);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

// "pursuit_fc1_mfma": -1 (default) = the faster form as measured (profiles/pursuit_timing.txt), 0 = VALU, 1 = MFMA
int pursuit_rollout(ses_handle *h, const RolloutArgs &a, const RolloutPlan &, int mode)
{
    SES_REQUIRE(mode == SES_MODE_EPISODIC, "ses_rollout: pursuit has no fixed-length mode");
    SES_REQUIRE(a.P == PU_P, "ses_rollout: pursuit runs the MLP policy 147 -> 32 -> 5 (%d parameters)", PU_P);
    const int tiles = ceil_div(a.E, PU_TILE_E);
    const bool mfma = h->tune.pursuit_fc1_mfma != 0;
    const auto kernel = mfma ? k_rollout_pursuit_mlp<true> : k_rollout_pursuit_mlp<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((long long)a.n_rows * tiles)), dim3(64), 0, h->stream, a.theta, a.init, a.per, a.n_rows,
                       a.E, a.P, a.max_step, tiles, a.epr, a.ep_steps);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int pursuit_policy_forward(ses_handle *h, const float *theta, const float *obs, int n, float *logits, float *act, int32_t *action)
{
    hipLaunchKernelGGL(k_policy_forward_pursuit, dim3(n), dim3(64), 0, h->stream, theta, obs, n, h->P, logits, act, action);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

}  // namespace ses
