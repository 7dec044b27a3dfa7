// ses_waterworld.hip -- waterworld (csrc/ses_waterworld.h) on the device, through every path the other envs have:
//   k_envs_reset_waterworld / k_envs_step_waterworld : env.reset() / env.step(a) for n independent envs, one lane per env
//                                                      (ses_env_reset / ses_env_step_generic); action float32[n, 5, 2] already
//                                                      scaled, obs [n, 5, 242], the reward rounded to float, done always 0
//   k_rollout_waterworld_mlp<MFMA>                   : RolloutWorker (loop.py:108-125) for one offspring's episodes x 5 pursuers
//                                                      with the MLP policy 242 -> 32 -> 2, the whole episode loop in the kernel
//   k_policy_forward_waterworld                      : ses_policy_forward for (num_state, num_action) = (242, 2)
// A unit of its own: the kernels of the other units keep their machine code byte for byte.
//
// The fused rollout.  One wave plays one TILE of one offspring: up to WW_TILE_E = 6 episodes, i.e. up to 30 (episode, pursuer)
// rows of 242 observations that all meet the offspring's one 242 x 32 fc1 matrix.  fc1 is that product on
// v_mfma_f32_32x32x2_f32: rows = (episode, pursuer), columns = the 32 hidden units, C = b1 in every row, then the 121 k-blocks
// in ascending order -- an MFMA adds its two products one after the other with one rounding each, so the run IS the canonical
// bias-first k-ascending fmaf chain (ses_gru_mfma.h, tools/mfma_exact.hip) and the result equals the oracle's policy_forward
// bit for bit.  The W1 fragments (B operand: lane l holds W1[l & 31][2 kb + (l >> 5)]) stay in 121 VGPRs for the whole rollout.
// Observations live in a wave-private LDS block k-major ([k][row], 32 rows): the A fragment of k-block kb is the 64
// consecutive floats from 64 kb, one conflict-free ds_read_b32.  The VALU form (MFMA = false; "waterworld_fc1_mfma" = 0) keeps
// all 242 weights of the lane's unit in VGPRs and runs the same chain with v_fma_f32 for the 16 rows the MFMA form would
// leave in that lane: identical bits, for A/B timing (tools/time_waterworld.py).
// tanh, fc2 (lane = (row, output): the canonical fc2_row -- groups of 4, balanced tree, bias last), the head (tanh, times
// 0.001f) and the env run on the VALU.  The env's cycle is spread over the lanes where the definition allows: every object's
// move, every pursuer's touches, then one lane per env for catches, rewards and respawns; the sensor work -- (row, sensor)
// items over the objects in the pursuer's reach, the bulk of a step -- over all 64 lanes, item = sensor * rows + row so that
// the lanes of one store hit different LDS banks.  Episodes never end early: no alive logic, every episode is min(max_step, 500) cycles.
#include "ses_gru.h"
#include "ses_env_table.h"
#include "ses_policy.h"
#include "ses_waterworld.h"

namespace ses {

constexpr int WW_TILE_E = 6;                  // episodes per wave: 30 of the tile's 32 rows
constexpr int WW_ROWS = 32;
constexpr int WW_KB = WW_OBS / 2;             // 121 k-blocks of 2
constexpr int WW_P = H * WW_OBS + H + 2 * H + 2;
static_assert(WW_OBS % 2 == 0 && WW_TILE_E * WW_NP <= WW_ROWS, "the tile holds whole episodes and K is a whole number of k-blocks");

typedef float ww_f32x16 __attribute__((ext_vector_type(16)));

// all 242 observations of pursuer a of one env, for the one-lane-per-env kernels
__device__ __forceinline__ void ww_store_obs(const WaterState &s, float *__restrict__ dst)
{
    for (int a = 0; a < WW_NP; ++a) {
        float *o = dst + (size_t)a * WW_OBS;
        const uint32_t cand = ww_candidates(s, a);
        for (int k = 0; k < WW_SENSORS; ++k) {
            float f[8];
            ww_sensor(s, a, k, cand, f);
            for (int q = 0; q < 8; ++q) o[8 * k + q] = f[q];
        }
        o[8 * WW_SENSORS] = s.touch_ev[a] ? 1.0f : 0.0f;
        o[8 * WW_SENSORS + 1] = s.touch_po[a] ? 1.0f : 0.0f;
    }
}

__global__ __launch_bounds__(64) void k_envs_reset_waterworld(const float *__restrict__ init, int n, WaterState *__restrict__ state,
                                                              float *__restrict__ obs)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    WaterState s;
    ww_reset(s, init + (size_t)i * WW_INIT_W);
    state[i] = s;
    ww_store_obs(s, obs + (size_t)i * WW_NP * WW_OBS);
}

__global__ __launch_bounds__(64) void k_envs_step_waterworld(WaterState *__restrict__ state, const float *__restrict__ action, int n,
                                                             float *__restrict__ obs, float *__restrict__ reward,
                                                             int32_t *__restrict__ done)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    WaterState s = state[i];
    float act[WW_NP][2];
    for (int a = 0; a < WW_NP; ++a) {
        act[a][0] = action[((size_t)i * WW_NP + a) * 2];
        act[a][1] = action[((size_t)i * WW_NP + a) * 2 + 1];
    }
    const double r = ww_step(s, act);
    state[i] = s;
    ww_store_obs(s, obs + (size_t)i * WW_NP * WW_OBS);
    reward[i] = (float)r;
    done[i] = 0;
}

// ---- the fused rollout -----------------------------------------------------------------------------------------------------
struct alignas(16) WaterLds {
    float obsT[WW_OBS][WW_ROWS];      // observations, [component][row]; rows past the tile's last stay zero
    float act[WW_ROWS][H + 1];        // tanh(fc1), [row][unit]; the pad keeps a row's 32 reads and a unit's stores off one bank
    float action[WW_ROWS][2];         // the scaled actions
    double thrust[WW_ROWS];           // per row: the thrust term of the cycle, whom the pursuer touches, whom its sensors may see
    uint32_t ev[WW_ROWS], po[WW_ROWS], cand[WW_ROWS];
    WaterState st[WW_TILE_E];
};

// writes the tile's observations: the candidates and the two touch flags of every row, then item = sensor * rows + row over
// the wave's lanes
__device__ __forceinline__ void ww_observe_tile(WaterLds &lds, int lane, int n_rows)
{
    if (lane < n_rows) lds.cand[lane] = ww_candidates(lds.st[lane / WW_NP], lane % WW_NP);
    wave_lds_sync();
    for (int item = lane; item < n_rows * WW_SENSORS; item += 64) {
        const int k = item / n_rows, row = item - k * n_rows;
        const int e = row / WW_NP, a = row - e * WW_NP;
        float f[8];
        ww_sensor(lds.st[e], a, k, lds.cand[row], f);
#pragma unroll
        for (int q = 0; q < 8; ++q) lds.obsT[8 * k + q][row] = f[q];
    }
    if (lane < n_rows) {
        const int e = lane / WW_NP, a = lane - e * WW_NP;
        lds.obsT[8 * WW_SENSORS][lane] = lds.st[e].touch_ev[a] ? 1.0f : 0.0f;
        lds.obsT[8 * WW_SENSORS + 1][lane] = lds.st[e].touch_po[a] ? 1.0f : 0.0f;
    }
}

template <bool MFMA>
__global__ __launch_bounds__(64) void k_rollout_waterworld_mlp(const float *__restrict__ theta, const float *__restrict__ init,
                                                               int init_per_offspring, int n_rows, int E, int P, int max_step,
                                                               int tiles, double *__restrict__ ep_return,
                                                               int32_t *__restrict__ ep_steps)
{
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ WaterLds lds;
    stage_tanh_table(tanh_tab);
    const int lane = threadIdx.x;
    const int row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
    const int e0 = tile * WW_TILE_E;
    const int n_ep = E - e0 < WW_TILE_E ? E - e0 : WW_TILE_E;
    const int n_pairs = n_ep * WW_NP;
    const int horizon = max_step < WW_MAX_CYCLES ? max_step : WW_MAX_CYCLES;
    const float *th = theta + (size_t)row * P;
    const int unit = lane & 31, half = lane >> 5;

    // the policy: fc1 weights of this lane's unit (a k-block's half in the MFMA form, all of them in the VALU form) ...
    constexpr int NW1 = MFMA ? WW_KB : WW_OBS;
    float w1[NW1];
#pragma unroll
    for (int i = 0; i < NW1; ++i) w1[i] = MFMA ? th[unit * WW_OBS + 2 * i + half] : th[unit * WW_OBS + i];
    const float b1 = th[H * WW_OBS + unit];
    // ... and row lane >> 1's output lane & 1 of fc2
    const int frow = lane >> 1, fout = lane & 1;
    float w2[H];
#pragma unroll
    for (int j = 0; j < H; ++j) w2[j] = th[H * WW_OBS + H + fout * H + j];
    const float b2 = th[H * WW_OBS + H + 2 * H + fout];

    for (int i = lane; i < WW_OBS * WW_ROWS; i += 64) (&lds.obsT[0][0])[i] = 0.0f;
    if (lane < n_ep) ww_reset(lds.st[lane], init + ((size_t)(init_per_offspring ? row : 0) * E + e0 + lane) * WW_INIT_W);
    wave_lds_sync();
    ww_observe_tile(lds, lane, n_pairs);
    wave_lds_sync();

    double ret = 0.0;
    for (int t = 0; t < horizon; ++t) {
        // ---- fc1: acc[r] = the pre-activation of (row (r & 3) + 8 (r >> 2) + 4 half, this lane's unit)
        ww_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = b1;
        if constexpr (MFMA) {
            const float *frag = &lds.obsT[0][0] + lane;
#pragma unroll
            for (int kb = 0; kb < WW_KB; ++kb) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(frag[64 * kb], w1[kb], acc, 0, 0, 0);
        } else {
#pragma unroll
            for (int k = 0; k < WW_OBS; ++k) {
                const float4 *o = reinterpret_cast<const float4 *>(&lds.obsT[k][4 * half]);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const float4 x = o[2 * g];                                   // rows 8 g + 4 half .. + 3
                    acc[4 * g] = fma_(w1[k], x.x, acc[4 * g]);
                    acc[4 * g + 1] = fma_(w1[k], x.y, acc[4 * g + 1]);
                    acc[4 * g + 2] = fma_(w1[k], x.z, acc[4 * g + 2]);
                    acc[4 * g + 3] = fma_(w1[k], x.w, acc[4 * g + 3]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) lds.act[(r & 3) + 8 * (r >> 2) + 4 * half][unit] = tanh_(tanh_tab, acc[r]);
        wave_lds_sync();
        // ---- fc2 and the head
        {
            float p[8];
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const float *a = &lds.act[frow][4 * g];
                float q = w2[4 * g] * a[0];
                q = fma_(w2[4 * g + 1], a[1], q);
                q = fma_(w2[4 * g + 2], a[2], q);
                q = fma_(w2[4 * g + 3], a[3], q);
                p[g] = q;
            }
            const float logit = (((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))) + b2;
            lds.action[frow][fout] = tanh_(tanh_tab, logit) * WW_ACTION_SCALE;
        }
        wave_lds_sync();
        // ---- the envs' cycle: every object's move on a lane of its own, every pursuer's touches likewise, then one lane per env
        for (int item = lane; item < n_ep * WW_NOBJ; item += 64) {
            const int e = item / WW_NOBJ, i = item - e * WW_NOBJ;
            if (i < WW_NP) lds.thrust[e * WW_NP + i] = ww_move_pursuer(lds.st[e], i, lds.action[e * WW_NP + i][0], lds.action[e * WW_NP + i][1]);
            else ww_move_drifter(lds.st[e], i);
        }
        wave_lds_sync();
        if (lane < n_pairs) ww_touches(lds.st[lane / WW_NP], lane % WW_NP, lds.ev[lane], lds.po[lane]);
        wave_lds_sync();
        if (lane < n_ep) {
            double thrust[WW_NP];
            uint32_t ev[WW_NP], po[WW_NP];
#pragma unroll
            for (int a = 0; a < WW_NP; ++a) {
                thrust[a] = lds.thrust[lane * WW_NP + a];
                ev[a] = lds.ev[lane * WW_NP + a];
                po[a] = lds.po[lane * WW_NP + a];
            }
            ret += ww_settle(lds.st[lane], thrust, ev, po);
        }
        wave_lds_sync();
        ww_observe_tile(lds, lane, n_pairs);
        wave_lds_sync();
    }
    if (lane < n_ep) {
        ep_return[(size_t)row * E + e0 + lane] = ret;
        if (ep_steps) ep_steps[(size_t)row * E + e0 + lane] = horizon;
    }
}

// ---- ses_policy_forward for (242, 2): one wave per (row, obs) pair, lane & 31 = the hidden unit ---------------------------------
__global__ __launch_bounds__(64) void k_policy_forward_waterworld(const float *__restrict__ theta, const float *__restrict__ obs_in,
                                                                  int n, int P, float *__restrict__ logits_out,
                                                                  float *__restrict__ act_out, int32_t *__restrict__ action_out)
{
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ float hid[H];
    stage_tanh_table(tanh_tab);
    const int i = blockIdx.x, lane = threadIdx.x, unit = lane & 31;
    const float *th = theta + (size_t)i * P;
    const float *obs = obs_in + (size_t)i * WW_OBS;
    float acc = th[H * WW_OBS + unit];
    for (int k = 0; k < WW_OBS; ++k) acc = fma_(th[unit * WW_OBS + k], obs[k], acc);
    if (lane < H) hid[lane] = tanh_(tanh_tab, acc);
    __syncthreads();
    if (lane < 2) {
        const float *w2 = th + H * WW_OBS + H + lane * H;
        float p[8];
        for (int g = 0; g < 8; ++g) {
            float q = w2[4 * g] * hid[4 * g];
            q = fma_(w2[4 * g + 1], hid[4 * g + 1], q);
            q = fma_(w2[4 * g + 2], hid[4 * g + 2], q);
            q = fma_(w2[4 * g + 3], hid[4 * g + 3], q);
            p[g] = q;
        }
        const float logit = (((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))) + th[H * WW_OBS + H + 2 * H + lane];
        logits_out[(size_t)i * 2 + lane] = logit;
        if (act_out) act_out[(size_t)i * 2 + lane] = tanh_(tanh_tab, logit);
        const float other = __shfl(logit, 1);
        if (lane == 0) action_out[i] = other > logit ? 1 : 0;              // argmax, first maximum wins
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
int waterworld_env_state_bytes(const ses_config *) { return (int)sizeof(WaterState); }

int waterworld_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs)
{
    hipLaunchKernelGGL(k_envs_reset_waterworld, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, init, n, (WaterState *)state, obs);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int waterworld_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done)
{
    hipLaunchKernelGGL(k_envs_step_waterworld, dim3(ceil_div(n, 64)), dim3(64), 0, h->stream, (WaterState *)state, (const float *)action, n,
                       obs, reward, done);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

// "waterworld_fc1_mfma": -1 (default) = the faster form as measured (profiles/waterworld_timing.txt), 0 = VALU, 1 = MFMA
int waterworld_rollout(ses_handle *h, const RolloutArgs &a, const RolloutPlan &, int mode)
{
    SES_REQUIRE(mode == SES_MODE_EPISODIC, "ses_rollout: waterworld has no fixed-length mode");
    SES_REQUIRE(a.P == WW_P, "ses_rollout: waterworld runs the MLP policy 242 -> 32 -> 2 (%d parameters)", WW_P);
    const int tiles = ceil_div(a.E, WW_TILE_E);
    const bool mfma = h->tune.waterworld_fc1_mfma != 0;
    const auto kernel = mfma ? k_rollout_waterworld_mlp<true> : k_rollout_waterworld_mlp<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((long long)a.n_rows * tiles)), dim3(64), 0, h->stream, a.theta, a.init, a.per, a.n_rows,
                       a.E, a.P, a.max_step, tiles, a.epr, a.ep_steps);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

int waterworld_policy_forward(ses_handle *h, const float *theta, const float *obs, int n, float *logits, float *act, int32_t *action)
{
    hipLaunchKernelGGL(k_policy_forward_waterworld, dim3(n), dim3(64), 0, h->stream, theta, obs, n, h->P, logits, act, action);
    SES_HIP_TRY(hipGetLastError());
    return SES_OK;
}

}  // namespace ses
