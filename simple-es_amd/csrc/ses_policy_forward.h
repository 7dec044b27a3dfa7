// ses_policy_forward.h -- the standalone population-batched GymEnvModel.forward kernels (neural_network.py:20-36) behind
// ses_policy_forward: ses_rollout.hip instantiates the CartPole / Box2D / simple_spread shapes, ses_f64_envs.hip those
// of the float64 control envs (a unit of its own, so that the other units keep their machine code).
#pragma once
#include <hip/hip_runtime.h>

#include "ses_gru.h"
#include "ses_policy.h"

namespace ses {

// Standalone MLP forward, 4 lanes per (row, obs) pair.
template <int S, int A>
__global__ __launch_bounds__(64) void k_policy_forward_mlp(const float *__restrict__ theta,
                                                           const float *__restrict__ obs_in, int n, int P,
                                                           float *__restrict__ logits_out, float *__restrict__ act_out,
                                                           int32_t *__restrict__ action_out)
{
    constexpr int LPE = 4;
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    stage_tanh_table(tanh_tab);
    const long long gtid = (long long)blockIdx.x * 64 + threadIdx.x;
    int i = (int)(gtid / LPE);
    const int sub = (int)(threadIdx.x % LPE);
    const bool valid = i < n;
    i = valid ? i : n - 1;
    MlpSlice<S, A, LPE> net;
    net.load(theta + (size_t)i * P, sub);
    float obs[S];
#pragma unroll
    for (int k = 0; k < S; ++k) obs[k] = obs_in[(size_t)i * S + k];
    float logits[A];
    net.forward(tanh_tab, obs, logits);
    const int action = argmax_first<A>(logits);
    if (valid && sub == 0) {
#pragma unroll
        for (int k = 0; k < A; ++k) {
            logits_out[(size_t)i * A + k] = logits[k];
            if (act_out) act_out[(size_t)i * A + k] = tanh_(tanh_tab, logits[k]);
        }
        action_out[i] = action;
    }
}

// Standalone GRU forward: one (row, obs, hidden) triple per wavefront.
template <int S, int A>
__global__ __launch_bounds__(256) void k_policy_forward_gru(const float *__restrict__ theta,
                                                            const float *__restrict__ obs_in,
                                                            float *__restrict__ hidden, int n, int P,
                                                            float *__restrict__ logits_out, float *__restrict__ act_out,
                                                            int32_t *__restrict__ action_out)
{
    __shared__ TanhEntry tanh_tab[SES_TANH_N];
    __shared__ __attribute__((aligned(16))) float vecs[4][64];
    stage_tanh_table(tanh_tab);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int i = blockIdx.x * 4 + wave;
    const bool valid = i < n;
    i = valid ? i : n - 1;
    GruSlice<S, A> net;
    net.load(theta + (size_t)i * P, lane);
    float *vec = vecs[wave];
    float obs[S];
#pragma unroll
    for (int k = 0; k < S; ++k) obs[k] = obs_in[(size_t)i * S + k];
    float h = hidden[(size_t)i * H + (lane & 31)];
    if (lane < 32) vec[2 * lane + 1] = h;
    wave_lds_sync();
    float logits[A];
    net.forward(tanh_tab, obs, h, vec, lane, logits);
    const int action = argmax_first<A>(logits);
    if (valid && lane < 32) hidden[(size_t)i * H + lane] = h;
    if (valid && lane == 0) {
#pragma unroll
        for (int k = 0; k < A; ++k) {
            logits_out[(size_t)i * A + k] = logits[k];
            if (act_out) act_out[(size_t)i * A + k] = tanh_(tanh_tab, logits[k]);
        }
        action_out[i] = action;
    }
}

}  // namespace ses
