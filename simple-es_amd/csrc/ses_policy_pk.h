// ses_policy_pk.h -- the CartPole MLP step for a wave that issues at its own cadence: one that has its SIMD to itself
// (round 6), and the heavy wave of the light + heavy pair kernel, which is served first (round 9).
//
// Small per-GPU populations -- the 512 / 1024 offspring per GPU of the strong-scaling line, conf/cartpole.yaml's 97 -- are
// fewer waves than the chip has SIMDs: a rollout then costs max_step x the time ONE wave needs for a step.  A lone wave issues
// one instruction every ~2.2 ns whatever the instruction is (profiles/r01_valu_issue.txt: v_mul_f32 2.2 ns, v_pk_fma_f32 2.5 ns
// at one wave per SIMD; the two slots a packed instruction takes only show when several waves compete), and
// tools/chain_model.py shows the step of the 16-lanes-per-env loop to be bound by exactly that: 83 instructions issued in order
// take 207 ns (measured: 198) against a dependence chain of 144 ns.  So here two IEEE operations per instruction pay: this
// file is the same canonical arithmetic (ses_policy.h, ses_cartpole.h) with
//   fc1      the lane's hidden units in pairs: (unit 2p, unit 2p + 1) advance with ONE v_pk_fma_f32 per input;
//   fc2      the two logits as a pair: one packed product / fma per hidden unit instead of two;
//   sin/cos  the two polynomials' Horner steps as a pair;
//   state    (x, theta) += tau (xd, thetad) and (xd, thetad) += tau (xacc, thetaacc) as pairs.
// Every half of a packed instruction is the IEEE operation the scalar form performs, in the same order: results are
// bit-identical (tests/test_gpu_parity.py, tests/test_gpu_heavy_packed.py and tools/fuzz_parity.py run both forms against the
// oracle and against each other).  The plan (ses_rollout_plan.h: cartpole_mlp_packed) takes this form when the population
// gives every wave a SIMD of its own.  With two or more waves per SIMD that compete as equals the scalar form is faster (round 1
// measured packing at +1.5 ... +9 % there: NOTES.md).  The pair kernel's two waves are not equals: the heavy wave (4 lanes per
// env, 160 VALU instructions per step) runs at s_setprio 1, the light wave fills its stalls and ends early.  16 extra moves per
// step cost 12.8 us per generation in the heavy loop and 4.1 us in the light one (profiles/r09_heavy_stream.txt), so the heavy
// wave pays for its instruction count: packed (132 VALU per step) it measured 0.1894 against 0.1924 ms per generation, -1.5 %,
// ranges apart.  That is a fifth of what the instruction count alone would give: the counters (profiles/r09_sq_rollout.json) show
// the light wave ending at 73 % of the dispatch instead of 85 % and the heavy wave's step at 2.34 ns per instruction where it
// was 2.06 -- it waits on its own dependences (the chain behind the action), which packing does not shorten.  The light wave
// stays scalar.
// Round 10: what such a wave pays most for is not the chain behind the action but its s_waitcnt.  Computing the action-dependent half
// of the physics for BOTH actions in packed halves ahead of the argmax (9 v_pk_* + 2 selects for 10 scalar instructions, the modelled
// stalls down from 20 to 7 ns per step) measured 4 % SLOWER in the heavy wave and 3 % slower in a lone one, and is not in the tree.
// Taking the per-step s_waitcnt vmcnt(0) out of the loop (the fc2 bias is waited for once, in front of it) and evaluating the heavy
// wave's eight table entries in an order that needs three or four waits for seven (finish(), U == 8) measured 0.1889 -> 0.1791 ms per
// generation, -5.2 %, and 94 -> 91 us in the lone wave at 16 lanes per env (NOTES.md "round 10", profiles/r10_action_speculated.txt).
// The clock stamps of round 10 (profiles/r10_wave_stamps.txt) correct the picture above: in every stamped pair the LIGHT wave is the last
// to end (at 1.11 of the heavy wave's run, 1.16 after this change), so the dispatch is paced by what the heavy wave leaves the light one.
// Round 13: the table entry's address without a conversion.  v_cvt_i32_f32 and v_lshlrev_b32 are half-rate; (t - fract t) times the
// subnormal 2^-145 has the bit pattern 16 floor(t), the entry's byte offset, and costs a v_sub_f32 and a v_mul_f32 (tanh_offset_scaled,
// ses_math.h; profiles/r13_valu_issue.txt: a multiply with a subnormal result issues at the full rate).  It pays only in the order
// begin() now states: the compiler, left alone, emits a unit's clamp, fraction, difference and product back to back -- four dependent
// instructions in a row, eight times -- and the headline generation then took 0.1854 ms for the parent's 0.1746; every stage over all
// eight units in turn, with a sched_barrier between the stages: 0.1685 for 0.1752, -3.8 %, ranges apart (profiles/r13_step_trim.txt).
// The same round tried the step without its four clamps (they never act on a live env): 11 VALU instructions fewer per pair and step,
// 3 % SLOWER, alone and on top of the above -- the compiler moves this loop's table reads and waits when the tail of the step changes
// (NOTES.md, round 13).  The clamps stay.
#pragma once
#include "ses_cartpole.h"
#include "ses_policy.h"

namespace ses {

typedef float pk2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ pk2 pk_fma(pk2 a, pk2 b, pk2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ pk2 pk_splat(float v) { return pk2{v, v}; }

// MLP 4 -> 32 -> 2 with the hidden units spread over LPE = 4, 8 or 16 adjacent lanes
template <int LPE>
struct MlpSlicePk {
    static constexpr int S = 4, A = 2;
    static constexpr int U = H / LPE;     // hidden units of this lane: 8, 4 or 2
    static constexpr int UP = U / 2;      // ... in pairs
    static constexpr int G = U / 4;       // whole fc2 groups of this lane: 2, 1 (or none: a lane pair owns one)
    static_assert(U == 2 || U == 4 || U == 8, "4, 8 or 16 lanes per env");
    pk2 w1[UP][S];    // (W1[j0 + 2p][k], W1[j0 + 2p + 1][k]) x 32
    pk2 b1[UP];
    pk2 w2[U];        // (W2[0][j0 + u], W2[1][j0 + u]): the lane's own columns of both outputs
    pk2 w2e[2];       // U == 2: the columns of the pair's EVEN lane (see MlpSlice<.., 16>::finish)
    pk2 b2;

    __device__ __forceinline__ void load(const float *__restrict__ theta, int sub)
    {
        const int j0 = sub * U;
        const float *pw1 = theta, *pb1 = theta + H * S, *pw2 = pb1 + H, *pb2 = pw2 + A * H;
#pragma unroll
        for (int p = 0; p < UP; ++p) {
#pragma unroll
            for (int k = 0; k < S; ++k)
                w1[p][k] = pk2{SES_TANH_H_INV * pw1[(j0 + 2 * p) * S + k], SES_TANH_H_INV * pw1[(j0 + 2 * p + 1) * S + k]};
            b1[p] = pk2{SES_TANH_H_INV * pb1[j0 + 2 * p], SES_TANH_H_INV * pb1[j0 + 2 * p + 1]};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) w2[u] = pk2{pw2[j0 + u], pw2[H + j0 + u]};
#pragma unroll
        for (int u = 0; u < 2; ++u) w2e[u] = pk2{pw2[(j0 & ~3) + u], pw2[H + (j0 & ~3) + u]};
        b2 = pk2{pb2[0], pb2[1]};
    }

    struct Pending {
        float pre[U], frac[U];
        TanhEntry ent[U];
    };

    // the table entries by their byte offsets (tanh_offset_scaled, ses_math.h): no v_cvt_i32_f32 / v_lshlrev_b32 per unit
    __device__ __forceinline__ void begin(const TanhEntry *tab, const float (&obs)[S], Pending &pd) const
    {
        uint32_t off[U];
        float t[U];
        pk2 acc[UP];
#pragma unroll
        for (int p = 0; p < UP; ++p) acc[p] = b1[p];
        // bias first, k ascending: canonical.  The unit pairs advance side by side: a packed instruction that reads the result
        // of the one before it costs an s_nop, which is an issue interval like any other for the wave this form is for
#pragma unroll
        for (int k = 0; k < S; ++k) {
#pragma unroll
            for (int p = 0; p < UP; ++p) acc[p] = pk_fma(w1[p][k], pk_splat(obs[k]), acc[p]);
        }
#pragma unroll
        for (int p = 0; p < UP; ++p) {
            pd.pre[2 * p] = acc[p].x;
            pd.pre[2 * p + 1] = acc[p].y;
            t[2 * p] = tanh_arg_scaled(acc[p].x);
            t[2 * p + 1] = tanh_arg_scaled(acc[p].y);
        }
        // every stage over all units before the next: a unit's clamp, fraction, difference and product depend on each other in turn
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u) pd.frac[u] = tanh_fract(t[u]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u) t[u] = t[u] - pd.frac[u];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u) off[u] = f2u(t[u] * u2f(0x10u));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < U; ++u) pd.ent[u] = *(const TanhEntry *)((const char *)tab + off[u]);
    }

    // (logit 0, logit 1), identical in all lanes of the env
    __device__ __forceinline__ pk2 finish(const Pending &pd) const
    {
        float a[U];
        if constexpr (U == 8) {
            // The table reads return in order and the compiler puts an s_waitcnt in front of each entry's first use: evaluated in
            // the order 0 ... 7 that is seven waits in a row, every one an issue interval (and a pause) of the wave that is served
            // first.  Entry 2 first, then 0 and 1, which have arrived by then; 5, then 3 and 4; then 7 and 6: three or four waits.
            // Measured, not modelled: 0.1889 -> 0.1791 ms per generation with this order, and NO gain or a loss with four others
            // that wait less often or for later entries (profiles/r10_action_speculated.txt).  4 and 2 units per lane: as before.
            // The gain hangs on where THIS compiler (AMD clang 22.0.0git, ROCm 7.2.0) puts its waits and how it schedules the rest of
            // the loop around this order: tools/issue_model.py records the loop's instruction count (148 of every kind at 4 lanes
            // per env), and after a compiler upgrade the order has to be measured again (NOTES.md, round 10).
            constexpr int order[8] = {2, 0, 1, 5, 3, 4, 7, 6};
#pragma unroll
            for (int i = 0; i < 8; ++i) a[order[i]] = tanh_eval(pd.ent[order[i]], pd.frac[order[i]], pd.pre[order[i]]);
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) a[u] = tanh_eval(pd.ent[u], pd.frac[u], pd.pre[u]);
        }
        pk2 q;
        if constexpr (U == 2) {
            // odd lane of a pair: the group's in-order chain, units 4g, 4g + 1 from the even neighbour (two DPP moves: packed
            // instructions take no DPP operand), then its own 4g + 2, 4g + 3
            const float e0 = dpp_mov<DPP_QUAD_00_22>(a[0]), e1 = dpp_mov<DPP_QUAD_00_22>(a[1]);
            q = w2e[0] * pk_splat(e0);
            q = pk_fma(w2e[1], pk_splat(e1), q);
            q = pk_fma(w2[0], pk_splat(a[0]), q);
            q = pk_fma(w2[1], pk_splat(a[1]), q);
            float q0 = q.x, q1 = q.y;
            q0 = q0 + dpp_mov<DPP_QUAD_XOR2>(q0);
            q1 = q1 + dpp_mov<DPP_QUAD_XOR2>(q1);
            q0 = q0 + dpp_mov<DPP_ROW_ROR12>(q0);
            q1 = q1 + dpp_mov<DPP_ROW_ROR12>(q1);
            q0 = q0 + dpp_mov<DPP_ROW_ROR8>(q0);
            q1 = q1 + dpp_mov<DPP_ROW_ROR8>(q1);
            const pk2 lg = pk2{q0, q1} + b2;
            return pk2{dpp_mov<DPP_ROW_BCAST1>(lg.x), dpp_mov<DPP_ROW_BCAST1>(lg.y)};
        } else {
            // G fc2 groups per lane: the chain over the four units of each, the in-lane level of the tree (G == 2: the heavy
            // wave of the pair kernel, as MlpSlice<4, 2, 4>), the tree over the LPE lanes of the env (DPP takes no packed operand)
            pk2 p[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                p[g] = w2[4 * g] * pk_splat(a[4 * g]);
                p[g] = pk_fma(w2[4 * g + 1], pk_splat(a[4 * g + 1]), p[g]);
                p[g] = pk_fma(w2[4 * g + 2], pk_splat(a[4 * g + 2]), p[g]);
                p[g] = pk_fma(w2[4 * g + 3], pk_splat(a[4 * g + 3]), p[g]);
            }
            if constexpr (G == 2) q = p[0] + p[1];
            else q = p[0];
            const float q0 = lanes_sum<LPE>(q.x), q1 = lanes_sum<LPE>(q.y);
            return pk2{q0, q1} + b2;
        }
    }
};

// (x, theta) and (xd, thetad) of one env as pairs
struct CartPoleSimPk {
    pk2 P, V;
    __device__ __forceinline__ void init(const float *s0)
    {
        P = pk2{s0[0], s0[2]};
        V = pk2{s0[1], s0[3]};
    }
};

// The step loop of a wave that issues at its own cadence -- a lone wave, or the heavy wave of the pair kernel at s_setprio 1:
// fp32 dynamics, every lane's pole angle inside |th| <= SINCOS_SMALL_MAX (checked by the caller, wave-uniform).  Same control
// flow as rollout_cartpole_mlp_loop (ses_rollout.hip); one text for 4, 8 and 16 lanes per env.  Fixed length: alive_mask holds the
// wave's live lanes on entry and on exit, and sim the state, so that a run may be made in segments.
template <int LPE, bool FIXED_LENGTH, bool MASKED, class PADS = NoLoopPads>
__device__ __forceinline__ void rollout_cartpole_mlp_loop_pk(const TanhEntry *tanh_tab, const MlpSlicePk<LPE> &net,
                                                             CartPoleSimPk &sim, int max_step, uint32_t obs_mask, int &steps,
                                                             unsigned long long &alive_mask)
{
    pk2 P = sim.P;                                            // (x, theta)
    pk2 V = sim.V;                                            // (xd, thetad)
    const float th_clamp = register_constant(CP_TH_CLAMP), lim_clamp = register_constant(CP_CLAMP);
    const pk2 tau2 = pk_splat(register_constant(CP_TAU));
    // the two polynomials of sincos_small_ side by side: (cos, sin)
    const pk2 k0 = {register_constant(2.443315711809948e-5f), register_constant(-1.9515295891e-4f)};
    const pk2 k1 = {register_constant(-1.388731625493765e-3f), register_constant(8.3321608736e-3f)};
    const pk2 k2 = {register_constant(4.166664568298827e-2f), register_constant(-1.6666654611e-1f)};
    // the fc2 bias is the last of the net a step needs: where it came by a global load, that load ends here and not behind an
    // s_waitcnt vmcnt(0) inside every step.  The statement emits no instruction and is NOT dead code: it is a fence that makes the
    // compiler wait for the load in front of the loop (every instance: 4, 8, 16 lanes per env, masked, episodic, empty segments)
    asm volatile("" ::"v"(net.b2));
    bool alive = true;
    place_loop<PADS::loop(LPE, true, MASKED, true)>();
    for (int t = 0; t < max_step; ++t) {
        if constexpr (!FIXED_LENGTH) {
            if (__ballot(alive) == 0ull) break;
        }
        float obs[4] = {P.x, V.x, P.y, V.y};
        if constexpr (MASKED) {
#pragma unroll
            for (int k = 0; k < 4; ++k) obs[k] = ((obs_mask >> k) & 1u) ? 0.0f : obs[k];
        }
        typename MlpSlicePk<LPE>::Pending pending;
        net.begin(tanh_tab, obs, pending);
        // ---- the action-independent half of the physics (cartpole_pre_small), next to the table reads
        const float th = P.y, thd = V.y;
        const float z = th * th;
        const pk2 zz = pk_splat(z);
        pk2 pz = pk_fma(k0, zz, k1);
        pz = pk_fma(pz, zz, k2);
        pz = pz * zz;                                         // (pc * z, ps * z)
        CartPolePre pre;
        pre.sn = fma_(pz.y, th, th);
        pre.cs = fma_(pz.x, z, fma_(-0.5f, z, 1.0f));
        pre.q = CP_PML_OVER_MASS * (thd * thd);
        pre.gsn = CP_GRAVITY * pre.sn;
        pre.den = fma_(CP_DEN_C1, pre.cs * pre.cs, CP_DEN_C0);
        {
            const float r0 = __builtin_amdgcn_rcpf(pre.den);
            pre.rden = fma_(fma_(-pre.den, r0, 1.0f), r0, r0);
        }
        // ---- policy, action, the action-dependent half (cartpole_post)
        const pk2 lg = net.finish(pending);
        const bool one = lg.y > lg.x;                         // argmax_first<2>: the first maximum wins
        const float fom = one ? CP_FORCE_OVER_MASS : -CP_FORCE_OVER_MASS;
        const float temp = fma_(pre.q, pre.sn, fom);
        const float num = fma_(-pre.cs, temp, pre.gsn);
        const float thacc = cartpole_quotient(num, pre);
        const float xacc = fma_(-CP_PML_OVER_MASS * thacc, pre.cs, temp);
        const pk2 Pn = pk_fma(tau2, V, P);                    // (x + tau xd, theta + tau thetad): old velocities
        const pk2 Vn = pk_fma(tau2, pk2{xacc, thacc}, V);
        const float nx = clamp_sym_reg(Pn.x, lim_clamp);
        const float nth = __builtin_amdgcn_fmed3f(Pn.y, -th_clamp, th_clamp);
        const float nxd = clamp_sym_reg(Vn.x, lim_clamp);
        const float nthd = clamp_sym_reg(Vn.y, lim_clamp);
        if constexpr (FIXED_LENGTH) {
            P = pk2{nx, nth};
            V = pk2{nxd, nthd};
            steps = add_mask_bit(steps, alive_mask);
            alive_mask &= ~(__builtin_amdgcn_ballot_w64(__builtin_fabsf(nx) > CP_X_LIMIT) |
                            __builtin_amdgcn_ballot_w64(__builtin_fabsf(nth) > CP_THETA_LIMIT));
        } else {
            const bool term = (nx < -CP_X_LIMIT) || (nx > CP_X_LIMIT) || (nth < -CP_THETA_LIMIT) || (nth > CP_THETA_LIMIT);
            P = pk2{alive ? nx : P.x, alive ? nth : P.y};     // a finished env is frozen
            V = pk2{alive ? nxd : V.x, alive ? nthd : V.y};
            steps += (int)alive;
            alive = alive & !term;
        }
    }
    sim.P = P;
    sim.V = V;
}

}  // namespace ses
