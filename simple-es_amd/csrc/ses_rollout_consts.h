// ses_rollout_consts.h -- the few constants that both the rollout kernels and the launch rules (ses_rollout_plan.h) read: a kernel's
// layout on one side, a rule's threshold on the other.  Plain C++, no HIP header.
#pragma once

namespace ses {

inline int ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }

constexpr int GL_EB = 8;   // episodes per lockstep batch = owner slots per 8-lane group (ses_gru_lockstep.h)
constexpr int G4_EB = 8;   // episodes per batch of the 4x4x1 MFMA form = 2 column blocks of 4 (ses_gru_mfma4.h)

constexpr int HANDOVER_PAIRS = 4;   // light + heavy wave pairs of one workgroup of the pair kernels (ses_rollout.hip)

// waves per SIMD the Box2D MLP rollout kernel is built for (its launch bounds) and its wave shape is chosen by
constexpr int LANDER_MLP_WAVES_PER_SIMD = 2;   // 256 registers for the kernel and for ll_step: enough
constexpr int WALKER_MLP_WAVES_PER_SIMD = 1;   // bw_step may then use all 512 registers (ses_rollout.hip: WalkerMlpEnv)
constexpr int HOPPER_MLP_WAVES_PER_SIMD = 2;   // the hopper's world is a third smaller than the walker's (ses_hopper.hip)
#ifndef SES_WALKER2D_WAVES
#define SES_WALKER2D_WAVES 1                   // -DSES_WALKER2D_WAVES=2: the other build of tools/time_walker2d.py
#endif
// measured both ways on an MI355X (profiles/walker2d_timing.txt): with 512 registers w2d_step keeps the seven-body world out
// of scratch in both iteration loops, and one wave per SIMD is 1.5 - 3.4 x faster than two on every row
constexpr int WALKER2D_MLP_WAVES_PER_SIMD = SES_WALKER2D_WAVES;
// BipedalWalkerHardcore-v3 (ses_walker_hardcore.hip): the walker's world with eight manifold slots per leg needs the 512 registers
// no less than bw_step does; and a terrain row is 2192 bytes of LDS, so four single-wave workgroups fit a CU's 160 KiB -- one wave on
// each SIMD -- with at most 16 rows each next to the tanh table (the unit's header has the table)
constexpr int WALKER_HARDCORE_MLP_WAVES_PER_SIMD = 1;
constexpr int WALKER_HARDCORE_MAX_EPW = 16;

}  // namespace ses
