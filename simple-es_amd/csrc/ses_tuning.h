// ses_tuning.h -- the tuning knobs of a handle (ses_set_tuning), ONCE: struct Tuning holds every knob with its default and its one
// comment, tuning_knob() the table row of each -- public name, member, range, and the only values allowed where the range says too
// much -- and tuning_set() is the one place a (name, value) pair is checked and applied.  ses_set_tuning, ses_tuning_info and the
// overrides of ses_rollout_plan go through it.  Host only: include/ses.h and the standard library, no HIP header, no handle.
#pragma once
#include <cstring>

#include "../../include/ses.h"

namespace ses {

int set_error(int code, const char *fmt, ...);   // ses_core.hip: the message ses_last_error returns

// The defaults are the measured crossovers; the rules that read the rollout knobs are in ses_rollout_plan.h.
struct Tuning {
    int rollout_block = 64;         // workgroup size of the pure-LPE CartPole MLP rollout: 64 or 256
    int gru_mfma_min_e = 12;        // eval_ep_num from which GRU rollouts run on the MFMA kernel
    int gru_mfma4_min_e = 7;        // eval_ep_num (... 8) from which the CartPole GRU rollout takes the 4x4x1 MFMA step; 0 = never.  Measured
                                    // (profiles/r06_time_gru.txt): 2.97 ms for any E <= 8 against 3.14 / 3.34 ms of the VALU lockstep kernel at 7 / 8
    int gru_ep_parallel_max = 4096; // (offspring x episode) count up to which GRU rollouts use one wave per episode
    int gru_sequential = 0;         // 1: episode-after-episode GRU kernels only
    int rollout_mix = 1;            // 0: no mixed LPE-8 / LPE-4 split for mid-sized CartPole MLP populations
    int rollout_waves8 = 1024;      // light waves of the mixed split
    int rollout_mix_light = 0;      // lanes per env of the light waves: 0 = choose, 8, 16
    int rollout_lpe32_max = 0;      // CartPole MLP populations of up to this many envs run at 32 lanes per env (0: never)
    int rollout_mix_8_16 = 1;       // 1: the (8 lanes per env on every SIMD + the rest at 16) split is a candidate (round 6)
    int rollout_handover_step = 1 << 30;      // (16, 4) mix, fixed length: step at which the heavy wave hands half its envs over (round 7);
                                              // off: measured slower than the priority alone (NOTES round 7)
    int rollout_heavy_prio_steps = 1 << 30;   // (16, 4) mix, fixed length: steps the heavy wave runs at s_setprio 1 (round 7); the whole
                                              // episode: 0.213 -> 0.197 ms per generation (profiles/r07_handover_sweep.txt)
    int rollout_packed = -1;        // the packed step of lone waves (ses_policy_pk.h): -1 = when every wave has a SIMD to itself, 0 / 1
    int rollout_heavy_packed = -1;  // the packed step in the heavy wave of the pair kernels: -1 = the launcher decides, 0 / 1 (round 9)
    int comm_force_rccl = 0;        // 1: ses_allgather_fitness ignores an attached peer-store transport (A/B measurements)
    int es_final_max_chunks = 0;    // ses_openai_generation: up to this many 1024-row chunks the gradient kernel applies Adam itself;
                                    // measured: the wave-per-parameter update launch beats the in-kernel finisher
    int es_tail_wide = 1;           // ses_openai_generation: 1 (default) = the wide (1024-thread) form of the gradient kernel, 0 = the form before it
    int box2d_lpe = 0;              // lanes per env of the Box2D MLP rollout: 0 = by population size, 1 / 2 / 4 / ... / 64
    int env_step_block = 64;        // threads per workgroup of the standalone env-step kernel (64)
    int env_step_lds = -1;          // bytes of LDS each of its workgroups reserves without touching them: limits the waves in flight;
                                    // -1 (default): derived from the device's LDS per CU and env_step_waves (ses_rollout.hip: env_step_resolve)
    int env_step_waves = 7;         // waves per CU the derived reservation keeps in flight (7: what the memory system wants)
    int fused_elite = 1;            // 1 (default): ses_run_generations on one GPU runs the elite strategies' tail of populations up to 512
                                    // rows (the kernel serves 1024; ONE workgroup counts -- n compares per row -- so the loop stops using it at 512, twice the reference's largest config) as [mean + rank + best + selection] and, simple_evolution, [elite rows + mean]: two launches for seven
    int fused_apply_perturb = 1;    // 1 (default): the replicated openai_es tail of policies up to 1024 parameters applies the update inside the
                                    // launch that writes the next population (k_es_apply_perturb): one launch less per generation
    int fused_mean = 1;             // 1 (default): ses_run_generations on one GPU, openai_es up to 8192 rows: the rollout leaves the episode returns and the
                                    // counting rank of the tail forms the means itself (k_rank_count_episodes): one launch less per generation
    int box2d_epw = 0;              // different envs per wave of the Box2D MLP rollout: 0 = by population size, else <= 64 / lanes per env
    int lander_per_wave = 0;        // offspring per wave of the lockstep lander rollout: 0 = by population size, 1 / 2 / 4
    int comm_p2p_timeout_ms = 0;    // how long a peer-store exchange waits for a peer (0 = the default, 60 s)
    int comm_p2p_keep_going = 0;    // 1: exchanges continue after a time-out (the host polls ses_comm_p2p_status and recovers)
    int fused_fitness = 1;          // 1 (default): in a sharded ses_run_generations the FITNESS exchange needs no launch either: the episode-mean kernel stores the values as
                                    // granules into every rank's mailbox, the rank kernel of the tail polls them (RolloutOpts, OpenaiTailOpts)
    int comm_granules_enabled = 1;  // 0: this handle's transport refuses granule exchanges (comm_p2p_granules_begin: unsupported) -- set by a host
                                    // whose check of them failed (ses/parallel.py); the flag-based exchanges carry everything then
    int comm_granules = 0;          // 1: ses_allgather_fitness over the peer-store transport moves {sequence, value} granules (no flag, no fence)
                                    // while a shard fits half a mailbox section; 0 (default): the kernel with sequence words -- for a whole
                                    // shard the per-float stores and polls cost more than the one release / acquire round they save
                                    // (measured: 12.4 us against 6.3, 4096 floats, two ranks)
    int openai_granules = 1;        // 0: the shard form all-gathers its chunk partials as floats with a launch of its own also on the
                                    // peer-store transport (default 1: {sequence, value} granules stored by the gradient kernel itself)
    int openai_sharded_tail = 1;    // 0: ses_openai_sharded_ok says no (sharded runs use the replicated openai_es tail; A/B runs)
    int openai_sharded_min_rows = 8192;   // populations below this many rows IN TOTAL keep the replicated tail (default 8192)
    int fused_perturb_rollout = 1;  // 1 (default): inside ses_run_generations the rollout of the pair kernel forms its own rows of the
                                    // population from the previous generation's chunk partials (k_rollout_cartpole_mlp_handover_perturb):
                                    // no k_es_apply_perturb launch between generations of one call
    int pendulum_generic = 0;       // 1: the Pendulum MLP rollout runs the generic observe / step form of k_rollout_f64_mlp instead of the
                                    // one-trig form; identical results, for A/B timing (default 0)
    int pgpe_fused_apply_perturb = 1;     // 1 (default): ses_pgpe_generation for policies up to 1024 parameters and 16 chunks of pairs applies
                                          // the update inside the launch that draws the next population (k_pgpe_apply_perturb); 0: two launches
    int spread_gru_wave_per_batch = -1;   // simple_spread GRU rollout: 0 = a wave plays the column batches of its offspring one after the
                                          // other, 1 = one wave per (offspring, batch), -1 (default): by the number of waves (ses_spread_gru.hip)
    int waterworld_fc1_mfma = -1;   // waterworld rollout: 1 = fc1 on v_mfma_f32_32x32x2_f32, 0 = the same chain on the VALU, -1 (default):
                                    // the form measured faster (ses_waterworld.hip)
    int pursuit_fc1_mfma = -1;      // pursuit rollout: the same choice for its 147-wide fc1 (ses_pursuit.hip)
    int pendula_generic = -1;       // MLP rollout of the inverted-pendulum family: 1 = the generic observe / step form of k_rollout_f64_mlp,
                                    // 0 = the one-trig form, -1 (default): the form measured faster for the env (ses_f64_envs.hip); identical results
    int reacher_generic = -1;       // the same choice for the Reacher MLP rollout (ses_f64_envs.hip); -1 (default): the one-trig form
    int ars_fused_apply_perturb = 1;      // 1 (default): ses_ars_generation for policies up to 1024 parameters and 16 chunks of selected pairs
                                          // applies the update inside the launch that draws the next population (k_ars_perturb<true>); 0: two launches
};

// One row per member of Tuning: the name ses_set_tuning knows it by, [lo, hi], and -- where not every value of the range is
// one -- the values allowed (n_allowed of them) with the words the refusal says them in.
struct Knob {
    const char *name;
    int Tuning::*field;
    int lo, hi;
    int n_allowed;                  // 0: the whole range
    int allowed[8];
    const char *allowed_text;
};

// row i of the table, nullptr past its last row (a function's static, as the env table: ses_env_table.h)
inline const Knob *tuning_knob(int i)
{
    static const Knob table[] = {
        {"rollout_block", &Tuning::rollout_block, 64, 256, 2, {64, 256}, "64 or 256"},
        {"gru_mfma_min_e", &Tuning::gru_mfma_min_e, 1, 1 << 30},
        {"gru_mfma4_min_e", &Tuning::gru_mfma4_min_e, 0, 8},
        {"gru_ep_parallel_max", &Tuning::gru_ep_parallel_max, 0, 1 << 30},
        {"gru_sequential", &Tuning::gru_sequential, 0, 1},
        {"rollout_mix", &Tuning::rollout_mix, 0, 1},
        {"rollout_waves8", &Tuning::rollout_waves8, 1, 1 << 20},
        {"rollout_mix_light", &Tuning::rollout_mix_light, 0, 16, 3, {0, 8, 16}, "0, 8 or 16"},
        {"rollout_lpe32_max_envs", &Tuning::rollout_lpe32_max, 0, 1 << 30},
        {"rollout_packed", &Tuning::rollout_packed, -1, 1},
        {"rollout_heavy_packed", &Tuning::rollout_heavy_packed, -1, 1},
        {"rollout_mix_8_16", &Tuning::rollout_mix_8_16, 0, 1},
        {"rollout_handover_step", &Tuning::rollout_handover_step, 0, 1 << 30},
        {"rollout_heavy_prio_steps", &Tuning::rollout_heavy_prio_steps, 0, 1 << 30},
        {"lander_offspring_per_wave", &Tuning::lander_per_wave, 0, 4, 4, {0, 1, 2, 4}, "0, 1, 2 or 4"},
        {"box2d_lanes_per_env", &Tuning::box2d_lpe, 0, 64, 8, {0, 1, 2, 4, 8, 16, 32, 64}, "0 or a power of two up to 64"},
        {"box2d_envs_per_wave", &Tuning::box2d_epw, 0, 64},
        {"pendulum_generic_step", &Tuning::pendulum_generic, 0, 1},
        {"pendula_generic_step", &Tuning::pendula_generic, -1, 1},
        {"reacher_generic_step", &Tuning::reacher_generic, -1, 1},
        {"env_step_block", &Tuning::env_step_block, 64, 256, 3, {64, 128, 256}, "64, 128 or 256"},
        {"env_step_lds_bytes", &Tuning::env_step_lds, -1, 65536},
        {"env_step_waves_per_cu", &Tuning::env_step_waves, 1, 32},
        {"es_final_max_chunks", &Tuning::es_final_max_chunks, 0, 1 << 20},
        {"es_tail_wide", &Tuning::es_tail_wide, 0, 1},
        {"comm_force_rccl", &Tuning::comm_force_rccl, 0, 1},
        {"comm_p2p_timeout_ms", &Tuning::comm_p2p_timeout_ms, 0, 1 << 30},
        {"comm_p2p_keep_going", &Tuning::comm_p2p_keep_going, 0, 1},
        {"openai_sharded_tail", &Tuning::openai_sharded_tail, 0, 1},
        {"openai_sharded_min_rows", &Tuning::openai_sharded_min_rows, 0, 1 << 30},
        {"openai_granule_exchange", &Tuning::openai_granules, 0, 1},
        {"comm_granule_allgather", &Tuning::comm_granules, 0, 1},
        {"comm_granules_enabled", &Tuning::comm_granules_enabled, 0, 1},
        {"fused_fitness_exchange", &Tuning::fused_fitness, 0, 1},
        {"fused_episode_mean", &Tuning::fused_mean, 0, 1},
        {"fused_elite_tail", &Tuning::fused_elite, 0, 1},
        {"fused_apply_perturb", &Tuning::fused_apply_perturb, 0, 1},
        {"fused_perturb_rollout", &Tuning::fused_perturb_rollout, 0, 1},
        {"pgpe_fused_apply_perturb", &Tuning::pgpe_fused_apply_perturb, 0, 1},
        {"ars_fused_apply_perturb", &Tuning::ars_fused_apply_perturb, 0, 1},
        {"spread_gru_wave_per_batch", &Tuning::spread_gru_wave_per_batch, -1, 1},
        {"waterworld_fc1_mfma", &Tuning::waterworld_fc1_mfma, -1, 1},
        {"pursuit_fc1_mfma", &Tuning::pursuit_fc1_mfma, -1, 1},
    };
    constexpr int rows = (int)(sizeof table / sizeof table[0]);
    static_assert(rows == (int)(sizeof(Tuning) / sizeof(int)), "every member of Tuning has one row in the knob table");
    return i >= 0 && i < rows ? &table[i] : nullptr;
}

// Checks `value` against the row of knob `name` and stores it in t: SES_OK, or SES_ERR_INVALID_ARG and the message, said by `who`
// (range first, then the value list; a name without a row last).  *set (or null): the row that took the value.
inline int tuning_set(Tuning &t, const char *who, const char *name, int value, const Knob **set = nullptr)
{
    for (int i = 0; const Knob *k = tuning_knob(i); ++i) {
        if (std::strcmp(k->name, name) != 0) continue;
        if (value < k->lo || value > k->hi)
            return set_error(SES_ERR_INVALID_ARG, "%s: %s = %d outside [%d, %d]", who, name, value, k->lo, k->hi);
        bool listed = k->n_allowed == 0;
        for (int j = 0; j < k->n_allowed; ++j) listed = listed || k->allowed[j] == value;
        if (!listed) return set_error(SES_ERR_INVALID_ARG, "%s: %s must be %s", who, name, k->allowed_text);
        t.*(k->field) = value;
        if (set) *set = k;
        return SES_OK;
    }
    return set_error(SES_ERR_INVALID_ARG, "%s: unknown knob '%s'", who, name);
}

}  // namespace ses
