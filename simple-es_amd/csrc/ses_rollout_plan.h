// ses_rollout_plan.h -- which form of its rollout kernels a population runs in: plan_rollout() decides it ONCE per rollout, from the
// config, the knobs (ses_tuning.h) and the population alone, and the launchers of ses_rollout.hip only dispatch on the RolloutPlan.
// The rules below carry the project's measured crossovers; every form computes the same bits, so a wrong choice costs time, never
// a result -- which is why they are pure host functions: ses_rollout_plan (include/ses.h) evaluates them without a device and
// tests/test_rollout_plan_host.py pins them.  Host only: include/ses.h, ses_tuning.h, the shared constants, the standard library.
#pragma once
#include <cstddef>
#include <initializer_list>

#include "ses_rollout_consts.h"
#include "ses_tuning.h"

namespace ses {

// The forms of the GRU rollout (CartPole, LunarLander); gru_form() below holds the precedence.  (values: SES_GRU_FORM_*, include/ses.h)
enum class GruForm {
    Sequential = SES_GRU_FORM_SEQUENTIAL, EpisodeParallel = SES_GRU_FORM_EPISODE_PARALLEL, Mfma4 = SES_GRU_FORM_MFMA4, Mfma = SES_GRU_FORM_MFMA,
    LockstepMulti4 = SES_GRU_FORM_LOCKSTEP_MULTI4, LockstepMulti2 = SES_GRU_FORM_LOCKSTEP_MULTI2, Lockstep = SES_GRU_FORM_LOCKSTEP
};

// Whose launcher runs the rollout (values: SES_PLAN_*, include/ses.h).  Other: the envs whose form is chosen in other units -- the
// float64 envs, simple_spread, waterworld, pursuit -- and nothing else of the plan is set.
enum class RolloutFamily {
    Other = SES_PLAN_OTHER, CartPoleMlpPure = SES_PLAN_CARTPOLE_MLP_PURE, CartPoleMlpMix = SES_PLAN_CARTPOLE_MLP_MIX,
    CartPoleMlpPair = SES_PLAN_CARTPOLE_MLP_PAIR, CartPoleMlpF64 = SES_PLAN_CARTPOLE_MLP_F64, Gru = SES_PLAN_GRU, Box2dMlp = SES_PLAN_BOX2D_MLP
};

struct RolloutPlan {
    RolloutFamily family = RolloutFamily::Other;
    // CartPole MLP.  Pure, F64: every wave at lanes_rest lanes per env.  Mix, Pair: the first waves_light waves at lanes_light lanes
    // per env, the remaining waves_rest at lanes_rest; Pair: as light + heavy wave pairs whose heavy wave hands over at step `handover`.
    int lanes_light = 0, lanes_rest = 0;
    int waves_light = 0, waves_rest = 0, handover = 0;
    bool packed = false;          // Pure: the packed step (ses_policy_pk.h)
    int heavy_packed = 0;         // Pair: the packed step in the heavy wave
    int block = 64;               // Pure: threads per workgroup
    bool own_rows_ok = false;     // Pair: the rollout may form its own rows in its prologue (cartpole_perturb_rollout_ok)
    GruForm gru_form = GruForm::Lockstep;        // Gru
    int box2d_lpe = 0, box2d_epw = 0;            // Box2dMlp: lanes per env, different envs per wave
};

inline int pick_lanes_per_env(const ses_config &cfg, long long n_env)
{
    if (cfg.lanes_per_env) return cfg.lanes_per_env;
    // Measured on MI355X (round 1 sweep, profiles/r01_rollout_occupancy_sweep.txt): 4 lanes per env wins from 20 480 envs (1280 waves) up to
    // 327 680 envs; below ~10 000 envs only LPE = 8 still gives every SIMD a wavefront, and while even that leaves the
    // population within one wave per SIMD (4096 envs) 16 lanes per env make the lone wave's step shorter still
    // (83 instead of 104 instructions: conf/cartpole.yaml's 480 envs are 500 sequential steps of such a wave).
    if (n_env * 4 / 64 >= 640) return 4;
    return n_env <= 4096 ? 16 : 8;
}

// The packed step (ses_policy_pk.h) pays where a wave has its SIMD to itself: populations of at most one wave per SIMD at the
// chosen lanes per env.  ses_set_tuning "rollout_packed": -1 = this rule (default), 0 = never, 1 = whenever the split is 8 or 16.
inline bool cartpole_mlp_packed(const Tuning &t, int lpe, long long episodes)
{
    if (lpe != 8 && lpe != 16) return false;
    if (t.rollout_packed >= 0) return t.rollout_packed != 0;
    return ceil_div(episodes * lpe, 64) <= t.rollout_waves8;          // (the knob holds the chip's SIMD count: 1024)
}

// Envs per wave and lanes per env of the Box2D MLP rollout.  A wave-step costs about as much as the wave carries
// different envs (the union of their contact rows, impacts, position iterations), so the population is spread over every
// wave slot of the chip -- 1024 SIMDs x EnvB::WAVES_PER_SIMD, all resident at once -- with as few envs per wave as that
// allows, and the lanes per env are the largest power of two that fits them.  BipedalWalker, 4096 x 5 episodes: 32 envs
// on each of 640 waves 374 ms, 16 on each of 1280 (two rounds on 1024 slots) 356 ms, 20 on each of 1024 -> see DESIGN.md.
// ses_set_tuning "box2d_lanes_per_env" forces LPE (and 64 / LPE envs per wave unless "box2d_envs_per_wave" is set too).
inline void box2d_wave_shape(const Tuning &t, long long episodes, int waves_per_simd, int &lpe, int &epw)
{
    if (t.box2d_lpe) {
        lpe = t.box2d_lpe;
        epw = t.box2d_epw ? t.box2d_epw : 64 / lpe;
        if (epw > 64 / lpe) epw = 64 / lpe;
        return;
    }
    const long long slots = 1024ll * waves_per_simd;
    long long need = t.box2d_epw ? t.box2d_epw : (episodes + slots - 1) / slots;
    epw = (int)(need < 1 ? 1 : need > 64 ? 64 : need);
    lpe = 64;
    while (lpe > 1 && epw * lpe > 64) lpe >>= 1;
}

// Offspring per wave of the lockstep lander rollout (k_rollout_gru_lockstep_multi): as many as leave about two waves
// per SIMD (2048 on the chip), all resident at once.  The env step is a sequential 20 000-instruction routine: a
// rollout costs (steps of the longest episode) x (time of one wave-step), a wave-step costs the same for 5 or 20 envs,
// and two waves on a SIMD fill each other's dependency stalls.  Measured, C3 (4096 offspring x 5 episodes, one box):
// 1 offspring per wave 44.8 ms, 2: 31.8 ms, 4: 35.9 ms (one wave per SIMD, and with 20 envs in a wave most steps have
// some env on the ground, i.e. run the contact rows).
// ses_set_tuning "lander_offspring_per_wave": 0 = this rule, 1 / 2 / 4 = forced.
inline int lander_offspring_per_wave(const Tuning &t, int n_rows)
{
    if (t.lander_per_wave) return t.lander_per_wave;
    // round 3: a finished offspring's GRU step is skipped, which makes four offspring per wave the better choice from
    // ~3000 offspring on (C3, 4096 x 5 x <= 300: 40.6 ms at two per wave, 37.4 at four, same box; tools/c3_breakdown.py)
    return n_rows >= 3072 ? 4 : (n_rows >= 1536 ? 2 : 1);
}

// Which form of the GRU rollout runs (CartPole, LunarLander).  The tests below, IN THIS ORDER, are the whole precedence:
// the first that holds decides.  Every form computes the same bits, so no GPU test sees a wrong choice here: only the clock does
// -- and tests/test_rollout_plan_host.py, which holds the crossovers.  (lander: LunarLander, else CartPole)
inline GruForm gru_form(const ses_config &cfg, const Tuning &t, int n_rows, bool lander)
{
    const int E = cfg.eval_ep_num;
    // ses_set_tuning "gru_sequential" = 1 selects the episode-after-episode GRU kernels
    if (t.gru_sequential != 0) return GruForm::Sequential;
    // Small populations: the chip is far from full and what a rollout costs is the latency of max_step sequential env
    // steps.  The lockstep kernel spends ~1.7 us per step (all E episodes of an offspring in one wave), the
    // episode-after-episode kernel ~0.75 us per step and episode -- launched with one wave per (offspring, episode) it
    // finishes in one episode's time.  Measured, POMDP CartPole, E = 5, 500 steps (lockstep / episode-parallel, ms):
    // 96 offspring 0.87 / 0.37, 400: 0.87 / 0.46, 800: 0.87 / 0.82, 1200: 1.22 / 1.13, 1600: 1.23 / 1.48, 4096: 2.41 / 3.50.
    // (ses_set_tuning "gru_ep_parallel_max": (offspring x episode) waves up to which the form is used, default 4096)
    if ((long long)n_rows * E <= t.gru_ep_parallel_max && E > 1) return GruForm::EpisodeParallel;
    // eval_ep_num for which the CartPole GRU rollout takes the 4x4x1 MFMA step (ses_set_tuning "gru_mfma4_min_e" ... 8; 0 = never)
    if (!lander && t.gru_mfma4_min_e > 0 && E >= t.gru_mfma4_min_e && E <= G4_EB) return GruForm::Mfma4;
    // eval_ep_num from which the GRU rollouts run on the matrix cores (ses_set_tuning "gru_mfma_min_e", default 12).
    // Measured, POMDP CartPole, 4096 offspring x 500 steps: the MFMA form takes 5.1 ms for any E <= 16 (the padded tile
    // costs the same), the VALU lockstep form 2.4 / 3.5 / 5.6 / 7.2 ms at E = 5 / 8 / 12 / 16 -- the crossover is at 12.
    if (E >= t.gru_mfma_min_e) return GruForm::Mfma;
    const int per_wave = lander && E <= GL_EB ? lander_offspring_per_wave(t, n_rows) : 1;
    return per_wave == 4 ? GruForm::LockstepMulti4 : (per_wave == 2 ? GruForm::LockstepMulti2 : GruForm::Lockstep);
}

// Which split of the lanes runs a CartPole MLP population of `episodes` envs.  Every split evaluates the same canonical
// arithmetic; what differs is how much the busiest SIMD has to issue per env step and with how many waves it shares the
// issue port.  Model (profiles/r03_ab_mix_light.txt, MI355X): a wave's loop body is 160 / 104 / 84 VALU instructions at 4 / 8 / 16
// lanes per env; a SIMD that holds k waves issues one of their instructions every 5.0 / 3.45 / 3.1 / 2.95 cycles (k = 1,
// 2, 3, >= 4: a lone wave waits for its own dependences).  Candidates: the pure splits, and "one light wave per SIMD
// (8 or 16 lanes per env) + the rest at 4 lanes per env".  Measured against the model at 3072 / 4096 / 5120 offspring x 5
// episodes: pure 8 (167.7 us) / light 16 + 4 (195.0 us; round 2's light 8 + 4: 213.8) / pure 4 (239.5), all as predicted.
struct MlpSplit {
    int light;      // 0: pure split at `lpe` lanes per env; 8 / 16: mixed, the first waves at this many lanes per env
    int lpe;        // pure: lanes per env; mixed: lanes per env of the remaining waves (4, or 16 behind first waves of 8)
};

inline MlpSplit choose_cartpole_mlp_split(const ses_config &cfg, const Tuning &t, long long episodes)
{
    if (cfg.lanes_per_env) return MlpSplit{0, cfg.lanes_per_env};
    // round 6: 32 lanes per env (77 VALU instructions per step against 83 at 16, but two more dependent steps in fc2) -- a knob,
    // off by default: profiles/r06_small_populations.txt has the A/B that decides it
    if (t.rollout_lpe32_max > 0 && episodes <= t.rollout_lpe32_max) return MlpSplit{0, 32};
    if (episodes > 49152) return MlpSplit{0, 4};                       // large populations: 4 lanes per env (round 1 sweep)
    const int simds = t.rollout_waves8;                                 // 1024 = 256 CUs x 4 (knob: the first waves of a mix)
    auto instr = [](int lpe) { return lpe == 4 ? 160.0 : (lpe == 8 ? 104.0 : 84.0); };
    auto cadence = [](long long k) { return k <= 1 ? 5.0 : (k == 2 ? 3.45 : (k == 3 ? 3.1 : 2.95)); };
    MlpSplit best{0, 8};
    double best_cost = -1.0;
    auto consider = [&](MlpSplit sp, double cost) {
        if (best_cost < 0.0 || cost < best_cost) { best_cost = cost; best = sp; }
    };
    const bool mix_only = t.rollout_mix_light != 0;
    if (!mix_only) {
        for (int lpe : {16, 8, 4}) {
            const long long k = ceil_div(ceil_div(episodes * lpe, 64), simds);
            consider(MlpSplit{0, lpe}, k * instr(lpe) * cadence(k));
        }
    }
    if ((t.rollout_mix || mix_only) && episodes > 8192) {
        for (int light : {16, 8}) {
            if (mix_only && light != t.rollout_mix_light) continue;
            const long long envs_light = (long long)simds * (64 / light);
            if (episodes <= envs_light) continue;
            const long long kh = ceil_div(ceil_div(episodes - envs_light, 16), simds);
            consider(MlpSplit{light, 4}, (instr(light) + 160.0 * kh) * cadence(1 + kh));
        }
        // 8 lanes per env on every SIMD, the rest at 16 lanes per env (round 6; knob "rollout_mix_8_16", default on)
        const long long envs8 = (long long)simds * 8;
        if (t.rollout_mix_8_16 && !mix_only && episodes > envs8) {
            const long long k16 = ceil_div(ceil_div(episodes - envs8, 4), simds);
            consider(MlpSplit{8, 16}, (104.0 + 84.0 * k16) * cadence(1 + k16));
        }
    }
    return best;
}

// The light + heavy pair kernel's launch shape for a mixed split `sp` of this population (the waves of any mix are counted the
// same way), or false when the mix kernel runs it
struct PairShape {
    int waves_light, waves_rest, handover;
};
inline bool cartpole_mlp_pair_shape(const ses_config &cfg, const Tuning &t, MlpSplit sp, long long episodes, int mode, PairShape &ps)
{
    const int epw = 64 / sp.light, knob = t.rollout_waves8, epw_rest = 64 / sp.lpe;
    ps.waves_light = (long long)knob * epw < episodes ? knob : (int)(episodes / epw);
    ps.waves_rest = ceil_div(episodes - (long long)epw * ps.waves_light, epw_rest);
    ps.handover = t.rollout_handover_step;
    return mode == SES_MODE_FIXED_LENGTH && sp.light == 16 && sp.lpe == 4 && ps.waves_rest <= ps.waves_light &&
           (ps.handover < cfg.max_step || t.rollout_heavy_prio_steps > 0);
}

// The heavy wave's step in the pair kernels.  ses_set_tuning "rollout_heavy_packed": -1 = this rule (default), 0 = the scalar
// form, 1 = the packed form (ses_policy_pk.h) wherever the wave's envs start inside the small-angle range.
constexpr int HEAVY_PACKED_DEFAULT = 1;
inline int cartpole_mlp_heavy_packed(const Tuning &t)
{
    return t.rollout_heavy_packed >= 0 ? t.rollout_heavy_packed : HEAVY_PACKED_DEFAULT;
}

// how many rows n consecutive envs can touch at most
inline int max_rows_of_envs(int n, int E) { return n <= 1 ? n : (n - 2) / E + 2; }
// rows of LDS the prologue form of the pair kernel needs at E envs per row
inline int pair_own_rows(int E) { return max_rows_of_envs(HANDOVER_PAIRS * (64 / 16), E) + max_rows_of_envs(HANDOVER_PAIRS * (64 / 4), E); }

// LDS the prologue form of the pair kernel may ask for on top of its static 6.5 KB (tanh table, hand-over slots): the mean and the
// workgroup's rows.  56 KB keeps the workgroup inside the 64 KB a workgroup may have; P = 226 fits E >= 2 (42 rows at E = 2).
constexpr size_t PERTURB_ROLLOUT_LDS_MAX = 56u << 10;
inline size_t perturb_rollout_lds(int P, int E) { return sizeof(float) * ((size_t)(P + 3) / 4 * 4 + (size_t)pair_own_rows(E) * P); }

// ses_run_generations, one GPU, replicated openai_es tail of at most APPLY_PERTURB_MAX_P parameters and _MAX_CHUNKS chunks (the
// caller's half): the CartPole rollout of these rows runs the pair kernel (`pair`), and its rows fit the LDS budget
inline bool cartpole_perturb_rollout_ok(const ses_config &cfg, const Tuning &t, int P, bool pair)
{
    if (!t.fused_perturb_rollout || cfg.gru || cfg.physics64) return false;
    if (P & 1) return false;                                         // (the prologue stores its rows 8 bytes at a time; P = 226 here)
    return pair && perturb_rollout_lds(P, cfg.eval_ep_num) <= PERTURB_ROLLOUT_LDS_MAX;
}

// The plan of the rollout of n_rows offspring (n_rows >= 1) of P parameters under `mode` (SES_MODE_*), by the env of the config.
inline RolloutPlan plan_rollout(const ses_config &cfg, const Tuning &t, int P, int n_rows, int mode)
{
    RolloutPlan p;
    const long long episodes = (long long)n_rows * cfg.eval_ep_num;
    switch (cfg.env_id) {
        case SES_ENV_CARTPOLE:
            if (cfg.gru) {
                p.family = RolloutFamily::Gru;             // (float64 dynamics: the lockstep form only)
                p.gru_form = cfg.physics64 ? GruForm::Lockstep : gru_form(cfg, t, n_rows, false);
            } else if (cfg.physics64) {
                // gym-order float64 dynamics: 4 / 8 lanes per env (parity option, not the bench path)
                p.family = RolloutFamily::CartPoleMlpF64;
                p.lanes_rest = pick_lanes_per_env(cfg, episodes) >= 8 ? 8 : 4;
            } else {
                const MlpSplit sp = choose_cartpole_mlp_split(cfg, t, episodes);
                p.lanes_light = sp.light;
                p.lanes_rest = sp.lpe;
                if (sp.light) {
                    // one wave of the first kind per SIMD (the dispatcher deals the first workgroups one per SIMD) + the rest
                    PairShape ps;
                    const bool pair = cartpole_mlp_pair_shape(cfg, t, sp, episodes, mode, ps);
                    p.family = pair ? RolloutFamily::CartPoleMlpPair : RolloutFamily::CartPoleMlpMix;
                    p.waves_light = ps.waves_light;
                    p.waves_rest = ps.waves_rest;
                    p.handover = ps.handover;
                    if (pair) p.heavy_packed = cartpole_mlp_heavy_packed(t);
                    p.own_rows_ok = cartpole_perturb_rollout_ok(cfg, t, P, pair);
                } else {
                    p.family = RolloutFamily::CartPoleMlpPure;
                    p.block = t.rollout_block == 256 ? 256 : 64;
                    p.packed = p.block != 256 && cartpole_mlp_packed(t, sp.lpe, episodes);
                }
            }
            break;
        case SES_ENV_LUNARLANDER:                          // either action head: LunarLander-v2 takes the continuous env's rules
            if (cfg.gru) {
                p.family = RolloutFamily::Gru;
                p.gru_form = gru_form(cfg, t, n_rows, true);
            } else {
                p.family = RolloutFamily::Box2dMlp;
                box2d_wave_shape(t, episodes, LANDER_MLP_WAVES_PER_SIMD, p.box2d_lpe, p.box2d_epw);
            }
            break;
        case SES_ENV_BIPEDALWALKER:
            p.family = RolloutFamily::Box2dMlp;
            box2d_wave_shape(t, episodes, WALKER_MLP_WAVES_PER_SIMD, p.box2d_lpe, p.box2d_epw);
            break;
        case SES_ENV_HOPPER:                               // (ses_hopper.hip) GRU: the single-wave lockstep form only
            if (cfg.gru) {
                p.family = RolloutFamily::Gru;
                p.gru_form = GruForm::Lockstep;
            } else {
                p.family = RolloutFamily::Box2dMlp;
                box2d_wave_shape(t, episodes, HOPPER_MLP_WAVES_PER_SIMD, p.box2d_lpe, p.box2d_epw);
            }
            break;
        case SES_ENV_WALKER2D:                             // (ses_walker2d.hip) GRU: the single-wave lockstep form only
            if (cfg.gru) {
                p.family = RolloutFamily::Gru;
                p.gru_form = GruForm::Lockstep;
            } else {
                p.family = RolloutFamily::Box2dMlp;
                box2d_wave_shape(t, episodes, WALKER2D_MLP_WAVES_PER_SIMD, p.box2d_lpe, p.box2d_epw);
            }
            break;
        case SES_ENV_BIPEDALWALKER_HARDCORE:               // (ses_walker_hardcore.hip) GRU: the single-wave lockstep form only
            if (cfg.gru) {
                p.family = RolloutFamily::Gru;
                p.gru_form = GruForm::Lockstep;
            } else {
                p.family = RolloutFamily::Box2dMlp;
                box2d_wave_shape(t, episodes, WALKER_HARDCORE_MLP_WAVES_PER_SIMD, p.box2d_lpe, p.box2d_epw);
                // a wave's terrain rows must leave LDS for one wave on every SIMD: unless the tuning forces a shape, no more than
                // WALKER_HARDCORE_MAX_EPW envs per wave (larger populations take more rounds of waves instead)
                if (!t.box2d_lpe && !t.box2d_epw && p.box2d_epw > WALKER_HARDCORE_MAX_EPW) {
                    p.box2d_epw = WALKER_HARDCORE_MAX_EPW;
                    p.box2d_lpe = 64 / WALKER_HARDCORE_MAX_EPW;
                }
            }
            break;
        default:
            break;
    }
    return p;
}

}  // namespace ses
