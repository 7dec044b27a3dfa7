// ses_env_table.h -- what an env IS to the library: one EnvDesc row per env_id (the table itself: ses_envs.hip).  ses_create and
// ses_env_info validate a config by walking its row, the step-wise entry points and ses_rollout dispatch through its pointers.
// Declarations only.  What chooses kernel instances and tuning stays where it was (with_f64_env, ses_f64_envs.hip; ses_render.hip).
#pragma once
#include "ses_internal.h"

namespace ses {

constexpr int EITHER = -1;                       // EnvDesc::discrete: both heads exist (LunarLander-v2 / LunarLanderContinuous-v2)

struct EnvDesc {
    int env_id;
    const char *name;                            // as the messages say it
    // the policy shape: num_state = S, or s_per_agent * n_agents where s_per_agent is set; num_action = A
    int S, s_per_agent, A;
    int discrete;                                // discrete_action: 0, 1 or EITHER
    int agents_lo, agents_hi;                    // allowed n_agents; 0, 0: one agent, n_agents is not looked at
    bool gru_ok, pomdp_ok, physics64_ok;
    uint32_t pomdp_mask;                         // bit k: observation component k is zeroed under pomdp
    int max_eval_ep;                             // largest eval_ep_num; 0: no cap
    int init_w, init_w_per_agent;                // one initial-state row: init_w + init_w_per_agent * n_agents floats ...
    double init_lo, init_hi;                     // ... uniform in [init_lo, init_hi)
    bool has_ep_steps;                           // false: the rollout reports no ep_steps (episodes of one fixed length)
    bool is_f64;                                 // one of the float64 control envs (ses_f64_envs.hip)
    int (*state_bytes)(const ses_config *cfg);
    int (*reset)(ses_handle *h, const float *init, int n, void *state, float *obs);
    int (*step)(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done);
    int (*rollout)(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode);   // plan: ses_rollout_plan.h

    int agents(const ses_config *cfg) const { return agents_hi ? cfg->n_agents : 1; }
    int num_state(const ses_config *cfg) const { return s_per_agent ? s_per_agent * cfg->n_agents : S; }
    int obs_width(const ses_config *cfg) const { return num_state(cfg) * agents(cfg); }
    int init_width(const ses_config *cfg) const { return init_w + init_w_per_agent * cfg->n_agents; }
    // the step-wise action: int32 under the discrete head, float32[.., A] under the continuous one; a team's has an agents axis
    int action_layout(const ses_config *cfg) const
    {
        if (cfg->discrete_action) return agents_hi ? SES_ACTION_I32_N_AGENTS : SES_ACTION_I32_N;
        return agents_hi ? SES_ACTION_F32_N_AGENTS_A : SES_ACTION_F32_N_A;
    }
};

const EnvDesc *env_table_row(int i);             // row i of the table, nullptr past its last row

const EnvDesc *env_desc(int env_id);             // nullptr: SES_ENV_NONE, or an id without a row
const EnvDesc *env_desc(const ses_handle *h);
inline bool is_f64_env(const ses_handle *h) { const EnvDesc *d = env_desc(h); return d && d->is_f64; }

// Walks the row of cfg->env_id: SES_OK and *row, or SES_ERR_INVALID_ARG with "<who>: <name> needs <field>=<want>, got <have>".
// SES_ENV_NONE is SES_OK with *row = nullptr.
int env_check_config(const char *who, const ses_config *cfg, const EnvDesc **row);

// ---- the rows' entry functions that live in other units (the four envs of ses_envs.hip have theirs there) ----------------------
int rollout_cartpole(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode);     // ses_rollout.hip
int rollout_lander(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode);
int rollout_walker(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode);
int rollout_spread(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode);

// The eight float64 control envs (ses_f64_envs.hip).  The step-wise action is int32[n] for the discrete ones, float32[n, A] for the others.
int f64_env_state_bytes(const ses_config *cfg);
int f64_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs);
int f64_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done);
int f64_rollout(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode);

// waterworld (ses_waterworld.hip): action float32[n, 5, 2], already scaled
int waterworld_env_state_bytes(const ses_config *cfg);
int waterworld_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs);
int waterworld_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done);
int waterworld_rollout(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode);

// pursuit (ses_pursuit.hip): action int32[n, 8]
int pursuit_env_state_bytes(const ses_config *cfg);
int pursuit_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs);
int pursuit_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done);
int pursuit_rollout(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode);


// HopperBulletEnv-v0 (ses_hopper.hip): action float32[n, 3]
int hopper_env_state_bytes(const ses_config *cfg);
int hopper_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs);
int hopper_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done);
int hopper_rollout(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode);

// Walker2DBulletEnv-v0 (ses_walker2d.hip): action float32[n, 6]
int walker2d_env_state_bytes(const ses_config *cfg);
int walker2d_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs);
int walker2d_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done);
int walker2d_rollout(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode);

// BipedalWalkerHardcore-v3 (ses_walker_hardcore.hip): action float32[n, 4]
int walker_hardcore_env_state_bytes(const ses_config *cfg);
int walker_hardcore_env_reset(ses_handle *h, const float *init, int n, void *state, float *obs);
int walker_hardcore_env_step(ses_handle *h, void *state, const void *action, int n, float *obs, float *reward, int32_t *done);
int walker_hardcore_rollout(ses_handle *h, const RolloutArgs &a, const RolloutPlan &plan, int mode);

}  // namespace ses
