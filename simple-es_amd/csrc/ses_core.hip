// ses_core.hip -- handle lifecycle and error reporting of libses_hip.so (see include/ses.h)
#include <cstring>
#include <string>

#include "ses_env_table.h"

namespace ses {

static thread_local char g_err[512] = "";

int set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

int ensure_episode_scratch(ses_handle *h, size_t episodes)
{
    if (episodes <= h->ep_cap) return SES_OK;
    if (h->ep_return || h->ep_steps) SES_HIP_TRY(hipStreamSynchronize(h->stream));   // kernels may still use the old buffers
    if (h->ep_return) SES_HIP_TRY(hipFree(h->ep_return));
    if (h->ep_steps) SES_HIP_TRY(hipFree(h->ep_steps));
    h->ep_return = nullptr;
    h->ep_steps = nullptr;
    h->ep_cap = 0;
    SES_HIP_TRY(hipMalloc(&h->ep_return, episodes * sizeof(double)));
    SES_HIP_TRY(hipMalloc(&h->ep_steps, episodes * sizeof(int32_t)));
    h->ep_cap = episodes;
    return SES_OK;
}

int ensure_obs_norm_scratch(ses_handle *h, size_t doubles)
{
    if (doubles <= h->obs_norm_cap) return SES_OK;
    if (h->obs_norm_partials) {
        SES_HIP_TRY(hipStreamSynchronize(h->stream));               // kernels may still use the old buffer
        SES_HIP_TRY(hipFree(h->obs_norm_partials));
    }
    h->obs_norm_partials = nullptr;
    h->obs_norm_cap = 0;
    SES_HIP_TRY(hipMalloc(&h->obs_norm_partials, doubles * sizeof(double)));
    h->obs_norm_cap = doubles;
    return SES_OK;
}

int ensure_reduce_scratch(ses_handle *h, size_t bytes)
{
    if (bytes <= h->red_cap) return SES_OK;
    // grow generously: the buffer is re-used by every generation and a free/alloc pair would stall the stream
    size_t want = bytes < (1u << 20) ? (1u << 20) : bytes * 2;
    if (h->red_scratch) {
        SES_HIP_TRY(hipStreamSynchronize(h->stream));
        SES_HIP_TRY(hipFree(h->red_scratch));
    }
    h->red_scratch = nullptr;
    h->red_cap = 0;
    h->rank_zeroed = nullptr;                       // whatever was known about the old buffer's contents is gone
    h->counter_armed = nullptr;
    SES_HIP_TRY(hipMalloc(&h->red_scratch, want));
    h->red_cap = want;
    return SES_OK;
}

}  // namespace ses

extern "C" {

const char *ses_last_error(void) { return ses::g_err; }

const char *ses_version(void) { return "ses-hip 0.1 (gfx950)"; }

int ses_param_count(int32_t S, int32_t A, int32_t gru)
{
    int p = SES_HIDDEN * S + SES_HIDDEN + A * SES_HIDDEN + A;
    if (gru) p += 2 * (3 * SES_HIDDEN * SES_HIDDEN) + 2 * (3 * SES_HIDDEN);
    return p;
}

int ses_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return ses::set_error(SES_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

int ses_create(const ses_config *cfg, void *stream, ses_handle **out)
{
    SES_REQUIRE(cfg && out, "ses_create: null argument");
    const ses::EnvDesc *row;                                         // the env's own fields, by its table row (ses_env_table.h)
    const int checked = ses::env_check_config("ses_create", cfg, &row);
    if (checked != SES_OK) return checked;
    if (!row) {
        // A handle without an env serves the strategies and ses_policy_forward: the narrow policies, and the MLPs of the rows whose
        // observations are wider than those (waterworld, pursuit).
        bool wide = false;
        for (int i = 0; const ses::EnvDesc *d = ses::env_table_row(i); ++i)
            wide = wide || (d->S > 32 && cfg->num_state == d->S && cfg->num_action == d->A && !cfg->gru);
        SES_REQUIRE((cfg->num_state >= 1 && cfg->num_state <= 32) || wide, "ses_create: num_state %d out of range", cfg->num_state);
        SES_REQUIRE(cfg->num_action >= 1 && cfg->num_action <= 8, "ses_create: num_action %d out of range", cfg->num_action);
        SES_REQUIRE(!cfg->physics64, "ses_create: physics64 is a CartPole rollout option");
    }
    SES_REQUIRE(cfg->eval_ep_num >= 1, "ses_create: eval_ep_num must be >= 1");
    SES_REQUIRE(cfg->max_step >= 1 && cfg->max_step < (1 << 30), "ses_create: max_step must be in [1, 2^30)");
    SES_REQUIRE(cfg->lanes_per_env == 0 || cfg->lanes_per_env == 1 || cfg->lanes_per_env == 2 ||
                    cfg->lanes_per_env == 4 || cfg->lanes_per_env == 8 || cfg->lanes_per_env == 16 || cfg->lanes_per_env == 32,
                "ses_create: lanes_per_env must be 0, 1, 2, 4, 8, 16 or 32");
    int ndev = ses_device_count();
    if (ndev <= 0) return ses::set_error(SES_ERR_NO_DEVICE, "ses_create: no HIP device visible");
    SES_REQUIRE(cfg->device >= 0 && cfg->device < ndev, "ses_create: device %d not in [0,%d)", cfg->device, ndev);
    SES_HIP_TRY(hipSetDevice(cfg->device));
    ses_handle *h = new ses_handle();
    std::memset(h, 0, sizeof *h);
    h->cfg = *cfg;
    h->stream = (hipStream_t)stream;
    h->P = ses_param_count(cfg->num_state, cfg->num_action, cfg->gru);
    h->obs_mask = row && cfg->pomdp ? row->pomdp_mask : 0u;
    h->tune = ses::Tuning{};
    h->env_step_key[0] = -2;
    {
        int lds = 0;
        const hipError_t e = hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, cfg->device);
        if (e != hipSuccess) {
            delete h;                         // nothing else is owned yet
            return ses::set_error(SES_ERR_HIP, "ses_create: hipDeviceGetAttribute: %s", hipGetErrorString(e));
        }
        h->lds_per_cu = lds;
    }
    *out = h;
    return SES_OK;
}

int ses_set_tuning(ses_handle *h, const char *name, int32_t value)
{
    SES_REQUIRE(h && name, "ses_set_tuning: null argument");
    const ses::Knob *k;
    const int rc = ses::tuning_set(h->tune, "ses_set_tuning", name, value, &k);
    if (rc == SES_OK && k->field == &ses::Tuning::comm_p2p_timeout_ms) ses::comm_p2p_set_timeout(h);   // also for a live mailbox
    return rc;
}

int ses_tuning_info(int32_t index, const char **name, int32_t *default_value, int32_t *lo, int32_t *hi)
{
    const ses::Knob *k = ses::tuning_knob(index);
    SES_REQUIRE(k, "ses_tuning_info: no knob %d", index);
    if (name) *name = k->name;
    if (default_value) *default_value = ses::Tuning{}.*(k->field);
    if (lo) *lo = k->lo;
    if (hi) *hi = k->hi;
    return SES_OK;
}

int ses_rollout_plan(const ses_config *cfg, const char *const *knob_names, const int32_t *knob_values, int32_t n_knobs, int32_t n_rows,
                     int32_t mode, struct ses_rollout_plan_info *out)
{
    using namespace ses;
    SES_REQUIRE(cfg && out && n_knobs >= 0 && (n_knobs == 0 || (knob_names && knob_values)), "ses_rollout_plan: null argument");
    const EnvDesc *d;
    int rc = env_check_config("ses_rollout_plan", cfg, &d);
    if (rc != SES_OK) return rc;
    SES_REQUIRE(d, "ses_rollout_plan: SES_ENV_NONE is no env");
    SES_REQUIRE(cfg->eval_ep_num >= 1, "ses_rollout_plan: eval_ep_num must be >= 1");
    SES_REQUIRE(cfg->lanes_per_env >= 0 && cfg->lanes_per_env <= 32 && (cfg->lanes_per_env & (cfg->lanes_per_env - 1)) == 0,
                "ses_rollout_plan: lanes_per_env must be 0, 1, 2, 4, 8, 16 or 32");
    SES_REQUIRE(n_rows >= 1, "ses_rollout_plan: n_rows must be >= 1");
    SES_REQUIRE(mode == SES_MODE_EPISODIC || mode == SES_MODE_FIXED_LENGTH, "ses_rollout_plan: bad mode %d", mode);
    Tuning t;
    for (int i = 0; i < n_knobs; ++i) {
        SES_REQUIRE(knob_names[i], "ses_rollout_plan: null knob name");
        rc = tuning_set(t, "ses_rollout_plan", knob_names[i], knob_values[i]);
        if (rc != SES_OK) return rc;
    }
    const RolloutPlan p = plan_rollout(*cfg, t, ses_param_count(cfg->num_state, cfg->num_action, cfg->gru), n_rows, mode);
    *out = ses_rollout_plan_info{(int32_t)p.family, p.lanes_light, p.lanes_rest, p.waves_light, p.waves_rest, p.handover, p.packed,
                                 p.heavy_packed, p.family == RolloutFamily::CartPoleMlpPure ? p.block : 0, p.own_rows_ok,
                                 p.family == RolloutFamily::Gru ? (int32_t)p.gru_form : 0, p.box2d_lpe, p.box2d_epw};
    return SES_OK;
}

int ses_launch_counts(ses_handle *h, int64_t *pair_rollouts, int64_t *perturb_rollouts, int64_t *apply_perturb)
{
    SES_REQUIRE(h, "ses_launch_counts: null handle");
    if (pair_rollouts) *pair_rollouts = h->count_pair_rollouts;
    if (perturb_rollouts) *perturb_rollouts = h->count_perturb_rollouts;
    if (apply_perturb) *apply_perturb = h->count_apply_perturb;
    return SES_OK;
}

int ses_set_stamp(ses_handle *h, uint64_t *dst)
{
    SES_REQUIRE(h, "ses_set_stamp: null handle");
    h->stamp = (unsigned long long *)dst;
    return SES_OK;
}

int ses_destroy(ses_handle *h)
{
    if (!h) return SES_OK;
    (void)hipSetDevice(h->cfg.device);
    (void)ses::comm_release(h);
    if (h->ep_return) (void)hipFree(h->ep_return);
    if (h->ep_steps) (void)hipFree(h->ep_steps);
    if (h->red_scratch) (void)hipFree(h->red_scratch);
    if (h->gen_init) (void)hipFree(h->gen_init);
    if (h->obs_norm_partials) (void)hipFree(h->obs_norm_partials);
    delete h;
    return SES_OK;
}

int ses_sync(ses_handle *h)
{
    SES_REQUIRE(h, "ses_sync: null handle");
    SES_HIP_TRY(hipStreamSynchronize(h->stream));
    return SES_OK;
}

}  // extern "C"
