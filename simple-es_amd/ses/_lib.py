"""ctypes binding of libses_hip.so (C ABI: include/ses.h).

The library is the product: there is NO CPU fallback.  If it is missing or no MI355X is visible,
everything here raises -- loudly -- instead of computing anything on the host.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SES_LIB_PATH") or os.path.join(os.path.dirname(_HERE), "libses_hip.so")  # env: dev A/B builds

SES_OK = 0
SES_ERR_UNSUPPORTED = -2
RENDER_MAX_PRIMS = 256      # SES_RENDER_MAX_PRIMS
ENV_NONE = -1
ENV_CARTPOLE = 0
ENV_LUNARLANDER = 1
ENV_SIMPLE_SPREAD = 2
ENV_BIPEDALWALKER = 3
ENV_ACROBOT = 4
ENV_MOUNTAINCAR = 5
ENV_PENDULUM = 6
ENV_MOUNTAINCAR_CONT = 7
ENV_WATERWORLD = 8
ENV_INVERTED_PENDULUM = 9
ENV_PENDULUM_SWINGUP = 10
ENV_DOUBLE_PENDULUM = 11
ENV_PURSUIT = 12
ENV_REACHER = 13
ENV_HOPPER = 14
ENV_WALKER2D = 15
ENV_BIPEDALWALKER_HARDCORE = 16
MODE_EPISODIC = 0
MODE_FIXED_LENGTH = 1
HIDDEN = 32


class SesConfig(ctypes.Structure):
    _fields_ = [
        ("env_id", ctypes.c_int32),
        ("num_state", ctypes.c_int32),
        ("num_action", ctypes.c_int32),
        ("discrete_action", ctypes.c_int32),
        ("gru", ctypes.c_int32),
        ("pomdp", ctypes.c_int32),
        ("max_step", ctypes.c_int32),
        ("eval_ep_num", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("lanes_per_env", ctypes.c_int32),
        ("n_agents", ctypes.c_int32),
        ("physics64", ctypes.c_int32),
    ]


class SesEnvInfo(ctypes.Structure):
    """struct ses_env_info of include/ses.h: what the library's env table says about a config's env."""
    _fields_ = [
        ("init_width", ctypes.c_int32), ("obs_width", ctypes.c_int32), ("state_bytes", ctypes.c_int32),
        ("action_layout", ctypes.c_int32), ("agents", ctypes.c_int32), ("num_action", ctypes.c_int32),
        ("has_ep_steps", ctypes.c_int32), ("is_f64", ctypes.c_int32),
        ("init_lo", ctypes.c_double), ("init_hi", ctypes.c_double),
    ]


ACTION_I32_N, ACTION_I32_N_AGENTS, ACTION_F32_N_A, ACTION_F32_N_AGENTS_A = 0, 1, 2, 3      # SES_ACTION_*


class SesRolloutPlanInfo(ctypes.Structure):
    """struct ses_rollout_plan_info of include/ses.h: the launch form ses_rollout chooses (csrc/ses_rollout_plan.h)."""
    _fields_ = [(name, ctypes.c_int32) for name in (
        "family", "lanes_light", "lanes_rest", "waves_light", "waves_rest", "handover", "packed", "heavy_packed", "block",
        "own_rows_ok", "gru_form", "box2d_lpe", "box2d_epw")]


# SES_PLAN_*, SES_GRU_FORM_*
(PLAN_OTHER, PLAN_CARTPOLE_MLP_PURE, PLAN_CARTPOLE_MLP_MIX, PLAN_CARTPOLE_MLP_PAIR, PLAN_CARTPOLE_MLP_F64, PLAN_GRU,
 PLAN_BOX2D_MLP) = range(7)
(GRU_FORM_SEQUENTIAL, GRU_FORM_EPISODE_PARALLEL, GRU_FORM_MFMA4, GRU_FORM_MFMA, GRU_FORM_LOCKSTEP_MULTI4, GRU_FORM_LOCKSTEP_MULTI2,
 GRU_FORM_LOCKSTEP) = range(7)


class SesSepcmaParams(ctypes.Structure):
    """ses_sepcma_params of include/ses.h (ses_sepcma_generation)."""
    _fields_ = [
        ("mu", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("mueff", ctypes.c_double), ("c_sigma", ctypes.c_double), ("d_sigma", ctypes.c_double), ("c_c", ctypes.c_double),
        ("c_1", ctypes.c_double), ("c_mu", ctypes.c_double), ("chi", ctypes.c_double),
        ("scale_lo", ctypes.c_float), ("scale_hi", ctypes.c_float), ("step_lo", ctypes.c_float), ("step_hi", ctypes.c_float),
    ]


class SesLmmaParams(ctypes.Structure):
    """ses_lmma_params of include/ses.h (ses_perturb_lmma, ses_lmma_generation)."""
    _fields_ = [
        ("mu", ctypes.c_int32), ("m", ctypes.c_int32),
        ("mueff", ctypes.c_double), ("c_sigma", ctypes.c_double), ("d_sigma", ctypes.c_double), ("chi", ctypes.c_double),
        ("step_lo", ctypes.c_float), ("step_hi", ctypes.c_float),
        ("cd", ctypes.c_float * 32), ("ad", ctypes.c_float * 32), ("ac", ctypes.c_float * 32), ("bc", ctypes.c_float * 32),
    ]


LMMA_MAX_MEMORY = 32        # SES_LMMA_MAX_MEMORY
LMMA_MAX_P = 16384          # SES_LMMA_MAX_P


class SesMaesParams(ctypes.Structure):
    """ses_maes_params of include/ses.h (ses_maes_generation)."""
    _fields_ = [
        ("mu", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("mueff", ctypes.c_double), ("c_sigma", ctypes.c_double), ("d_sigma", ctypes.c_double), ("chi", ctypes.c_double),
        ("c_1", ctypes.c_double), ("c_mu", ctypes.c_double),
        ("a_m", ctypes.c_float), ("c1h", ctypes.c_float), ("cmuh", ctypes.c_float),
        ("step_lo", ctypes.c_float), ("step_hi", ctypes.c_float),
    ]


MAES_MAX_P = 1024           # SES_MAES_MAX_P


class SesBatchTrial(ctypes.Structure):
    """ses_batch_trial of include/ses.h (ses_openai_generation_batch): one record per trial, 40 bytes."""
    _fields_ = [
        ("seed", ctypes.c_uint64), ("gen", ctypes.c_uint64), ("next_gen", ctypes.c_uint64),
        ("adam_a", ctypes.c_double), ("update_factor", ctypes.c_float), ("next_sigma", ctypes.c_float),
    ]


BATCH_MAX_N = 8192          # rows per trial of ses_openai_generation_batch (the counting rank)
BATCH_MAX_ROWS = 1 << 20    # rows of all its trials together


class SesBatchEliteTrial(ctypes.Structure):
    """ses_batch_elite_trial of include/ses.h (ses_elite_generation_batch): one record per (generation, trial), 48 bytes."""
    _fields_ = [
        ("seed", ctypes.c_uint64), ("gen", ctypes.c_uint64), ("next_gen", ctypes.c_uint64),
        ("pop_sigma", ctypes.c_float), ("next_sigma", ctypes.c_float),
        ("row0", ctypes.c_int32), ("n", ctypes.c_int32), ("elite_num", ctypes.c_int32), ("parent0", ctypes.c_int32),
    ]


BATCH_ELITE_MAX_N = 1024    # rows per trial of ses_elite_generation_batch (one workgroup ranks a trial)


class SesBatchSepcmaTrial(ctypes.Structure):
    """ses_batch_sepcma_trial of include/ses.h (ses_sepcma_generation_batch): one record per (generation, trial), 40 bytes."""
    _fields_ = [
        ("seed", ctypes.c_uint64), ("gen", ctypes.c_uint64), ("next_gen", ctypes.c_uint64),
        ("hsig_scale", ctypes.c_double), ("sigma", ctypes.c_float), ("next_sigma", ctypes.c_float),
    ]


class SesBatchSepcmaConsts(ctypes.Structure):
    """ses_batch_sepcma_consts of include/ses.h (ses_sepcma_generation_batch): one block per trial, 80 bytes."""
    _fields_ = [
        ("hsig_thr", ctypes.c_double), ("cs_over_ds", ctypes.c_double), ("chi", ctypes.c_double),
        ("a_s", ctypes.c_float), ("b_s", ctypes.c_float), ("a_c", ctypes.c_float), ("hb1", ctypes.c_float),
        ("c1f", ctypes.c_float), ("cmuf", ctypes.c_float), ("k0_h1", ctypes.c_float), ("k0_h0", ctypes.c_float),
        ("var_lo", ctypes.c_float), ("var_hi", ctypes.c_float), ("step_lo", ctypes.c_float), ("step_hi", ctypes.c_float),
        ("mu", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


BATCH_SEPCMA_MIN_N = 4      # rows per trial of ses_sepcma_generation_batch: sep_cma_es's own minimum ..
BATCH_SEPCMA_MAX_N = 8192   # .. up to the counting rank's limit; BATCH_MAX_ROWS rows in all


class SesBatchArsTrial(ctypes.Structure):
    """ses_batch_ars_trial of include/ses.h (ses_ars_generation_batch): one record per (generation, trial), 40 bytes."""
    _fields_ = [
        ("seed", ctypes.c_uint64), ("gen", ctypes.c_uint64), ("next_gen", ctypes.c_uint64),
        ("learning_rate", ctypes.c_double), ("next_sigma", ctypes.c_float), ("b", ctypes.c_int32),
    ]


BATCH_ARS_MIN_N = 4         # rows per trial of ses_ars_generation_batch (even): ars's own minimum ..
BATCH_ARS_MAX_N = 16384     # .. up to 8192 pair scores, the counting rank's limit; BATCH_MAX_ROWS rows in all


class SesGenState(ctypes.Structure):
    """ses_gen_state of include/ses.h (ses_run_generations)."""
    _fields_ = [
        ("strategy", ctypes.c_int32), ("n", ctypes.c_int32), ("elite_num", ctypes.c_int32), ("mode", ctypes.c_int32),
        ("shared_init", ctypes.c_int32), ("init_width", ctypes.c_int32),
        ("init_lo", ctypes.c_float), ("init_hi", ctypes.c_float),
        ("seed", ctypes.c_uint64), ("env_seed", ctypes.c_uint64),
        ("learning_rate", ctypes.c_double), ("sigma_decay", ctypes.c_double),
        ("sigma", ctypes.c_double), ("pop_sigma", ctypes.c_double),
        ("pop_gen", ctypes.c_uint64), ("adam_t", ctypes.c_int64),
        ("cur", ctypes.c_int32), ("world", ctypes.c_int32),
        ("theta", ctypes.c_void_p * 2), ("parents", ctypes.c_void_p * 2),
        ("adam_m", ctypes.c_void_p * 2), ("adam_v", ctypes.c_void_p * 2),
        ("parent_map", ctypes.c_void_p), ("alias_state", ctypes.c_void_p),
        ("fitness", ctypes.c_void_p), ("init", ctypes.c_void_p),
        ("work_i32", ctypes.c_void_p), ("work_f32", ctypes.c_void_p),
        ("first_row", ctypes.c_int64), ("n_local", ctypes.c_int32), ("per_rank", ctypes.c_int32),
        ("comm", ctypes.c_void_p), ("fit_local", ctypes.c_void_p),
        ("scale", ctypes.c_void_p * 2),
        ("sigma_learning_rate", ctypes.c_double), ("sigma_max_change", ctypes.c_double),
        ("scale_lo", ctypes.c_float), ("scale_hi", ctypes.c_float),
        ("cma_C", ctypes.c_void_p * 2), ("cma_ps", ctypes.c_void_p * 2), ("cma_pc", ctypes.c_void_p * 2),
        ("cma_step", ctypes.c_void_p * 2), ("cma_weights", ctypes.c_void_p), ("cma", SesSepcmaParams),
        ("lm_ps", ctypes.c_void_p * 2), ("lm_M", ctypes.c_void_p * 2), ("lm_step", ctypes.c_void_p * 2),
        ("lm_weights", ctypes.c_void_p), ("lm", SesLmmaParams),
        ("ma_ps", ctypes.c_void_p * 2), ("ma_M", ctypes.c_void_p * 2), ("ma_step", ctypes.c_void_p * 2),
        ("ma_D", ctypes.c_void_p * 2), ("ma_weights", ctypes.c_void_p), ("ma", SesMaesParams),
        ("ars_b", ctypes.c_int32), ("ars_reserved", ctypes.c_int32),
    ]


STRATEGY_OPENAI_ES, STRATEGY_SIMPLE_EVOLUTION, STRATEGY_SIMPLE_GENETIC, STRATEGY_PGPE, STRATEGY_SEP_CMA_ES = 0, 1, 2, 3, 4
STRATEGY_LM_MA_ES = 5
STRATEGY_MA_ES = 6
STRATEGY_ARS = 7

_vp = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64
_u64 = ctypes.c_uint64
_f32 = ctypes.c_float
_f64 = ctypes.c_double

# name -> argtypes; every entry point declared in include/ses.h (tests/test_abi.py checks the two agree)
SIGNATURES = {
    "ses_create": [ctypes.POINTER(SesConfig), _vp, ctypes.POINTER(_vp)],
    "ses_destroy": [_vp],
    "ses_sync": [_vp],
    "ses_set_tuning": [_vp, ctypes.c_char_p, _i32],
    "ses_tuning_info": [_i32, ctypes.POINTER(ctypes.c_char_p), _vp, _vp, _vp],
    "ses_launch_counts": [_vp, _vp, _vp, _vp],
    "ses_set_stamp": [_vp, _vp],
    "ses_last_error": [],
    "ses_version": [],
    "ses_param_count": [_i32, _i32, _i32],
    "ses_device_count": [],
    "ses_env_info": [ctypes.POINTER(SesConfig), ctypes.POINTER(SesEnvInfo)],
    "ses_rollout_plan": [ctypes.POINTER(SesConfig), ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_int32), _i32, _i32, _i32,
                         ctypes.POINTER(SesRolloutPlanInfo)],
    "ses_perturb": [_vp, _vp, _vp, _vp, _f32, _u64, _u64, _i64, _i32, _vp],
    "ses_noise": [_vp, _u64, _u64, _i64, _i32, _vp],
    "ses_perturb_host_noise": [_vp, _vp, _vp, _vp, _f64, _i32, _vp, _vp],
    "ses_init_states_uniform": [_vp, _u64, _u64, _i64, _i32, _i32, _i32, _f32, _f32, _vp],
    "ses_init_states_uniform_gens": [_vp, _u64, _u64, _i32, _i64, _i32, _i32, _i32, _f32, _f32, _vp],
    "ses_policy_forward": [_vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp],
    "ses_obs_norm_bind": [_vp, _vp, _vp, _i32],
    "ses_obs_norm_merge": [_vp, _vp, _i32, _vp, _vp],
    "ses_env_step": [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "ses_env_state_bytes": [_vp],
    "ses_env_obs_width": [_vp],
    "ses_env_reset": [_vp, _vp, _i32, _vp, _vp],
    "ses_env_step_generic": [_vp, _vp, _vp, _i32, _vp, _vp, _vp],
    "ses_env_step_shape": [_vp, _vp, _vp, _vp, _vp],
    "ses_render_palette": [_vp],
    "ses_render_size": [_vp, _vp, _vp],
    "ses_render_scene": [_vp, _vp, _i32, _vp, _vp],
    "ses_render_frames": [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp],
    "ses_stream_probe": [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "ses_rollout": [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp],
    "ses_rank_center": [_vp, _vp, _i32, _vp, _vp, _vp],
    "ses_es_update_philox": [_vp, _vp, _i32, _i32, _u64, _u64, _f64, _f64, _f64, _vp, _vp, _vp, _vp],
    "ses_openai_generation": [_vp, _vp, _i32, _u64, _u64, _f64, _f64, _f64, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _u64, _i64, _i32,
                              _vp, _vp],
    "ses_openai_sharded_ok": [_vp, _vp, _i32, _i32, _i32],
    "ses_openai_generation_sharded": [_vp, _vp, _vp, _i32, _u64, _u64, _f64, _f64, _f64, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _u64,
                                      _i64, _i32, _i32, _i32, _vp, _vp],
    "ses_openai_generation_batch": [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "ses_elite_generation_batch": [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp],
    "ses_es_update_stored": [_vp, _vp, _i32, _vp, _f64, _f64, _f64, _vp, _vp, _vp, _vp],
    "ses_perturb_mirrored": [_vp, _vp, _vp, _f32, _u64, _u64, _i64, _i32, _vp],
    "ses_pgpe_generation": [_vp, _vp, _i32, _u64, _u64, _f64, _f64, _f64, _f64, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                            _f32, _u64, _i64, _i32, _vp, _vp, _vp, _vp],
    "ses_perturb_sepcma": [_vp, _vp, _vp, _vp, _f32, _u64, _u64, _i64, _i32, _vp],
    "ses_sepcma_generation": [_vp, _vp, _i32, _u64, _u64, _f64, _f64, ctypes.POINTER(SesSepcmaParams), _vp, _vp, _vp, _vp, _vp, _vp,
                              _vp, _vp, _vp, _vp, _vp, _f32, _u64, _i64, _i32, _vp, _vp, _vp, _vp, _vp],
    "ses_sepcma_generation_batch": [_vp, _vp, _i32, _i32, ctypes.POINTER(ctypes.c_int32), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "ses_perturb_lmma": [_vp, _vp, _vp, _vp, ctypes.POINTER(SesLmmaParams), _i32, _f32, _u64, _u64, _i64, _i32, _vp, _vp],
    "ses_lmma_generation": [_vp, _vp, _i32, _u64, _u64, _f64, ctypes.POINTER(SesLmmaParams), _vp, _i32, _i32, _vp, _vp, _vp, _vp,
                            _vp, _vp, _vp, _vp, _f32, _u64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "ses_perturb_maes": [_vp, _vp, _vp, _vp, _f32, _u64, _u64, _i64, _i32, _vp, _vp],
    "ses_maes_generation": [_vp, _vp, _i32, _u64, _u64, _f64, ctypes.POINTER(SesMaesParams), _vp, _vp, _vp, _vp, _vp, _vp,
                            _vp, _vp, _vp, _vp, _f32, _u64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "ses_ars_generation": [_vp, _vp, _i32, _i32, _u64, _u64, _f64, _f64, _vp, _vp, _f32, _u64, _i64, _i32, _vp, _vp, _vp, _vp],
    "ses_ars_generation_batch": [_vp, _vp, _i32, _i32, ctypes.POINTER(ctypes.c_int32), _vp, _vp, _vp, _vp, _vp, _vp, _vp],
    "ses_elite_ids": [_vp, _vp, _i32, _i32, _vp],
    "ses_elite_select": [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp],
    "ses_elite_mean": [_vp, _vp, _vp, _i32, _vp],
    "ses_gather_rows": [_vp, _vp, _vp, _i32, _vp],
    "ses_run_generations": [_vp, ctypes.POINTER(SesGenState), _i32, _vp, _vp],
    "ses_comm_unique_id": [_vp],
    "ses_comm_init": [_vp, _i32, _i32, _vp],
    "ses_comm_info": [_vp, _vp, _vp, _vp],
    "ses_comm_destroy": [_vp],
    "ses_allgather_fitness": [_vp, _vp, _i32, _vp],
    "ses_comm_p2p_export": [_vp, _i32, _i32, _i32, _vp],
    "ses_comm_p2p_attach": [_vp, _vp],
    "ses_comm_p2p_attach_local": [_vp, _vp],
    "ses_stream_create_exclusive": [_i32, _vp],
    "ses_stream_destroy": [_vp],
    "ses_comm_p2p_info": [_vp, _vp, _vp, _vp],
    "ses_comm_p2p_counts": [_vp, _vp, _vp],
    "ses_comm_p2p_status": [_vp, _vp],
    "ses_comm_p2p_reset_status": [_vp],
    "ses_comm_p2p_detach": [_vp],
}
COMM_ID_BYTES = 128
COMM_P2P_HANDLE_BYTES = 64
_RESTYPE = {"ses_last_error": ctypes.c_char_p, "ses_version": ctypes.c_char_p}

_lib = None


class SesError(RuntimeError):
    pass


def load():
    """dlopen libses_hip.so; raises if it has not been built (python __graft_entry__.py / csrc/build.sh)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SesError(f"{LIB_PATH} not found: build it with simple-es_amd/csrc/build.sh "
                       f"(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here == ABI drift; let it surface
        fn.argtypes = argtypes
        fn.restype = _RESTYPE.get(name, ctypes.c_int)
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != SES_OK:
        msg = load().ses_last_error().decode("utf-8", "replace")
        raise SesError(f"{what or 'libses_hip'} failed (code {rc}): {msg}")
    return rc


def env_info(env_id, num_state, num_action, discrete_action, gru=False, pomdp=False, eval_ep_num=1, n_agents=1, physics64=False):
    """ses_env_info: the SesEnvInfo of this config's env.  Needs no device; a config the env refuses raises with the library's message."""
    cfg = SesConfig(int(env_id), int(num_state), int(num_action), int(bool(discrete_action)), int(bool(gru)), int(bool(pomdp)), 1,
                    int(eval_ep_num), 0, 0, int(n_agents), int(bool(physics64)))
    info = SesEnvInfo()
    check(load().ses_env_info(ctypes.byref(cfg), ctypes.byref(info)), "ses_env_info")
    return info


def tuning_info():
    """ses_tuning_info, every row: [(name, default, lo, hi)] of the knobs ses_set_tuning knows.  Needs no device."""
    lib, rows = load(), []
    name, default, lo, hi = ctypes.c_char_p(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    while lib.ses_tuning_info(len(rows), ctypes.byref(name), ctypes.byref(default), ctypes.byref(lo), ctypes.byref(hi)) == SES_OK:
        rows.append((name.value.decode(), default.value, lo.value, hi.value))
    return rows


def rollout_plan(cfg, n_rows, mode, **knobs):
    """ses_rollout_plan: the SesRolloutPlanInfo of a rollout of n_rows offspring of the SesConfig `cfg` under `mode`, the knobs at
    their defaults except those given.  Needs no device; a refused config, knob or argument raises with the library's message."""
    names = (ctypes.c_char_p * len(knobs))(*[k.encode() for k in knobs])
    values = (ctypes.c_int32 * len(knobs))(*[int(v) for v in knobs.values()])
    info = SesRolloutPlanInfo()
    check(load().ses_rollout_plan(ctypes.byref(cfg), names, values, len(knobs), int(n_rows), int(mode), ctypes.byref(info)),
          "ses_rollout_plan")
    return info
