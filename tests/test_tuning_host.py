"""The tuning knobs are defined once, in the table of csrc/ses_tuning.h.  No device: ses_tuning_info walks the table, and the
overrides of ses_rollout_plan go through the validator ses_set_tuning uses.  The literals below were copied from the ses_create
and the ses_set_tuning of the commit before the table existed: the table must say what those said."""
import os
import re

import pytest

from ses import _lib
from ses._lib import SesConfig, SesError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ses_create's explicit assignments; 0 where it left the field to its memset
DEFAULTS = {
    "rollout_block": 64, "gru_mfma_min_e": 12, "gru_mfma4_min_e": 7, "gru_ep_parallel_max": 4096, "gru_sequential": 0,
    "rollout_mix": 1, "rollout_waves8": 1024, "rollout_packed": -1, "rollout_heavy_packed": -1, "rollout_mix_8_16": 1,
    "rollout_handover_step": 1 << 30, "rollout_heavy_prio_steps": 1 << 30, "lander_offspring_per_wave": 0,
    "box2d_lanes_per_env": 0, "box2d_envs_per_wave": 0, "env_step_block": 64, "env_step_lds_bytes": -1, "env_step_waves_per_cu": 7,
    "openai_sharded_tail": 1, "openai_sharded_min_rows": 8192, "openai_granule_exchange": 1, "comm_granules_enabled": 1,
    "fused_fitness_exchange": 1, "fused_episode_mean": 1, "fused_elite_tail": 1, "fused_apply_perturb": 1,
    "fused_perturb_rollout": 1, "pgpe_fused_apply_perturb": 1, "ars_fused_apply_perturb": 1, "spread_gru_wave_per_batch": -1,
    "waterworld_fc1_mfma": -1, "pursuit_fc1_mfma": -1, "pendula_generic_step": -1, "reacher_generic_step": -1,
    "comm_granule_allgather": 0, "es_final_max_chunks": 0, "es_tail_wide": 1,
    "pendulum_generic_step": 0, "rollout_mix_light": 0, "rollout_lpe32_max_envs": 0, "comm_force_rccl": 0,
    "comm_p2p_timeout_ms": 0, "comm_p2p_keep_going": 0,
}
# ses_set_tuning's knobs[]
RANGES = {
    "rollout_block": (64, 256), "gru_mfma_min_e": (1, 1 << 30), "gru_mfma4_min_e": (0, 8), "gru_ep_parallel_max": (0, 1 << 30),
    "gru_sequential": (0, 1), "rollout_mix": (0, 1), "rollout_waves8": (1, 1 << 20), "rollout_mix_light": (0, 16),
    "rollout_lpe32_max_envs": (0, 1 << 30), "rollout_packed": (-1, 1), "rollout_heavy_packed": (-1, 1), "rollout_mix_8_16": (0, 1),
    "rollout_handover_step": (0, 1 << 30), "rollout_heavy_prio_steps": (0, 1 << 30), "lander_offspring_per_wave": (0, 4),
    "box2d_lanes_per_env": (0, 64), "box2d_envs_per_wave": (0, 64), "pendulum_generic_step": (0, 1),
    "pendula_generic_step": (-1, 1), "reacher_generic_step": (-1, 1), "env_step_block": (64, 256),
    "env_step_lds_bytes": (-1, 65536), "env_step_waves_per_cu": (1, 32), "es_final_max_chunks": (0, 1 << 20),
    "es_tail_wide": (0, 1), "comm_force_rccl": (0, 1), "comm_p2p_timeout_ms": (0, 1 << 30), "comm_p2p_keep_going": (0, 1),
    "openai_sharded_tail": (0, 1), "openai_sharded_min_rows": (0, 1 << 30), "openai_granule_exchange": (0, 1),
    "comm_granule_allgather": (0, 1), "comm_granules_enabled": (0, 1), "fused_fitness_exchange": (0, 1),
    "fused_episode_mean": (0, 1), "fused_elite_tail": (0, 1), "fused_apply_perturb": (0, 1), "fused_perturb_rollout": (0, 1),
    "pgpe_fused_apply_perturb": (0, 1), "ars_fused_apply_perturb": (0, 1), "spread_gru_wave_per_batch": (-1, 1),
    "waterworld_fc1_mfma": (-1, 1), "pursuit_fc1_mfma": (-1, 1),
}
# the only values allowed where the range says too much
VALUE_LISTS = {
    "rollout_block": (64, 256), "env_step_block": (64, 128, 256), "lander_offspring_per_wave": (0, 1, 2, 4),
    "box2d_lanes_per_env": (0, 1, 2, 4, 8, 16, 32, 64), "rollout_mix_light": (0, 8, 16),
}
CARTPOLE = SesConfig(_lib.ENV_CARTPOLE, 4, 2, 1, 0, 0, 500, 5, 0, 0, 1, 0)


def plan(**knobs):
    return _lib.rollout_plan(CARTPOLE, 96, _lib.MODE_EPISODIC, **knobs)


@pytest.fixture(scope="module")
def table():
    return _lib.tuning_info()


def test_the_table_has_43_knobs_with_unique_names(table):
    names = [name for name, _, _, _ in table]
    assert len(names) == 43 and len(set(names)) == 43
    assert len(DEFAULTS) == 43 and len(RANGES) == 43


def test_defaults_are_what_ses_create_set(table):
    assert {name: default for name, default, _, _ in table} == DEFAULTS


def test_ranges_are_what_ses_set_tuning_checked(table):
    assert {name: (lo, hi) for name, _, lo, hi in table} == RANGES


def test_header_comment_and_table_name_the_same_knobs(table):
    header = open(os.path.join(ROOT, "include", "ses.h")).read()
    end = header.index("int ses_set_tuning(")
    comment = header[header.rindex("/*", 0, end):end]
    assert comment.rstrip().endswith("*/") and comment.count("/*") == 1
    quoted = set(re.findall(r'"([a-z][a-z0-9_]*)"', comment))
    assert quoted == {name for name, _, _, _ in table}


def test_every_knob_refuses_outside_its_range_and_takes_its_ends(table):
    for name, _, lo, hi in table:
        for value in (lo - 1, hi + 1):
            with pytest.raises(SesError, match=rf"{name} = {value} outside \[{lo}, {hi}\]"):
                plan(**{name: value})
        for value in (lo, hi):
            if value in VALUE_LISTS.get(name, (value,)):
                plan(**{name: value})


@pytest.mark.parametrize("name, off_list", [("rollout_block", 128), ("env_step_block", 96), ("lander_offspring_per_wave", 3),
                                            ("box2d_lanes_per_env", 24), ("rollout_mix_light", 4)])
def test_value_lists_refuse_a_value_off_the_list(name, off_list):
    lo, hi = RANGES[name]
    assert lo < off_list < hi and off_list not in VALUE_LISTS[name]
    with pytest.raises(SesError, match=rf"{name} must be "):
        plan(**{name: off_list})
    for value in VALUE_LISTS[name]:
        plan(**{name: value})


def test_an_unknown_name_is_refused():
    with pytest.raises(SesError, match="unknown knob 'rollout_blok'"):
        plan(rollout_blok=64)
