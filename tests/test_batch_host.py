"""The host side of batched sweeps, without a device: how sweep_main.py groups trials, what BatchedRuns refuses, and the
per-generation trial records against an openai_es object and its Adam stepped by hand."""
import copy

import numpy as np
import pytest
import torch

BASE = {
    "env": {"name": "CartPole-v1", "max_step": 500, "pomdp": False},
    "network": {"name": "gym_model", "num_state": 4, "num_action": 2, "discrete_action": True, "gru": False},
    "strategy": {"name": "openai_es", "init_sigma": 0.1, "sigma_decay": 0.999, "learning_rate": 0.05, "offspring_num": 64},
}


def config(**changes):
    cfg = copy.deepcopy(BASE)
    for path, value in changes.items():
        block, key = path.split("__")
        cfg[block][key] = value
    return cfg


def test_grouping_of_a_mixed_sweep():
    import sweep_main
    cfgs = [config(), config(strategy__init_sigma=0.3), config(strategy__learning_rate=0.1),
            config(strategy__name="simple_evolution", strategy__elite_num=4),
            config(), config(strategy__offspring_num=32), config(strategy__offspring_num=32), config()]
    keys = [sweep_main.batch_key("conf/a.yaml", c, 30, 5) for c in cfgs]
    assert keys[3] is None and keys[0] == keys[1] == keys[2] == keys[4] == keys[7] and keys[5] == keys[6] != keys[0]
    groups = sweep_main.group_trials(keys, 4)
    assert groups == [[0, 1, 2], [3], [4], [5, 6], [7]]
    assert sweep_main.group_trials(keys, 2) == [[0, 1], [2], [3], [4], [5, 6], [7]]
    for concurrent in (1, 2, 3, 4, 16):
        got = sweep_main.group_trials(keys, concurrent)
        assert [i for g in got for i in g] == list(range(len(keys)))
        assert all(len(g) <= concurrent for g in got)
        assert all(keys[i] == keys[g[0]] and keys[i] is not None for g in got if len(g) > 1 for i in g)
    assert sweep_main.group_trials(keys, 1) == [[i] for i in range(len(keys))]
    # the other members of the key: config file, generations, episodes
    assert sweep_main.batch_key("conf/b.yaml", cfgs[0], 30, 5) != keys[0]
    assert sweep_main.batch_key("conf/a.yaml", cfgs[0], 31, 5) != keys[0]
    assert sweep_main.batch_key("conf/a.yaml", cfgs[0], 30, 4) != keys[0]
    assert sweep_main.batch_key("conf/a.yaml", config(strategy__noise="numpy"), 30, 5) is None


@pytest.mark.parametrize("change,key", [
    (dict(env__max_step=200), "env.max_step"),
    (dict(env__name="CartPole-v0"), "env.name"),
    (dict(network__gru=True), "network.gru"),
    (dict(strategy__offspring_num=32), "strategy.offspring_num"),
    (dict(strategy__name="simple_evolution"), "strategy.name"),
    (dict(strategy__noise="numpy"), "strategy.noise"),
])
def test_batched_runs_refuses_configs_that_differ_elsewhere(change, key):
    from learning_strategies.evolution.batch import BatchedRuns
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        BatchedRuns([config(), config(strategy__seed=1), config(**change)], 5, 2)


def test_what_may_differ_is_accepted_by_the_check():
    from learning_strategies.evolution.batch import check_batchable
    check_batchable([config(), config(strategy__init_sigma=0.3, strategy__sigma_decay=0.99, strategy__learning_rate=0.2, strategy__seed=4,
                                      env__seed=9), config(strategy__noise="philox")])


def test_trial_table_reproduces_openai_es_and_its_adam():
    from learning_strategies.evolution.batch import TrialSchedule, build_trial_table
    from learning_strategies.evolution.offspring_strategies import openai_es
    from learning_strategies.optimizers import Adam
    blocks = [dict(BASE["strategy"], seed=3), dict(BASE["strategy"], init_sigma=0.37, sigma_decay=0.9, learning_rate=0.013, seed=(1 << 40) + 1)]
    table, sigmas = build_trial_table([TrialSchedule(b) for b in blocks], 5)
    assert table.shape == (5, 2) and table.dtype.itemsize == 40
    for r, b in enumerate(blocks):
        s = openai_es(b["init_sigma"], b["sigma_decay"], b["learning_rate"], b["offspring_num"], seed=b["seed"])
        s.optimizer = Adam(torch.zeros(1), s.learning_rate)
        gen = 0                                       # the initial population's key (_population bumps it per population)
        for g in range(5):
            # openai_es._generation and ses_openai_generation's host expressions (csrc/ses_strategy.hip: openai_generation_impl)
            a = s.optimizer.next_step_scale()
            sigma = s.curr_sigma
            s.curr_sigma *= s.sigma_decay
            uf = s.learning_rate / (float(s.offspring_num) * sigma)
            uf *= -1.0
            row = table[g, r]
            assert int(row["seed"]) == s.seed and int(row["gen"]) == gen and int(row["next_gen"]) == gen + 1
            assert float(row["adam_a"]) == a
            assert row["update_factor"] == np.float32(uf) and row["update_factor"].dtype == np.float32
            assert row["next_sigma"] == np.float32(s.curr_sigma)
            assert sigmas[g][r] == s.curr_sigma
            gen += 1
        assert s.optimizer.t == 5
