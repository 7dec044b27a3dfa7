"""The host side of batched simple_evolution / simple_genetic sweeps, without a device: the per-generation trial records against
the two classes' own evaluate_async (device calls stubbed out), the ragged layout, the closed-form parent maps against the arrays
the classes build, what BatchedRuns accepts and refuses, and how sweep_main.py groups such trials."""
import argparse
import copy
import os

import numpy as np
import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")

BASE = {
    "env": {"name": "CartPole-v1", "max_step": 500, "pomdp": False},
    "network": {"name": "gym_model", "num_state": 4, "num_action": 2, "discrete_action": True, "gru": False},
    "strategy": {"name": "simple_evolution", "init_sigma": 2, "sigma_decay": 0.9999, "elite_num": 10, "offspring_num": 96},
}


def config(**changes):
    cfg = copy.deepcopy(BASE)
    for path, value in changes.items():
        block, key = path.split("__")
        cfg[block][key] = value
    return cfg


# ---- the schedules ------------------------------------------------------------------------------------------------------------

class _NoDevice:
    def rank_center(self, fit, want_weights=True, best=None):
        return None, None

    def elite_mean(self, rows, alias_first=None):
        return None


class _NoRing:
    def arm(self):
        return None

    def push(self):
        return None


def stepped_by_the_class(cls, block, gens):
    """Run the class's own evaluate_async `gens` times with every device call stubbed out: per generation (sigma and key the elite rows
    are rebuilt with, sigma and key the next population is drawn with, the curr_sigma it returns)"""
    s = cls(block["init_sigma"], block["sigma_decay"], block["elite_num"], block["offspring_num"], seed=block["seed"])
    s.dev, s._ring = _NoDevice(), _NoRing()
    s._fitness_tensor = lambda rewards: rewards
    s._set_state = lambda vectors: None
    drawn, rebuilt = [], []

    def offsprings_at(sigma):                         # _materialise's bookkeeping: the population's sigma and key, the key bumped
        drawn.append((sigma, s.gen))
        s._last = {"sigma": sigma, "gen": s.gen}
        s.gen += 1

    def select_elites(rank, k, alias_state=None):     # _select_elites rebuilds the elite rows with the CURRENT population's values
        rebuilt.append((s._last["sigma"], s._last["gen"]))
        return None, None

    s._offsprings_at, s._select_elites = offsprings_at, select_elites
    offsprings_at(s.curr_sigma)                       # init_offspring
    returned = [s.evaluate_async(None)[2] for _ in range(gens)]
    return s, [(rebuilt[g], drawn[g + 1], returned[g]) for g in range(gens)]


@pytest.mark.parametrize("name", ["simple_genetic", "simple_evolution"])
def test_elite_trial_table_reproduces_the_strategy_classes(name):
    from learning_strategies.evolution import offspring_strategies
    from learning_strategies.evolution.batch import EliteSchedule, build_elite_trial_table
    from ses import BatchEliteLayout, _lib
    blocks = [dict(name=name, init_sigma=2, sigma_decay=0.9, elite_num=4, offspring_num=16, seed=3),
              dict(name=name, init_sigma=0.37, sigma_decay=0.9999, elite_num=5, offspring_num=16, seed=(1 << 40) + 1)]
    strategy = _lib.STRATEGY_SIMPLE_GENETIC if name == "simple_genetic" else _lib.STRATEGY_SIMPLE_EVOLUTION
    layout = BatchEliteLayout(strategy, 16, [b["elite_num"] for b in blocks])
    schedules = [EliteSchedule(b) for b in blocks]
    table, sigmas = build_elite_trial_table(schedules, layout, 6)
    assert table.shape == (6, 2) and table.dtype.itemsize == 48
    for r, b in enumerate(blocks):
        s, steps = stepped_by_the_class(getattr(offspring_strategies, name), b, 6)
        for g, ((pop_sigma, gen), (next_sigma, next_gen), curr_sigma) in enumerate(steps):
            row = table[g, r]
            assert int(row["seed"]) == s.seed and int(row["gen"]) == gen == g and int(row["next_gen"]) == next_gen == g + 1
            assert row["pop_sigma"] == np.float32(pop_sigma) and row["pop_sigma"].dtype == np.float32
            assert row["next_sigma"] == np.float32(next_sigma)
            assert sigmas[g][r] == curr_sigma
            assert (int(row["row0"]), int(row["n"]), int(row["elite_num"]), int(row["parent0"])) == (
                int(layout.row0[r]), int(layout.n[r]), b["elite_num"], int(layout.parent0[r]))
        assert schedules[r].curr_sigma == s.curr_sigma and schedules[r].t == s.t == 0
        # genetic redraws with the undecayed sigma and then decays, evolution decays first
        first_next = steps[0][1][0]
        assert first_next == (b["init_sigma"] if name == "simple_genetic" else b["init_sigma"] * b["sigma_decay"])


# ---- the layout -----------------------------------------------------------------------------------------------------------------

def test_layout_of_the_bipedal_genetic_sweep():
    from ses import BatchEliteLayout, _lib
    lay = BatchEliteLayout(_lib.STRATEGY_SIMPLE_GENETIC, 96, (5, 10, 15, 20))
    assert lay.R == 4 and not lay.evolution
    assert tuple(lay.n) == (95, 90, 90, 80) and tuple(lay.row0) == (0, 95, 185, 275) and tuple(lay.parent0) == (0, 5, 15, 30)
    assert tuple(lay.elite_num) == (5, 10, 15, 20)
    assert (lay.rows_total, lay.parents_total, lay.n_max, lay.k_max) == (355, 50, 95, 20)
    for a in (lay.n, lay.row0, lay.parent0, lay.elite_num):
        assert a.dtype == np.int32


def test_layout_of_an_evolution_batch():
    from ses import BatchEliteLayout, _lib
    lay = BatchEliteLayout(_lib.STRATEGY_SIMPLE_EVOLUTION, 96, (2, 4, 97))
    assert lay.evolution and tuple(lay.n) == (97, 97, 97) and tuple(lay.row0) == (0, 97, 194) and tuple(lay.parent0) == (0, 1, 2)
    assert (lay.rows_total, lay.parents_total, lay.n_max, lay.k_max) == (291, 3, 97, 97)


@pytest.mark.parametrize("strategy_name,N,ks,trial", [
    ("STRATEGY_SIMPLE_GENETIC", 96, (5, 0), 1),            # elite_num 0
    ("STRATEGY_SIMPLE_EVOLUTION", 96, (5, 5, 0), 2),
    ("STRATEGY_SIMPLE_GENETIC", 12, (3, 13), 1),           # elite_num > n (a genetic population of 13 > 12 offspring has no rows)
    ("STRATEGY_SIMPLE_EVOLUTION", 12, (14, 3), 0),         # elite_num > n = 13
    ("STRATEGY_SIMPLE_EVOLUTION", 1024, (3, 3), 0),        # 1025 rows
    ("STRATEGY_SIMPLE_GENETIC", 1025, (3, 1), 1),          # 1 * 1025 rows
])
def test_layout_refusals_name_the_trial(strategy_name, N, ks, trial):
    from ses import BatchEliteLayout, SesError, _lib
    with pytest.raises(SesError, match=f"trial {trial} "):
        BatchEliteLayout(getattr(_lib, strategy_name), N, ks)


def test_layout_limits_that_are_accepted():
    from ses import BatchEliteLayout, _lib
    assert BatchEliteLayout(_lib.STRATEGY_SIMPLE_EVOLUTION, 1023, (1, 1024)).n_max == 1024
    assert tuple(BatchEliteLayout(_lib.STRATEGY_SIMPLE_GENETIC, 1025, (2, 1024)).n) == (1024, 1024)
    with pytest.raises(_lib.SesError, match="strategy"):
        BatchEliteLayout(_lib.STRATEGY_OPENAI_ES, 16, (2,))


# ---- the closed-form parent maps ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,k", [(13, 2), (13, 13), (96, 10), (8, 3)])
def test_closed_form_maps_equal_the_classes_arrays(N, k):
    from learning_strategies.evolution.offspring_strategies import simple_evolution, simple_genetic
    from ses import BatchEliteLayout, _lib
    g = simple_genetic(1.0, 0.99, k, N)
    g._materialise = lambda parents, parent_idx_host, sigma: parent_idx_host
    want = g._gen_offsprings(None, None, k, N, 1.0)
    lay = BatchEliteLayout(_lib.STRATEGY_SIMPLE_GENETIC, N, (k, 1))
    got = lay.parent_map(0)
    assert got.dtype == np.int32 and len(got) == lay.n[0] == k * (N // k) == g._population_size()
    assert np.array_equal(got, want)
    e = simple_evolution(1.0, 0.99, k, N)
    want = e._parent_map(True)
    lay = BatchEliteLayout(_lib.STRATEGY_SIMPLE_EVOLUTION, N, (1, k))
    got = lay.parent_map(1)
    assert got.dtype == np.int32 and len(got) == N + 1 == e._population_size()
    assert np.array_equal(got, want)


# ---- check_batchable ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["simple_evolution", "simple_genetic"])
def test_elite_trials_may_differ_in_elite_num_sigmas_and_seeds(name):
    from learning_strategies.evolution.batch import check_batchable
    check_batchable([config(strategy__name=name),
                     config(strategy__name=name, strategy__elite_num=4, strategy__init_sigma=0.5, strategy__sigma_decay=0.999,
                            strategy__seed=4, env__seed=9),
                     config(strategy__name=name, strategy__noise="philox")])


@pytest.mark.parametrize("change,key", [
    (dict(strategy__offspring_num=32), "strategy.offspring_num"),
    (dict(network__gru=True), "network.gru"),
    (dict(strategy__noise="numpy"), "strategy.noise"),
    (dict(strategy__name="simple_genetic"), "strategy.name"),
    (dict(strategy__learning_rate=0.1), "strategy.learning_rate"),       # openai_es's key is not one of theirs
])
def test_elite_batches_refuse_configs_that_differ_elsewhere(change, key):
    from learning_strategies.evolution.batch import BatchedRuns, check_batchable
    configs = [config(), config(strategy__elite_num=3), config(**change)]
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        check_batchable(configs)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        BatchedRuns(configs, 5, 2)


def test_strategies_without_a_batch_are_refused_by_name():
    from learning_strategies.evolution.batch import check_batchable
    with pytest.raises(ValueError, match=r"strategy\.name"):
        check_batchable([config(strategy__name="pgpe"), config(strategy__name="pgpe")])
    with pytest.raises(ValueError, match="trial 1"):                       # a layout refusal surfaces as BatchedRuns' ValueError
        from learning_strategies.evolution.batch import BatchedRuns
        BatchedRuns([config(), config(strategy__elite_num=0)], 5, 2)


# ---- the driver -----------------------------------------------------------------------------------------------------------------------

def resolved_grid():
    import sweep_main
    with open(os.path.join(SRC, "sweep_config", "cartpole_genetic_grid.yaml")) as f:
        spec = yaml.load(f, Loader=yaml.FullLoader)
    args = argparse.Namespace(seed=0, generation_num=1000, eval_ep_num=5)
    out = []
    for point in sweep_main.trial_points(spec, None, None):
        with open(os.path.join(SRC, point["cfg_path"])) as f:
            cfg = yaml.load(f, Loader=yaml.FullLoader)
        cfg, _, generation_num, eval_ep_num = sweep_main.resolve_trial(cfg, point, args)
        out.append((point["cfg_path"], cfg, generation_num, eval_ep_num))
    return out


def test_the_cartpole_genetic_grid_is_grouped():
    import sweep_main
    trials = resolved_grid()
    assert len(trials) == 6
    assert all(sweep_main.batch_key(*t) is None for t in trials), "batch_key keeps its contract: openai_es only"
    keys = [sweep_main.elite_batch_key(*t) for t in trials]
    assert keys[0] == ("conf/cartpole.yaml", "simple_evolution", 96, 20, 5) and len(set(keys)) == 1
    assert sweep_main.group_trials(keys, 6) == [[0, 1, 2, 3, 4, 5]]
    assert sweep_main.group_trials(keys, 4) == [[0, 1, 2, 3], [4, 5]]
    assert sweep_main.group_trials(keys, 1) == [[i] for i in range(6)]
    from learning_strategies.evolution.batch import check_batchable
    check_batchable([t[1] for t in trials])
    assert sorted({t[1]["strategy"]["elite_num"] for t in trials}) == [2, 4]


def test_elite_batch_key_members_and_refusals():
    import sweep_main
    key = sweep_main.elite_batch_key("conf/a.yaml", config(), 30, 5)
    assert key == ("conf/a.yaml", "simple_evolution", 96, 30, 5)
    assert sweep_main.elite_batch_key("conf/a.yaml", config(strategy__elite_num=4), 30, 5) == key
    assert sweep_main.elite_batch_key("conf/a.yaml", config(strategy__name="simple_genetic"), 30, 5) not in (key, None)
    for other in (("conf/b.yaml", config(), 30, 5), ("conf/a.yaml", config(strategy__offspring_num=95), 30, 5),
                  ("conf/a.yaml", config(), 31, 5), ("conf/a.yaml", config(), 30, 4)):
        assert sweep_main.elite_batch_key(*other) not in (key, None)
    assert sweep_main.elite_batch_key("conf/a.yaml", config(strategy__noise="numpy"), 30, 5) is None
    assert sweep_main.elite_batch_key("conf/a.yaml", config(strategy__offspring_num=1024), 30, 5) is None        # 1025 rows
    assert sweep_main.elite_batch_key("conf/a.yaml", config(strategy__offspring_num=1023), 30, 5) is not None
    assert sweep_main.elite_batch_key("conf/a.yaml", config(strategy__name="simple_genetic", strategy__offspring_num=1100,
                                                            strategy__elite_num=1), 30, 5) is None
    assert sweep_main.elite_batch_key("conf/a.yaml", config(strategy__name="openai_es", strategy__learning_rate=0.1), 30, 5) is None
    assert sweep_main.elite_batch_key("conf/a.yaml", config(strategy__name="pgpe"), 30, 5) is None
