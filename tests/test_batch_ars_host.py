"""The host side of batched ars sweeps, without a device: what BatchedRuns accepts and refuses for the strategy, the per-generation
trial records against an ars object's own host scalars, how sweep_main.py groups such trials, and the ctypes struct against
include/ses.h."""
import argparse
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")

BASE = {
    "env": {"name": "CartPole-v1", "max_step": 500, "pomdp": False},
    "network": {"name": "gym_model", "num_state": 4, "num_action": 2, "discrete_action": True, "gru": False},
    "strategy": {"name": "ars", "init_sigma": 0.1, "sigma_decay": 1.0, "learning_rate": 0.2, "offspring_num": 64},
}


def config(**changes):
    cfg = copy.deepcopy(BASE)
    for path, value in changes.items():
        block, key = path.split("__")
        cfg[block][key] = value
    return cfg


# ---- check_batchable ------------------------------------------------------------------------------------------------------------------

def test_ars_trials_may_differ_in_every_allowed_key():
    from learning_strategies.evolution.batch import ARS_VARYING, BATCHED_STRATEGIES, check_batchable
    assert "ars" in BATCHED_STRATEGIES
    assert ARS_VARYING == {"strategy": ("init_sigma", "sigma_decay", "learning_rate", "elite_num", "seed"), "env": ("seed",)}
    for block, keys in ARS_VARYING.items():                               # each key on its own, then all of them at once
        for key, value in zip(keys, (0.3, 0.97, 0.05, 5, 4)):
            check_batchable([config(), config(**{f"{block}__{key}": value})])
    check_batchable([config(),
                     config(strategy__init_sigma=0.3, strategy__sigma_decay=0.97, strategy__learning_rate=0.05, strategy__elite_num=5,
                            strategy__seed=4, env__seed=9),
                     config(strategy__noise="philox", strategy__elite_num=32)])


@pytest.mark.parametrize("change,key", [
    (dict(strategy__offspring_num=32), "strategy.offspring_num"),
    (dict(network__gru=True), "network.gru"),
    (dict(env__name="CartPole-v0"), "env.name"),
    (dict(strategy__noise="numpy"), "strategy.noise"),
    (dict(strategy__scale_limits=[0.5, 2.0]), "strategy.scale_limits"),    # sep_cma_es's key is not one of ars's
])
def test_ars_batches_refuse_configs_that_differ_elsewhere(change, key):
    from learning_strategies.evolution.batch import BatchedRuns, check_batchable
    configs = [config(), config(strategy__elite_num=3), config(**change)]
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        check_batchable(configs)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        BatchedRuns(configs, 5, 2)


def test_ars_batches_draw_philox_noise():
    from learning_strategies.evolution.batch import check_batchable
    with pytest.raises(ValueError, match=r"strategy\.noise"):
        check_batchable([config(strategy__noise="numpy"), config(strategy__noise="numpy")])


def test_pgpe_stays_sequential_next_to_ars():
    from learning_strategies.evolution.batch import check_batchable
    with pytest.raises(ValueError, match=r"strategy\.name"):
        check_batchable([config(strategy__name="pgpe"), config(strategy__name="pgpe")])
    with pytest.raises(ValueError, match=r"strategy\.name"):
        check_batchable([config(), config(strategy__name="pgpe")])


@pytest.mark.parametrize("strategy", [BASE["strategy"],
                                      {"name": "openai_es", "init_sigma": 0.1, "sigma_decay": 1.0, "learning_rate": 0.1, "offspring_num": 64},
                                      {"name": "sep_cma_es", "init_sigma": 0.5, "sigma_decay": 1.0, "offspring_num": 64}],
                         ids=["ars", "openai_es", "sep_cma_es"])
def test_an_observation_normaliser_is_refused_for_every_strategy(strategy):
    from learning_strategies.evolution.batch import BatchedRuns, check_batchable
    plain = dict(config(), strategy=dict(strategy))
    check_batchable([plain, copy.deepcopy(plain)])
    check_batchable([dict(plain, network=dict(plain["network"], obs_normalizer=False))] * 2)
    normalised = dict(plain, network=dict(plain["network"], obs_normalizer=True))
    for configs in ([normalised, copy.deepcopy(normalised)], [plain, normalised]):
        with pytest.raises(ValueError, match=r"obs_normalizer.*cannot share R normalisers"):
            check_batchable(configs)
        with pytest.raises(ValueError, match=r"obs_normalizer"):
            BatchedRuns(configs, 5, 2)


@pytest.mark.parametrize("n", [2, 16386])
def test_batched_runs_refuses_populations_outside_the_counting_rank(n):
    from learning_strategies.evolution.batch import BatchedRuns
    with pytest.raises(ValueError, match="offspring_num"):
        BatchedRuns([config(strategy__offspring_num=n, strategy__elite_num=1)] * 2, 5, 2)


# ---- the schedule ---------------------------------------------------------------------------------------------------------------------

def test_trial_table_reproduces_an_ars_objects_host_scalars():
    """ArsSchedule against the class's own _generation, the device call stubbed out: it records what the call is given.  Four
    generations; sigma_decay 1.0 and 0.97."""
    from learning_strategies.evolution.batch import ARS_TRIAL_DTYPE, ArsSchedule, build_ars_trial_table
    from learning_strategies.evolution.offspring_strategies import ars
    G = 4
    blocks = [dict(BASE["strategy"], seed=3),                                                     # sigma_decay 1.0, elite_num defaulted
              dict(BASE["strategy"], init_sigma=0.37, sigma_decay=0.97, learning_rate=0.05, elite_num=5, seed=(1 << 40) + 1),
              dict(BASE["strategy"], init_sigma=2, sigma_decay=0.97, learning_rate=1, elite_num=32)]
    schedules = [ArsSchedule(b) for b in blocks]
    assert [s.elite_num for s in schedules] == [16, 5, 32]                # the default: max(1, n // 4)
    table, sigmas = build_ars_trial_table(schedules, G)
    assert table.shape == (G, 3) and table.dtype == ARS_TRIAL_DTYPE and table.dtype.itemsize == 40

    class Recorder:
        def ars_generation(self, fit, b, seed, gen, sigma, learning_rate, state_in, state_out, next_sigma, next_gen, first_row, n_rows,
                           best=None):
            self.got = (b, seed, gen, sigma, learning_rate, next_sigma, next_gen)

    class Shard:
        first, n_local = 0, 64

    for r, blk in enumerate(blocks):
        s = ars(blk["init_sigma"], blk["sigma_decay"], blk["learning_rate"], blk["offspring_num"],
                **{k: blk[k] for k in ("elite_num", "seed") if k in blk})
        s.dev = Recorder()
        s.gen = 1                                     # the initial population took key 0 (_population bumps it per population)
        for g in range(G):
            s._last = {"gen": s.gen - 1}
            s._generation(None, None, None, Shard, None)
            b, seed, gen, sigma, lr, next_sigma, next_gen = s.dev.got
            s.gen += 1
            row = table[g, r]
            assert int(row["seed"]) == seed == s.seed and int(row["gen"]) == gen == g and int(row["next_gen"]) == next_gen == g + 1
            assert float(row["learning_rate"]) == float(lr) and row["learning_rate"].dtype == np.float64
            assert int(row["b"]) == b == s.elite_num and row["b"].dtype == np.int32
            assert row["next_sigma"] == np.float32(next_sigma) and row["next_sigma"].dtype == np.float32
            assert next_sigma == s.curr_sigma == sigma * blk["sigma_decay"]
            assert sigmas[g][r] == s.curr_sigma
        assert schedules[r].curr_sigma == s.curr_sigma and schedules[r].gen == s.gen == G + 1 and schedules[r].t == 0
    assert all(sig[0] == 0.1 for sig in sigmas), "sigma_decay 1.0 leaves curr_sigma alone"
    assert sigmas[3][1] != sigmas[2][1] and sigmas[3][1] == 0.37 * 0.97 * 0.97 * 0.97 * 0.97


def test_the_schedule_refuses_what_the_class_refuses():
    from learning_strategies.evolution.batch import ArsSchedule
    for key, bad in (("elite_num", 0), ("elite_num", 33), ("offspring_num", 63), ("offspring_num", 2), ("noise", "numpy")):
        with pytest.raises(ValueError):
            ArsSchedule(dict(BASE["strategy"], **{key: bad}))


# ---- the driver -----------------------------------------------------------------------------------------------------------------------

def resolved_grid():
    import sweep_main
    with open(os.path.join(SRC, "sweep_config", "cartpole_ars_grid.yaml")) as f:
        spec = yaml.load(f, Loader=yaml.FullLoader)
    args = argparse.Namespace(seed=0, generation_num=1000, eval_ep_num=5)
    out = []
    for point in sweep_main.trial_points(spec, None, None):
        with open(os.path.join(SRC, point["cfg_path"])) as f:
            cfg = yaml.load(f, Loader=yaml.FullLoader)
        cfg, _, generation_num, eval_ep_num = sweep_main.resolve_trial(cfg, point, args)
        out.append((point["cfg_path"], cfg, generation_num, eval_ep_num))
    return out


def test_the_cartpole_ars_grid_is_grouped():
    import sweep_main
    from learning_strategies.evolution.batch import check_batchable
    trials = resolved_grid()
    assert len(trials) == 16
    assert all(sweep_main.batch_key(*t) is None and sweep_main.elite_batch_key(*t) is None and sweep_main.sepcma_batch_key(*t) is None
               for t in trials), "the three earlier keys keep their contracts"
    keys = [sweep_main.ars_batch_key(*t) for t in trials]
    assert keys[0] == ("conf/cartpole_ars.yaml", "ars", 256, 20, 5) and len(set(keys)) == 1
    assert sweep_main.group_trials(keys, 16) == [list(range(16))]
    assert sweep_main.group_trials(keys, 6) == [[0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10, 11], [12, 13, 14, 15]]
    assert sweep_main.group_trials(keys, 1) == [[i] for i in range(16)]
    check_batchable([t[1] for t in trials])
    # the grid's two axes reach the configs: the sweep's values override the config file's
    assert sorted({t[1]["strategy"]["elite_num"] for t in trials}) == [8, 32, 64, 128]
    assert sorted({t[1]["strategy"]["learning_rate"] for t in trials}) == [0.05, 0.1, 0.2, 0.4]
    assert len({(t[1]["strategy"]["elite_num"], t[1]["strategy"]["learning_rate"]) for t in trials}) == 16


def test_ars_batch_key_members_and_refusals():
    import sweep_main
    key = sweep_main.ars_batch_key("conf/a.yaml", config(), 30, 5)
    assert key == ("conf/a.yaml", "ars", 64, 30, 5)
    assert sweep_main.ars_batch_key("conf/a.yaml", config(strategy__elite_num=4, strategy__learning_rate=2.0), 30, 5) == key
    for other in (("conf/b.yaml", config(), 30, 5), ("conf/a.yaml", config(strategy__offspring_num=62), 30, 5),
                  ("conf/a.yaml", config(), 31, 5), ("conf/a.yaml", config(), 30, 4)):
        assert sweep_main.ars_batch_key(*other) not in (key, None)
    assert sweep_main.ars_batch_key("conf/a.yaml", config(strategy__noise="numpy"), 30, 5) is None
    assert sweep_main.ars_batch_key("conf/a.yaml", config(strategy__offspring_num=63), 30, 5) is None       # odd
    assert sweep_main.ars_batch_key("conf/a.yaml", config(strategy__offspring_num=2), 30, 5) is None
    assert sweep_main.ars_batch_key("conf/a.yaml", config(strategy__offspring_num=4), 30, 5) is not None
    assert sweep_main.ars_batch_key("conf/a.yaml", config(strategy__offspring_num=16384), 30, 5) is not None
    assert sweep_main.ars_batch_key("conf/a.yaml", config(strategy__offspring_num=16386), 30, 5) is None
    for name in ("pgpe", "lm_ma_es", "ma_es", "openai_es", "simple_evolution", "sep_cma_es"):
        assert sweep_main.ars_batch_key("conf/a.yaml", config(strategy__name=name), 30, 5) is None
    # consecutive equal keys group; a key of None (odd n, n = 16386) runs alone
    cfgs = [config(), config(strategy__elite_num=2), config(strategy__offspring_num=63), config(strategy__offspring_num=16386), config(),
            config(strategy__learning_rate=1.0)]
    keys = [sweep_main.ars_batch_key("conf/a.yaml", c, 30, 5) for c in cfgs]
    assert keys[2] is None and keys[3] is None
    assert sweep_main.group_trials(keys, 4) == [[0, 1], [2], [3], [4, 5]]


def test_main_groups_ars_trials_and_keeps_normalised_ones_alone(tmp_path, monkeypatch):
    """main() consults ars_batch_key: the grid's 16 trials go out in batches; with network.obs_normalizer they stay alone.  run_trial
    and run_batch are replaced by recorders, no device is touched."""
    import sys
    import sweep_main
    record = {"ep5_mean_reward": 0.0, "best_reward": 0.0, "generations": 0, "log_dir": None}
    calls = []
    monkeypatch.setattr(sweep_main, "run_trial", lambda config, point, args: calls.append(1) or dict(record))
    monkeypatch.setattr(sweep_main, "run_batch", lambda configs, g, e: calls.append(len(configs)) or [dict(record) for _ in configs])
    with open(os.path.join(SRC, "sweep_config", "cartpole_ars_grid.yaml")) as f:
        spec = yaml.load(f, Loader=yaml.FullLoader)
    with open(os.path.join(SRC, spec["parameters"]["cfg-path"]["value"])) as f:
        cfg = yaml.load(f, Loader=yaml.FullLoader)
    monkeypatch.chdir(tmp_path)
    for normalised, want in ((False, [6, 6, 4]), (True, [1] * 16)):
        cfg["network"]["obs_normalizer"] = normalised
        (tmp_path / f"cfg{normalised}.yaml").write_text(yaml.safe_dump(cfg))
        spec["parameters"]["cfg-path"]["value"] = str(tmp_path / f"cfg{normalised}.yaml")
        sweep = tmp_path / f"grid{normalised}.yaml"
        sweep.write_text(yaml.safe_dump(spec))
        calls.clear()
        monkeypatch.setattr(sys, "argv", ["sweep_main.py", "--sweep", str(sweep), "--concurrent", "6"])
        sweep_main.main()
        assert calls == want, (normalised, calls)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------

C_TYPES = {"uint64_t": ctypes.c_uint64, "int32_t": ctypes.c_int32, "double": ctypes.c_double, "float": ctypes.c_float}


def header_struct(name):
    """[(field, ctypes type)] of `typedef struct name { ... } name;` in include/ses.h, and the size its comment states"""
    text = open(os.path.join(ROOT, "include", "ses.h")).read()
    m = re.search(r"typedef struct " + name + r" \{ /\* (\d+) bytes \*/(.*?)\} " + name + ";", text, flags=re.S)
    assert m, name
    body = re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(f.strip(), C_TYPES[typ]) for f in names.split(",")]
    return fields, int(m.group(1))


def test_ctypes_struct_equals_the_header():
    from learning_strategies.evolution.batch import ARS_TRIAL_DTYPE
    from ses import _lib
    fields, stated = header_struct("ses_batch_ars_trial")
    cls = _lib.SesBatchArsTrial
    assert list(cls._fields_) == fields

    class FromHeader(ctypes.Structure):
        _fields_ = fields

    assert ctypes.sizeof(cls) == ctypes.sizeof(FromHeader) == stated == 40
    dt = np.dtype(cls)
    assert dt.itemsize == 40 and dt == ARS_TRIAL_DTYPE                   # 40 bytes, no padding
    assert {name: dt.fields[name][1] for name in dt.names} == {"seed": 0, "gen": 8, "next_gen": 16, "learning_rate": 24,
                                                               "next_sigma": 32, "b": 36}
    assert sum(dt.fields[name][0].itemsize for name in dt.names) == 40
    assert (_lib.BATCH_ARS_MIN_N, _lib.BATCH_ARS_MAX_N) == (4, 16384)
    assert len(_lib.SIGNATURES["ses_ars_generation_batch"]) == 12
