"""The host side of batched sep_cma_es sweeps, without a device: what BatchedRuns accepts and refuses for the strategy, the
per-generation trial records against a sep_cma_es object's own host scalars, the constants blocks and the weight table against
sep_cma_constants, how sweep_main.py groups such trials, and the two ctypes structs against include/ses.h."""
import argparse
import copy
import ctypes
import math
import os
import re

import numpy as np
import pytest
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
P = 226

BASE = {
    "env": {"name": "CartPole-v1", "max_step": 500, "pomdp": False},
    "network": {"name": "gym_model", "num_state": 4, "num_action": 2, "discrete_action": True, "gru": False},
    "strategy": {"name": "sep_cma_es", "init_sigma": 0.5, "sigma_decay": 1.0, "offspring_num": 64},
}


def config(**changes):
    cfg = copy.deepcopy(BASE)
    for path, value in changes.items():
        block, key = path.split("__")
        cfg[block][key] = value
    return cfg


# ---- check_batchable ------------------------------------------------------------------------------------------------------------------

def test_sep_cma_trials_may_differ_in_every_allowed_key():
    from learning_strategies.evolution.batch import BATCHED_STRATEGIES, SEPCMA_VARYING, check_batchable
    assert "sep_cma_es" in BATCHED_STRATEGIES
    assert SEPCMA_VARYING == {"strategy": ("init_sigma", "sigma_decay", "elite_num", "scale_limits", "step_limits", "seed"),
                              "env": ("seed",)}
    check_batchable([config(),
                     config(strategy__init_sigma=0.1, strategy__sigma_decay=0.999, strategy__elite_num=5, strategy__scale_limits=[0.5, 2.0],
                            strategy__step_limits=[0.1, 10.0], strategy__seed=4, env__seed=9),
                     config(strategy__noise="philox", strategy__elite_num=64)])


@pytest.mark.parametrize("change,key", [
    (dict(strategy__offspring_num=32), "strategy.offspring_num"),
    (dict(network__gru=True), "network.gru"),
    (dict(network__num_state=5), "network.num_state"),
    (dict(env__name="CartPole-v0"), "env.name"),
    (dict(strategy__noise="numpy"), "strategy.noise"),
    (dict(strategy__learning_rate=0.1), "strategy.learning_rate"),       # openai_es's key is not one of sep_cma_es's
])
def test_sep_cma_batches_refuse_configs_that_differ_elsewhere(change, key):
    from learning_strategies.evolution.batch import BatchedRuns, check_batchable
    configs = [config(), config(strategy__elite_num=3), config(**change)]
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        check_batchable(configs)
    with pytest.raises(ValueError, match=key.replace(".", r"\.")):
        BatchedRuns(configs, 5, 2)


@pytest.mark.parametrize("name", ["pgpe", "lm_ma_es", "ma_es"])
def test_the_other_distribution_strategies_stay_sequential(name):
    from learning_strategies.evolution.batch import check_batchable
    with pytest.raises(ValueError, match=r"strategy\.name"):
        check_batchable([config(strategy__name=name), config(strategy__name=name)])
    with pytest.raises(ValueError, match=r"strategy\.name"):
        check_batchable([config(), config(strategy__name=name)])


@pytest.mark.parametrize("change", [dict(strategy__offspring_num=3), dict(strategy__offspring_num=8193)])
def test_batched_runs_refuses_populations_outside_the_counting_rank(change):
    from learning_strategies.evolution.batch import BatchedRuns
    with pytest.raises(ValueError, match="offspring_num"):
        BatchedRuns([config(**change), config(**change)], 5, 2)


# ---- the schedule ---------------------------------------------------------------------------------------------------------------------

def test_trial_table_reproduces_a_sep_cma_es_objects_host_scalars():
    """SepCmaSchedule against the class's own _generation, the device call stubbed out: it records what the call is given"""
    from learning_strategies.evolution.batch import SEPCMA_TRIAL_DTYPE, SepCmaSchedule, build_sepcma_trial_table
    from learning_strategies.evolution.offspring_strategies import sep_cma_constants, sep_cma_es
    blocks = [dict(BASE["strategy"], seed=3),                                                     # sigma_decay 1.0, elite_num defaulted
              dict(BASE["strategy"], init_sigma=0.37, sigma_decay=0.999, elite_num=5, seed=(1 << 40) + 1),
              dict(BASE["strategy"], init_sigma=2, sigma_decay=0.9, elite_num=64, scale_limits=[0.5, 2.0], step_limits=[0.1, 10.0])]
    schedules = [SepCmaSchedule(b, P) for b in blocks]
    assert [s.elite_num for s in schedules] == [32, 5, 64]
    assert schedules[2].scale_limits == (0.5, 2.0) and schedules[2].step_limits == (0.1, 10.0)
    table, sigmas = build_sepcma_trial_table(schedules, 10)
    assert table.shape == (10, 3) and table.dtype == SEPCMA_TRIAL_DTYPE and table.dtype.itemsize == 40

    class Recorder:
        def sepcma_generation(self, fit, seed, gen, sigma, hsig_scale, params, weights, state_in, state_out, next_sigma, next_gen,
                              first_row, n_rows, best=None):
            self.got = (seed, gen, sigma, hsig_scale, next_sigma, next_gen)

    class Shard:
        first, n_local = 0, 64

    for r, b in enumerate(blocks):
        s = sep_cma_es(b["init_sigma"], b["sigma_decay"], b["offspring_num"],
                       **{k: b[k] for k in ("elite_num", "scale_limits", "step_limits", "seed") if k in b})
        s.constants, _ = sep_cma_constants(s.offspring_num, P, s.elite_num)
        s.dev = Recorder()
        s.gen = 1                                     # the initial population took key 0 (_population bumps it per population)
        for g in range(10):
            s._last = {"gen": s.gen - 1}
            s._generation(None, None, None, Shard, None)
            seed, gen, sigma, hs, next_sigma, next_gen = s.dev.got
            s.gen += 1
            row = table[g, r]
            assert int(row["seed"]) == seed == s.seed and int(row["gen"]) == gen == g and int(row["next_gen"]) == next_gen == g + 1
            assert float(row["hsig_scale"]) == hs == s.hsig_scale(g + 1) and s.t == g + 1
            assert row["sigma"] == np.float32(sigma) and row["sigma"].dtype == np.float32
            assert row["next_sigma"] == np.float32(next_sigma) and next_sigma == s.curr_sigma
            assert sigmas[g][r] == s.curr_sigma
        assert schedules[r].t == s.t == 10 and schedules[r].curr_sigma == s.curr_sigma
    assert all(sig[0] == 0.5 for sig in sigmas), "sigma_decay 1.0 leaves curr_sigma alone"
    assert sigmas[9][1] != sigmas[8][1]


def test_the_schedule_refuses_what_the_class_refuses():
    from learning_strategies.evolution.batch import SepCmaSchedule
    for key, bad in (("elite_num", 0), ("elite_num", 65), ("offspring_num", 3), ("scale_limits", [1.5, 2.0]), ("step_limits", [2.0, 3.0])):
        with pytest.raises(ValueError):
            SepCmaSchedule(dict(BASE["strategy"], **{key: bad}), P)


# ---- the tables -----------------------------------------------------------------------------------------------------------------------

def test_constants_blocks_and_weight_table_equal_sep_cma_constants():
    from learning_strategies.evolution.batch import SEPCMA_CONSTS_DTYPE, sepcma_batch_tables
    from learning_strategies.evolution.offspring_strategies import sep_cma_constants
    n, mus = 64, (32, 1, 64, 5)
    scale = [(0.01, 100.0), (0.5, 2.0), (0.1, 1.0), (0.01, 100.0)]
    step = [(1e-6, 1e6), (0.1, 10.0), (1e-6, 1e6), (0.5, 1.0)]
    for params in (226, 6562):
        consts, weights, dicts = sepcma_batch_tables(n, params, mus, scale, step)
        assert consts.shape == (4,) and consts.dtype == SEPCMA_CONSTS_DTYPE and consts.dtype.itemsize == 80
        assert weights.shape == (4, n) and weights.dtype == np.float32
        for r, mu in enumerate(mus):
            c, w = sep_cma_constants(n, params, mu)
            assert dicts[r] == c
            assert np.array_equal(weights[r, :mu], w) and not weights[r, mu:].any() and np.all(weights[r, :mu] > 0)
            k = consts[r]
            f32 = np.float32
            # the host expressions of ses_sepcma_generation (csrc/ses_sepcma.hip), in double, cast once
            want = dict(hsig_thr=(1.4 + 2.0 / (params + 1.0)) * c["chi"], cs_over_ds=c["c_sigma"] / c["d_sigma"], chi=c["chi"],
                        a_s=f32(1.0 - c["c_sigma"]), b_s=f32(math.sqrt(c["c_sigma"] * (2.0 - c["c_sigma"]) * c["mueff"])),
                        a_c=f32(1.0 - c["c_c"]), hb1=f32(math.sqrt(c["c_c"] * (2.0 - c["c_c"]) * c["mueff"])),
                        c1f=f32(c["c_1"]), cmuf=f32(c["c_mu"]), k0_h1=f32(1.0 - c["c_1"] - c["c_mu"] + 0.0),
                        k0_h0=f32(1.0 - c["c_1"] - c["c_mu"] + c["c_1"] * c["c_c"] * (2.0 - c["c_c"])),
                        var_lo=f32(scale[r][0]) * f32(scale[r][0]), var_hi=f32(scale[r][1]) * f32(scale[r][1]),
                        step_lo=f32(step[r][0]), step_hi=f32(step[r][1]), mu=mu, reserved=0)
            assert set(want) == set(consts.dtype.names)
            for name, value in want.items():
                assert k[name] == value, (params, r, name, k[name], value)
                assert k[name].dtype == (np.float64 if name in ("hsig_thr", "cs_over_ds", "chi") else
                                         np.int32 if name in ("mu", "reserved") else np.float32)


# ---- the driver -----------------------------------------------------------------------------------------------------------------------

def resolved_grid():
    import sweep_main
    with open(os.path.join(SRC, "sweep_config", "cartpole_sep_cma_grid.yaml")) as f:
        spec = yaml.load(f, Loader=yaml.FullLoader)
    args = argparse.Namespace(seed=0, generation_num=1000, eval_ep_num=5)
    out = []
    for point in sweep_main.trial_points(spec, None, None):
        with open(os.path.join(SRC, point["cfg_path"])) as f:
            cfg = yaml.load(f, Loader=yaml.FullLoader)
        cfg, _, generation_num, eval_ep_num = sweep_main.resolve_trial(cfg, point, args)
        out.append((point["cfg_path"], cfg, generation_num, eval_ep_num))
    return out


def test_the_cartpole_sep_cma_grid_is_grouped():
    import sweep_main
    from learning_strategies.evolution.batch import check_batchable
    trials = resolved_grid()
    assert len(trials) == 16
    assert all(sweep_main.batch_key(*t) is None and sweep_main.elite_batch_key(*t) is None for t in trials), \
        "the two earlier keys keep their contracts"
    keys = [sweep_main.sepcma_batch_key(*t) for t in trials]
    assert keys[0] == ("conf/cartpole_sep_cma.yaml", "sep_cma_es", 256, 20, 5) and len(set(keys)) == 1
    assert sweep_main.group_trials(keys, 16) == [list(range(16))]
    assert sweep_main.group_trials(keys, 6) == [[0, 1, 2, 3, 4, 5], [6, 7, 8, 9, 10, 11], [12, 13, 14, 15]]
    assert sweep_main.group_trials(keys, 1) == [[i] for i in range(16)]
    check_batchable([t[1] for t in trials])
    # the grid's two axes reach the configs: the sweep's elite-num overrides the config file's
    assert sorted({t[1]["strategy"]["elite_num"] for t in trials}) == [16, 64, 128, 256]
    assert sorted({t[1]["strategy"]["init_sigma"] for t in trials}) == [0.25, 0.5, 1.0, 2.0]
    assert len({(t[1]["strategy"]["elite_num"], t[1]["strategy"]["init_sigma"]) for t in trials}) == 16


def test_sepcma_batch_key_members_and_refusals():
    import sweep_main
    key = sweep_main.sepcma_batch_key("conf/a.yaml", config(), 30, 5)
    assert key == ("conf/a.yaml", "sep_cma_es", 64, 30, 5)
    assert sweep_main.sepcma_batch_key("conf/a.yaml", config(strategy__elite_num=4, strategy__init_sigma=2.0), 30, 5) == key
    for other in (("conf/b.yaml", config(), 30, 5), ("conf/a.yaml", config(strategy__offspring_num=63), 30, 5),
                  ("conf/a.yaml", config(), 31, 5), ("conf/a.yaml", config(), 30, 4)):
        assert sweep_main.sepcma_batch_key(*other) not in (key, None)
    assert sweep_main.sepcma_batch_key("conf/a.yaml", config(strategy__noise="numpy"), 30, 5) is None
    assert sweep_main.sepcma_batch_key("conf/a.yaml", config(strategy__offspring_num=3), 30, 5) is None
    assert sweep_main.sepcma_batch_key("conf/a.yaml", config(strategy__offspring_num=4), 30, 5) is not None
    assert sweep_main.sepcma_batch_key("conf/a.yaml", config(strategy__offspring_num=8192), 30, 5) is not None
    assert sweep_main.sepcma_batch_key("conf/a.yaml", config(strategy__offspring_num=8193), 30, 5) is None
    for name in ("pgpe", "lm_ma_es", "ma_es", "openai_es", "simple_evolution"):
        assert sweep_main.sepcma_batch_key("conf/a.yaml", config(strategy__name=name), 30, 5) is None
    # consecutive equal keys group; a key of None (n = 3, n = 8193) runs alone
    cfgs = [config(), config(strategy__elite_num=2), config(strategy__offspring_num=3), config(strategy__offspring_num=8193), config(),
            config(strategy__init_sigma=1.0)]
    keys = [sweep_main.sepcma_batch_key("conf/a.yaml", c, 30, 5) for c in cfgs]
    assert keys[2] is None and keys[3] is None
    assert sweep_main.group_trials(keys, 4) == [[0, 1], [2], [3], [4, 5]]


def test_log_keeps_every_trial_alone(tmp_path, monkeypatch):
    """--log (wandb) is a per-run service: main() gives every trial the key None, so nothing is grouped.  run_trial and run_batch are
    replaced by recorders, no device is touched."""
    import sys
    import sweep_main
    record = {"ep5_mean_reward": 0.0, "best_reward": 0.0, "generations": 0, "log_dir": None}
    calls = []
    monkeypatch.setattr(sweep_main, "run_trial", lambda config, point, args: calls.append(1) or dict(record))
    monkeypatch.setattr(sweep_main, "run_batch", lambda configs, g, e: calls.append(len(configs)) or [dict(record) for _ in configs])
    with open(os.path.join(SRC, "sweep_config", "cartpole_sep_cma_grid.yaml")) as f:
        spec = yaml.load(f, Loader=yaml.FullLoader)
    spec["parameters"]["cfg-path"]["value"] = os.path.join(SRC, spec["parameters"]["cfg-path"]["value"])
    sweep = tmp_path / "grid.yaml"
    sweep.write_text(yaml.safe_dump(spec))
    monkeypatch.chdir(tmp_path)
    for flags, want in ((["--log"], [1] * 16), ([], [6, 6, 4])):
        calls.clear()
        monkeypatch.setattr(sys, "argv", ["sweep_main.py", "--sweep", str(sweep), "--concurrent", "6"] + flags)
        sweep_main.main()
        assert calls == want, (flags, calls)


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


@pytest.mark.parametrize("c_name,py_name,size", [("ses_batch_sepcma_trial", "SesBatchSepcmaTrial", 40),
                                                  ("ses_batch_sepcma_consts", "SesBatchSepcmaConsts", 80)])
def test_ctypes_structs_equal_the_headers(c_name, py_name, size):
    from ses import _lib
    fields, stated = header_struct(c_name)
    cls = getattr(_lib, py_name)
    assert list(cls._fields_) == fields

    class FromHeader(ctypes.Structure):
        _fields_ = fields

    assert ctypes.sizeof(cls) == ctypes.sizeof(FromHeader) == stated == size
    assert np.dtype(cls).itemsize == size
    assert len(_lib.SIGNATURES["ses_sepcma_generation_batch"]) == 20
