"""python sweep_main.py --cfg-path conf/cartpole_openai.yaml --init-sigma 0.3   (one trial, like the reference)
python sweep_main.py --sweep sweep_config/cartpole_openaies.yaml --count 16     (a whole sweep, wandb-free)
python sweep_main.py --sweep sweep_config/cartpole_openaies.yaml --count 16 --concurrent 16   (its trials as one population)

The reference's sweep_main.py (sweep_main.py:33-88) is a per-trial entry point that a `wandb agent` calls with
hyper-parameter flags; the sweep itself lives in the wandb service.  Here a generation takes milliseconds, so the
driver can run every trial of a sweep in this process.  The sweep files keep the reference's format
(sweep_config/*.yaml: method / metric / parameters with value | values | min,max).  `method: grid` enumerates the
`values` lists; `random` and `bayes` draw uniformly (there is no surrogate model here -- with trials this cheap a
larger random budget does the same job).  One line per trial goes to logs/sweeps/<name>/trials.jsonl and the best
trial is printed at the end.

--concurrent R (default 1: one trial after the other) advances up to R consecutive openai_es, simple_evolution, simple_genetic,
sep_cma_es or ars trials of one config in lockstep as ONE device population (learning_strategies/evolution/batch.py): a trial of 96
or 256 offspring fills a fraction of the chip.  simple_evolution / simple_genetic trials may differ in elite_num as well (under
simple_genetic it sets the row count: the batch is ragged); populations above 1024 rows run alone.  sep_cma_es trials may differ in
elite_num, scale_limits and step_limits too (populations of 4 .. 8192 rows).  ars trials may differ in learning_rate and elite_num
too (even populations of 4 .. 16384 rows).  pgpe, lm_ma_es and ma_es trials run one after the other.
Each trial computes what it computes alone, bit for bit; the points, their order and the records are the same.
"""
import argparse
import copy
import itertools
import json
import os
import random

import numpy as np
import torch
import yaml

import builder
from run_es import change_value, set_seed

_OVERRIDES = (("init_sigma", float), ("sigma_decay", float), ("learning_rate", float), ("elite_num", int),
              ("offspring_num", int))
_RUN_KEYS = {"cfg_path": str, "generation_num": int, "eval_ep_num": int, "seed": int}


def trial_points(spec, count, rng):
    """Yield {flag_name: value} dicts from a reference-format `parameters` block."""
    params = {k.replace("-", "_"): v for k, v in spec["parameters"].items()}
    fixed = {k: v["value"] for k, v in params.items() if "value" in v}
    lists = {k: v["values"] for k, v in params.items() if "values" in v}
    ranges = {k: (v["min"], v["max"]) for k, v in params.items() if "min" in v}
    if spec.get("method", "random") == "grid":
        if ranges:
            raise ValueError("grid sweeps need `values` lists, not min/max ranges: " + ", ".join(ranges))
        for n, combo in enumerate(itertools.product(*lists.values())):
            if count is not None and n >= count:
                return
            yield {**fixed, **dict(zip(lists.keys(), combo))}
        return
    for _ in range(count if count is not None else 10):
        point = dict(fixed)
        point.update({k: rng.choice(v) for k, v in lists.items()})
        for k, (lo, hi) in ranges.items():
            point[k] = rng.randint(lo, hi) if isinstance(lo, int) and isinstance(hi, int) else rng.uniform(lo, hi)
        yield point


def resolve_trial(config, point, args):
    """(the config with the point's overrides and seeds, seed, generation_num, eval_ep_num) of one trial"""
    config = copy.deepcopy(config)
    for key, typ in _OVERRIDES:
        if point.get(key) is not None:
            change_value(config, key, typ(point[key]))
    seed = int(point.get("seed", args.seed))
    config.setdefault("strategy", {}).setdefault("seed", seed)
    config.setdefault("env", {}).setdefault("seed", seed)
    return config, seed, int(point.get("generation_num", args.generation_num)), int(point.get("eval_ep_num", args.eval_ep_num))


def trial_record(best, log_dir):
    tail = best[-5:]
    return {"ep5_mean_reward": sum(tail) / max(len(tail), 1), "best_reward": max(best) if best else None,
            "generations": len(best), "log_dir": log_dir}


def run_trial(config, point, args):
    """One ESLoop run with the point's overrides; returns the trial record."""
    config, seed, generation_num, eval_ep_num = resolve_trial(config, point, args)
    set_seed(seed)
    loop = builder.build_loop(config, generation_num, args.process_num, eval_ep_num, args.log, args.save_model_period)
    loop.run()
    return trial_record([b for b, _ in loop.history], loop.save_dir)


def batch_key(cfg_path, config, generation_num, eval_ep_num):
    """What two trials must share to advance as one population (BatchedRuns checks the rest), or None for a trial that runs alone."""
    strategy = config.get("strategy", {})
    if strategy.get("name") != "openai_es" or strategy.get("noise", "philox") != "philox":
        return None
    return (cfg_path, int(strategy["offspring_num"]), int(generation_num), int(eval_ep_num))


def elite_batch_key(cfg_path, config, generation_num, eval_ep_num):
    """batch_key for simple_evolution / simple_genetic trials: they may differ in elite_num too (a ragged batch), so the key holds
    the strategy and offspring_num; None unless the noise is Philox and the trial's population fits one workgroup's rank (1024 rows)."""
    strategy = config.get("strategy", {})
    name = strategy.get("name")
    if name not in ("simple_evolution", "simple_genetic") or strategy.get("noise", "philox") != "philox":
        return None
    offspring_num, elite_num = int(strategy["offspring_num"]), int(strategy.get("elite_num", 0))
    if elite_num < 1:
        return None
    rows = offspring_num + 1 if name == "simple_evolution" else elite_num * (offspring_num // elite_num)
    if not 2 <= rows <= 1024 or elite_num > rows:
        return None
    return (cfg_path, name, offspring_num, int(generation_num), int(eval_ep_num))


def sepcma_batch_key(cfg_path, config, generation_num, eval_ep_num):
    """batch_key for sep_cma_es trials: they may differ in elite_num and the limits too, each with its own constants on the device, so
    the key holds the strategy and offspring_num; None unless the noise is Philox and the population is one the counting rank serves
    (4 .. 8192 rows)."""
    strategy = config.get("strategy", {})
    if strategy.get("name") != "sep_cma_es" or strategy.get("noise", "philox") != "philox":
        return None
    offspring_num = int(strategy["offspring_num"])
    if not 4 <= offspring_num <= 8192:
        return None
    return (cfg_path, "sep_cma_es", offspring_num, int(generation_num), int(eval_ep_num))


def ars_batch_key(cfg_path, config, generation_num, eval_ep_num):
    """batch_key for ars trials: they may differ in learning_rate and elite_num too (the selected list is ragged on the device), so the
    key holds the strategy and offspring_num; None unless the noise is Philox and the population is one whose pair scores the counting
    rank serves (even, 4 .. 16384 rows)."""
    strategy = config.get("strategy", {})
    if strategy.get("name") != "ars" or strategy.get("noise", "philox") != "philox":
        return None
    offspring_num = int(strategy["offspring_num"])
    if offspring_num % 2 or not 4 <= offspring_num <= 16384:
        return None
    return (cfg_path, "ars", offspring_num, int(generation_num), int(eval_ep_num))


def group_trials(keys, concurrent):
    """Lists of trial indices, in index order: runs of CONSECUTIVE trials with the same key (not None) cut into batches of up to
    `concurrent`; every other trial alone.  Their concatenation is 0 .. len(keys) - 1."""
    groups = []
    for i, key in enumerate(keys):
        last = groups[-1] if groups else None
        if concurrent > 1 and key is not None and last is not None and len(last) < concurrent and keys[last[0]] == key:
            last.append(i)
        else:
            groups.append([i])
    return groups


def run_batch(configs, generation_num, eval_ep_num):
    """The trials of one group as one population; returns their records in order."""
    from learning_strategies.evolution.batch import BatchedRuns
    runs = BatchedRuns(configs, generation_num, eval_ep_num)
    try:
        runs.run()
        return [trial_record(runs.history[r], runs.save_dirs[r]) for r in range(runs.R)]
    finally:
        runs.close()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--cfg-path", type=str, default="conf/lunarlander_openai.yaml", help="config file to run.")
    parser.add_argument("--seed", type=int, default=0, help="random seed.")
    parser.add_argument("--process-num", type=int, default=12, help="kept for compatibility (no worker processes).")
    parser.add_argument("--generation-num", type=int, default=1000, help="max number of generation iteration.")
    parser.add_argument("--eval-ep-num", type=int, default=5, help="number of model evaluaion per iteration.")
    parser.add_argument("--log", action="store_true", help="wandb log")
    parser.add_argument("--save-model-period", type=int, default=10, help="save model for every n iteration.")
    for key, typ in _OVERRIDES:
        parser.add_argument("--" + key.replace("_", "-"), type=typ, default=None)
    parser.add_argument("--sweep", type=str, default=None, help="sweep file (reference sweep_config format).")
    parser.add_argument("--count", type=int, default=None, help="number of trials (default: whole grid / 10 draws).")
    parser.add_argument("--concurrent", type=int, default=1,
                        help="advance up to this many consecutive openai_es, simple_evolution, simple_genetic, sep_cma_es or ars "
                             "trials of one config as one device population (the elite strategies', sep_cma_es's and ars's trials "
                             "may differ in elite_num).")
    args = parser.parse_args()

    if args.sweep is None:                              # the reference's behaviour: one trial from the flags
        with open(args.cfg_path) as f:
            config = yaml.load(f, Loader=yaml.FullLoader)
        record = run_trial(config, {k: getattr(args, k) for k, _ in _OVERRIDES}, args)
        print(json.dumps(record))
        return

    with open(args.sweep) as f:
        spec = yaml.load(f, Loader=yaml.FullLoader)
    metric = (spec.get("metric") or {}).get("name", "ep5_mean_reward")
    sign = -1.0 if (spec.get("metric") or {}).get("goal", "maximize") == "minimize" else 1.0
    name = os.path.splitext(os.path.basename(args.sweep))[0]
    out_dir = os.path.join("logs", "sweeps", name)
    os.makedirs(out_dir, exist_ok=True)
    rng = random.Random(args.seed)
    best = None

    def report(n, point, result):
        nonlocal best
        record = {"trial": n, "params": point, **result}
        with open(os.path.join(out_dir, "trials.jsonl"), "a") as f:
            f.write(json.dumps(record) + "\n")
        print(f"trial {n}: {metric} = {record[metric]:.3f}  params = {point}")
        if best is None or sign * record[metric] > sign * best[metric]:
            best = record

    def load(point):
        cfg_path = point.get("cfg_path", args.cfg_path)
        with open(cfg_path) as f:
            return cfg_path, yaml.load(f, Loader=yaml.FullLoader)

    if args.concurrent <= 1:
        for n, point in enumerate(trial_points(spec, args.count, rng)):
            report(n, point, run_trial(load(point)[1], point, args))
        print("best:", json.dumps(best))
        return

    # all points first (the same draws, so the same points), then consecutive batchable ones together
    points = list(trial_points(spec, args.count, rng))
    loaded = [load(point) for point in points]
    resolved = [resolve_trial(config, point, args) for (_, config), point in zip(loaded, points)]
    # (a config with network.obs_normalizer runs its trials one after the other: one population cannot share R normalisers)
    keys = [None if args.log or config.get("network", {}).get("obs_normalizer", False) else (batch_key(cfg_path, config, generation_num, eval_ep_num)
                                   or elite_batch_key(cfg_path, config, generation_num, eval_ep_num)
                                   or sepcma_batch_key(cfg_path, config, generation_num, eval_ep_num)
                                   or ars_batch_key(cfg_path, config, generation_num, eval_ep_num))
            for (cfg_path, _), (config, _, generation_num, eval_ep_num) in zip(loaded, resolved)]
    for group in group_trials(keys, args.concurrent):
        if len(group) == 1:
            n = group[0]
            report(n, points[n], run_trial(loaded[n][1], points[n], args))
            continue
        set_seed(resolved[group[0]][1])
        results = run_batch([resolved[n][0] for n in group], resolved[group[0]][2], resolved[group[0]][3])
        for n, result in zip(group, results):
            report(n, points[n], result)
    print("best:", json.dumps(best))


if __name__ == "__main__":
    main()
