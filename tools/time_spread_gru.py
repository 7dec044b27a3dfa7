#!/usr/bin/env python3
"""The recurrent simple_spread rollout (csrc/ses_spread_gru.hip) by wave mapping -- "spread_gru_wave_per_batch" 0: a wave plays the
column batches of its offspring one after the other, 1: one wave per (offspring, batch) -- at 240 x 5 (conf/simplespread_gru.yaml) and
4096 x 5 episodes of 25 cycles (1024 and 2048 in between place the crossover of the default), two and three agents: us per ses_rollout (rollout kernel + episode-mean kernel), device events,
the candidates of a size alternating inside one process.  Yardsticks in the same run: the MLP spread rollout at the same sizes, and
the POMDP CartPole GRU rollout forced onto the plain lockstep form (gru_ep_parallel_max=0, gru_mfma4_min_e=0) at 8 episodes x 25
fixed-length steps = one full 8-column batch of 25 policy steps.

    python tools/time_spread_gru.py > profiles/spread_gru_timing.txt"""
import json, os, statistics, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "simple-es_amd")]
from ses import HipES, MODE_EPISODIC, MODE_FIXED_LENGTH

ROUNDS, CALLS = 15, 20


def prepare(es, n, mode):
    theta = es.perturb(es.zeros(es.P), 1.0, 0, 0, 0, n)
    init = es.init_states_uniform(0, 0, 0, n)
    fit = es.empty(n)
    run = lambda: es.rollout(theta, init, mode=mode, fitness=fit)
    for _ in range(30): run()
    torch.cuda.synchronize()
    return run


def alternate(runs):
    """{name: callable} -> {name: median us per call}: ROUNDS rounds, every candidate timed once per round, in turn"""
    ts = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS): run()
            e1.record(); e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1000 / CALLS)
    return {k: [round(statistics.median(v), 1), round(min(v), 1), round(max(v), 1)] for k, v in ts.items()}


print(json.dumps({"unit": "us per ses_rollout: [median, min, max] of %d rounds x %d calls" % (ROUNDS, CALLS)}), flush=True)
for n in (240, 1024, 2048, 4096):                   # the config, two sizes that place the crossover, the large population
    handles, runs = [], {}
    for na in (2, 3):
        mlp = HipES("simple_spread", 6 * na, 5, True, False, max_step=25, eval_ep_num=5, n_agents=na)
        handles.append(mlp)
        runs[f"na{na}_mlp"] = prepare(mlp, n, MODE_EPISODIC)
        for name, knob in (("per_offspring", 0), ("per_batch", 1), ("default", -1)):
            es = HipES("simple_spread", 6 * na, 5, True, True, max_step=25, eval_ep_num=5, n_agents=na)
            es.set_tuning("spread_gru_wave_per_batch", knob)
            handles.append(es)
            runs[f"na{na}_gru_{name}"] = prepare(es, n, MODE_EPISODIC)
    cp = HipES("CartPole-v1", 4, 2, True, True, pomdp=True, max_step=25, eval_ep_num=8)
    cp.set_tuning("gru_ep_parallel_max", 0)
    cp.set_tuning("gru_mfma4_min_e", 0)
    handles.append(cp)
    runs["cartpole_gru_lockstep_8x25"] = prepare(cp, n, MODE_FIXED_LENGTH)
    print(json.dumps({"offspring": n, "episodes": 5, "cycles": 25, **alternate(runs)}), flush=True)
    for h in handles: h.close()
