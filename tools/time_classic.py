#!/usr/bin/env python3
"""Rollout time of the classic-control kernels (Acrobot-v1, MountainCar-v0; csrc/ses_classic.hip): MLP at every lanes-per-env
setting (0 = the library's choice) and GRU, at the shipped configs' population sizes and at 4096 offspring, 5 episodes up
to the TimeLimit (500 / 200 steps).  The population is the first generation of the config's strategy (mu = 0 perturbed
with init_sigma): the policies are random, so nearly every episode runs to the cap -- the rollout's worst case.  One JSON
line per setting; median of `reps` launches timed with HIP events.   usage: time_classic.py [reps]
profiles/classic_control_timing.txt is its output."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-es_amd"))
from ses import HipES  # noqa: E402

# env -> (num_state, TimeLimit, population of the shipped config (conf/acrobot.yaml: simple_evolution, 96 offspring + mu;
# conf/mountaincar.yaml: openai_es, 240 offspring), init_sigma of that config)
ENVS = {"Acrobot-v1": (6, 500, 97, 1.0), "MountainCar-v0": (2, 200, 240, 0.5)}
E = 5


def run(env, gru, n, lanes, reps):
    S, T, _, sigma = ENVS[env]
    es = HipES(env, S, 3, True, gru, max_step=T, eval_ep_num=E, lanes_per_env=lanes)
    theta = es.perturb(es.zeros(1, es.P), sigma, 0, 0, 0, n)
    init = es.init_states_uniform(0, 0, 0, n)
    fit = es.empty(n)
    es.rollout(theta, init, fitness=fit)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        es.rollout(theta, init, fitness=fit)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    _, _, steps = es.rollout(theta, init, want_episodes=True)
    total = int(steps.sum().item())
    ms = statistics.median(ts)
    print(json.dumps({"env": env, "policy": "gru" if gru else "mlp", "offspring": n, "episodes": E, "max_step": T,
                      "lanes_per_env": lanes, "rollout_ms": round(ms, 4), "min_ms": round(min(ts), 4), "env_steps": total,
                      "mean_episode_steps": round(total / (n * E), 1), "env_steps_per_s": round(total / (ms * 1e-3))}), flush=True)
    es.close()


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    for env, (_, _, n_conf, _) in ENVS.items():
        for n in (n_conf, 4096):
            for lanes in (0, 1, 2, 4, 8, 16, 32):
                run(env, False, n, lanes, reps)
            run(env, True, n, 0, reps)


if __name__ == "__main__":
    main()
