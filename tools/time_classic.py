#!/usr/bin/env python3
"""Rollout time of the classic-control kernels (Pendulum-v1, MountainCarContinuous-v0, MountainCar-v0, Acrobot-v1;
csrc/ses_f64_envs.hip): MLP at every lanes-per-env setting (0 = the library's choice) and GRU, at the shipped configs'
population sizes and at 4096 offspring, 5 episodes up to the TimeLimit (200 / 999 / 200 / 500 steps).  Pendulum's MLP rollout
is timed in both of its forms: the one-trig form (one sincos per step; "form": "one-sincos") and the generic
observe / step form (ses_set_tuning pendulum_generic_step = 1; "form": "generic").  The population is the first generation
of the config's strategy (mu = 0 perturbed with init_sigma): random policies, so nearly every episode runs to the cap -- the
rollout's worst case.  One JSON line per setting; median of `reps` launches timed with HIP events after a warm-up launch.
usage: time_classic.py [reps]
profiles/classic_control_cont_timing.txt is its output; its MountainCar-v0 and Acrobot-v1 lines are the settings of
profiles/classic_control_timing.txt."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-es_amd"))
from ses import HipES  # noqa: E402

# env -> (num_state, num_action, discrete, TimeLimit, population of the shipped config (openai_es: offspring_num;
# simple_evolution: offspring_num + mu), init_sigma of that config)
ENVS = {"Pendulum-v1": (3, 1, False, 200, 240, 0.5), "MountainCarContinuous-v0": (2, 1, False, 999, 97, 1.0),
        "MountainCar-v0": (2, 3, True, 200, 240, 0.5), "Acrobot-v1": (6, 3, True, 500, 97, 1.0)}
E = 5


def run(env, gru, n, lanes, reps, generic=False):
    S, A, discrete, T, _, sigma = ENVS[env]
    es = HipES(env, S, A, discrete, gru, max_step=T, eval_ep_num=E, lanes_per_env=lanes)
    if generic:
        es.set_tuning("pendulum_generic_step", 1)
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
    line = {"env": env, "policy": "gru" if gru else "mlp", "offspring": n, "episodes": E, "max_step": T, "lanes_per_env": lanes,
            "rollout_ms": round(ms, 4), "min_ms": round(min(ts), 4), "env_steps": total,
            "mean_episode_steps": round(total / (n * E), 1), "env_steps_per_s": round(total / (ms * 1e-3))}
    if env == "Pendulum-v1" and not gru:
        line["form"] = "generic" if generic else "one-sincos"
    print(json.dumps(line), flush=True)
    es.close()


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    for env, spec in ENVS.items():
        for n in (spec[4], 4096):
            for lanes in (0, 1, 2, 4, 8, 16, 32):
                run(env, False, n, lanes, reps)
                if env == "Pendulum-v1" and lanes:
                    run(env, False, n, lanes, reps, generic=True)
            run(env, True, n, 0, reps)


if __name__ == "__main__":
    main()
