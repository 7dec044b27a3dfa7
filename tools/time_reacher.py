#!/usr/bin/env python3
"""Rollout time of the Reacher kernels (ReacherBulletEnv-v0; csrc/ses_f64_envs.hip) with Pendulum-v1 and the double pendulum
(InvertedDoublePendulumBulletEnv-v0) as yardsticks, in one process: MLP at every lanes-per-env setting (0 = the library's
choice) in both step forms -- one trig per step ("form": "one-trig") and the generic observe / step form (ses_set_tuning
reacher_generic_step = 1; "form": "generic") -- and GRU, at 240 and 4096 offspring, 5 episodes of 150 steps (Pendulum-v1 200;
the double pendulum up to 1000, ~21 under random policies).  The yardsticks run at the library's own lanes and form.  The
population is the first generation of openai_es (mu = 0 perturbed with init_sigma 0.5): random policies.
The candidates ALTERNATE: every round times each setting once, `rounds` rounds; a line carries the median and the minimum
over the rounds and "spread" = (max - min) / median of the same setting's repeats -- a difference between two settings counts
only beyond it.  One JSON line per setting.
usage: time_reacher.py [rounds] [launches per timing]
profiles/reacher_timing.txt is its output."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-es_amd"))
from ses import HipES  # noqa: E402

# env -> (num_state, num_action, max_step)
ENVS = {"ReacherBulletEnv-v0": (9, 2, 150), "Pendulum-v1": (3, 1, 200), "InvertedDoublePendulumBulletEnv-v0": (9, 1, 1000)}
REACHER = "ReacherBulletEnv-v0"
E = 5
SIGMA = 0.5


class Setting:
    def __init__(self, env, gru, n, lanes, generic=None):
        S, A, T = ENVS[env]
        self.key = dict(env=env, policy="gru" if gru else "mlp", offspring=n, episodes=E, max_step=T, lanes_per_env=lanes)
        self.es = HipES(env, S, A, False, gru, max_step=T, eval_ep_num=E, lanes_per_env=lanes)
        if generic is not None:
            self.key["form"] = "generic" if generic else "one-trig"
            self.es.set_tuning("reacher_generic_step", int(generic))
        elif not gru:
            self.key["form"] = "default"
        self.theta = self.es.perturb(self.es.zeros(1, self.es.P), SIGMA, 0, 0, 0, n)
        self.init = self.es.init_states_uniform(0, 0, 0, n)
        self.fit = self.es.empty(n)
        self.es.rollout(self.theta, self.init, fitness=self.fit)        # warm-up: loads the kernel
        torch.cuda.synchronize()
        self.ms = []

    def time(self, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            self.es.rollout(self.theta, self.init, fitness=self.fit)
        e1.record()
        e1.synchronize()
        self.ms.append(e0.elapsed_time(e1) / launches)

    def report(self):
        _, _, steps = self.es.rollout(self.theta, self.init, want_episodes=True)
        total = int(steps.sum().item())
        med = statistics.median(self.ms)
        line = dict(self.key, rollout_ms=round(med, 4), min_ms=round(min(self.ms), 4), spread=round((max(self.ms) - min(self.ms)) / med, 3),
                    env_steps=total, mean_episode_steps=round(total / (self.key["offspring"] * E), 1), env_steps_per_s=round(total / (med * 1e-3)))
        print(json.dumps(line), flush=True)
        self.es.close()


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    launches = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    for n in (240, 4096):
        settings = []
        for lanes in (0, 1, 2, 4, 8, 16, 32):
            settings.append(Setting(REACHER, False, n, lanes, False))
            settings.append(Setting(REACHER, False, n, lanes, True))
        settings.append(Setting(REACHER, True, n, 0))
        for env in ("Pendulum-v1", "InvertedDoublePendulumBulletEnv-v0"):
            settings.append(Setting(env, False, n, 0))
            settings.append(Setting(env, True, n, 0))
        for _ in range(rounds):
            for s in settings:
                s.time(launches)
        for s in settings:
            s.report()


if __name__ == "__main__":
    main()
