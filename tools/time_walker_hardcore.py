#!/usr/bin/env python3
"""Rollout time of the BipedalWalkerHardcore-v3 kernels (csrc/ses_walker_hardcore.hip) with BipedalWalker-v3 timed in the same
process: MLP (the plan's own wave shape, ses_rollout_plan.h) and GRU, at 96, 256 and 4096 offspring x 5 episodes of up to 300 steps
(both configs' max_step), once with first-generation policies (mu = 0 perturbed with conf/bipedalwalker_hardcore.yaml's init_sigma 2)
and once with the zero policy.  BipedalWalker-v3 has no GRU kernel.
The settings ALTERNATE: every round times each setting once, `rounds` rounds; a line carries the median and the minimum over the
rounds and "spread" = (max - min) / median of the same setting's repeats -- a difference between two settings counts only beyond
it.  One JSON line per setting.
usage: time_walker_hardcore.py [rounds] [launches per timing] [shapes]
"shapes": BipedalWalkerHardcore-v3's MLP rollout at 4096 offspring with ses_set_tuning box2d_envs_per_wave forced to 8 ... 32 next to
the plan's own shape (0), the same way.
profiles/walker_hardcore_timing.txt is its output."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-es_amd"))
from ses import HipES  # noqa: E402

HARDCORE, WALKER = "BipedalWalkerHardcore-v3", "BipedalWalker-v3"
E, T, SIGMA = 5, 300, 2.0


class Setting:
    def __init__(self, env, gru, n, zero, epw=0):
        self.key = dict(env=env, policy="gru" if gru else "mlp", offspring=n, episodes=E, max_step=T,
                        population="zero" if zero else "first-generation")
        self.es = HipES(env, 24, 4, False, gru, max_step=T, eval_ep_num=E)
        if epw:
            self.es.set_tuning("box2d_envs_per_wave", epw)
        if not gru:
            plan = self.es.rollout_plan(n, **({"box2d_envs_per_wave": epw} if epw else {}))
            self.key["lanes_per_env"], self.key["envs_per_wave"] = int(plan.box2d_lpe), int(plan.box2d_epw)
        mu = self.es.zeros(1, self.es.P)
        self.theta = self.es.zeros(n, self.es.P) if zero else self.es.perturb(mu, SIGMA, 0, 0, 0, n)
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
        total, longest = int(steps.sum().item()), int(steps.max().item())
        med = statistics.median(self.ms)
        line = dict(self.key, rollout_ms=round(med, 4), min_ms=round(min(self.ms), 4), spread=round((max(self.ms) - min(self.ms)) / med, 3),
                    env_steps=total, mean_episode_steps=round(total / (self.key["offspring"] * E), 1), longest_episode=longest,
                    env_steps_per_s=round(total / (med * 1e-3)))
        print(json.dumps(line), flush=True)
        self.es.close()


def shapes(rounds, launches):
    """the plan's cap of 16 envs per wave against forced shapes at 4096 offspring: fewer envs in more waves, and more than the LDS of
    four workgroups per CU admits"""
    settings = [Setting(HARDCORE, False, 4096, zero, epw) for zero in (False, True) for epw in (0, 8, 10, 12, 16, 20, 32)]
    for _ in range(rounds):
        for s in settings:
            s.time(launches)
    for s in settings:
        s.report()


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    launches = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    if sys.argv[3:4] == ["shapes"]:
        return shapes(rounds, launches)
    for n in (96, 256, 4096):
        settings = []
        for zero in (False, True):
            settings.append(Setting(HARDCORE, False, n, zero))
            settings.append(Setting(HARDCORE, True, n, zero))
            settings.append(Setting(WALKER, False, n, zero))
        for _ in range(rounds):
            for s in settings:
                s.time(launches)
        for s in settings:
            s.report()


if __name__ == "__main__":
    main()
