#!/usr/bin/env python3
"""Rollout time of the hopper kernels (HopperBulletEnv-v0; csrc/ses_hopper.hip) with BipedalWalker-v3 and ReacherBulletEnv-v0 timed
in the same process for scale: MLP at every lanes-per-env setting (ses_set_tuning box2d_lanes_per_env; 0 = the plan's own rule,
ses_rollout_plan.h box2d_wave_shape) and GRU, at 96, 256 and 4096 offspring x 5 episodes of up to 1000 steps, once with
first-generation policies (mu = 0 perturbed with conf/hopper.yaml's init_sigma 0.2) and once with the zero policy.  The yardsticks
run their own configs' horizons at the library's own wave shape, first-generation policies.
The candidates ALTERNATE: every round times each setting once, `rounds` rounds; a line carries the median and the minimum over the
rounds and "spread" = (max - min) / median of the same setting's repeats -- a difference between two settings counts only beyond
it.  One JSON line per setting.
usage: time_hopper.py [rounds] [launches per timing]
profiles/hopper_timing.txt is its output."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-es_amd"))
from ses import HipES  # noqa: E402

# env -> (num_state, num_action, max_step, init_sigma of its config)
ENVS = {"HopperBulletEnv-v0": (15, 3, 1000, 0.2), "BipedalWalker-v3": (24, 4, 1600, 2.0), "ReacherBulletEnv-v0": (9, 2, 150, 0.2)}
HOPPER = "HopperBulletEnv-v0"
E = 5


class Setting:
    def __init__(self, env, gru, n, lanes=0, zero=False):
        S, A, T, sigma = ENVS[env]
        self.key = dict(env=env, policy="gru" if gru else "mlp", offspring=n, episodes=E, max_step=T,
                        population="zero" if zero else "first-generation")
        self.es = HipES(env, S, A, False, gru, max_step=T, eval_ep_num=E)
        if env == HOPPER and not gru:
            self.key["box2d_lanes_per_env"] = lanes
            if lanes:
                self.es.set_tuning("box2d_lanes_per_env", lanes)
        mu = self.es.zeros(1, self.es.P)
        self.theta = self.es.zeros(n, self.es.P) if zero else self.es.perturb(mu, sigma, 0, 0, 0, n)
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


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    launches = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    for n in (96, 256, 4096):
        settings = []
        for zero in (False, True):
            for lanes in (0, 1, 2, 4, 8, 16, 32, 64):
                settings.append(Setting(HOPPER, False, n, lanes, zero))
            settings.append(Setting(HOPPER, True, n, 0, zero))
        settings.append(Setting("BipedalWalker-v3", False, n))
        settings.append(Setting("ReacherBulletEnv-v0", False, n))
        for _ in range(rounds):
            for s in settings:
                s.time(launches)
        for s in settings:
            s.report()


if __name__ == "__main__":
    main()
