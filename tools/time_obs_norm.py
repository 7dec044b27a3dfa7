#!/usr/bin/env python3
"""What the running observation normaliser costs a rollout (csrc/ses_obs_norm.hip; include/ses.h: ses_obs_norm_bind), in one
process: Pendulum-v1 (200 steps), InvertedPendulumSwingupBulletEnv-v0 (1000) and ReacherBulletEnv-v0 (150) -- none of them
terminates, so every setting does the same number of env steps -- at 240 and 4096 offspring x 5 episodes and the library's own
lanes per env, as
    unbound      nothing bound: the kernel every handle ran before the normaliser existed
    frozen       bound with update off: the normalising kernel (playback, evaluation)
    update       bound with update on: the accumulating kernel plus the merge launch
and the merge launch alone on partials of the same population ("merge").  The population is the first generation of openai_es
(mu = 0 perturbed with init_sigma 0.5): random policies.  The candidates ALTERNATE: every round times each setting once,
`rounds` rounds; a line carries the median and the minimum over the rounds and "spread" = (max - min) / median of the same
setting's repeats, and "ratio" = its median over the unbound rollout's of the same env and population in the same process -- a
ratio counts only beyond the spreads.  One JSON line per setting.
usage: time_obs_norm.py [rounds] [launches per timing]
profiles/obs_norm_timing.txt is its output."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-es_amd"))
from ses import HipES  # noqa: E402

# env -> (num_state, num_action, max_step)
ENVS = {"Pendulum-v1": (3, 1, 200), "InvertedPendulumSwingupBulletEnv-v0": (5, 1, 1000), "ReacherBulletEnv-v0": (9, 2, 150)}
E = 5
SIGMA = 0.5


class Setting:
    def __init__(self, env, n, mode):
        S, A, T = ENVS[env]
        self.key = dict(env=env, offspring=n, episodes=E, max_step=T, mode=mode)
        self.mode = mode
        self.es = HipES(env, S, A, False, False, max_step=T, eval_ep_num=E)
        self.theta = self.es.perturb(self.es.zeros(1, self.es.P), SIGMA, 0, 0, 0, n)
        self.init = self.es.init_states_uniform(0, 0, 0, n)
        self.fit = self.es.empty(n)
        self.stats, self.affine = self.es.obs_norm_new()
        if mode in ("frozen", "update"):
            self.es.obs_norm_bind(self.stats, self.affine, update=mode == "update")
        if mode == "merge":
            self.partials = torch.rand(2 * S + 1, n * E, dtype=torch.float64, device=self.es.device) + 1.0
        self.launch()                                                   # warm-up: loads the kernel
        torch.cuda.synchronize()
        self.ms = []

    def launch(self):
        if self.mode == "merge":
            self.es.obs_norm_merge(self.partials, self.stats, self.affine)
        else:
            self.es.rollout(self.theta, self.init, fitness=self.fit)

    def time(self, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            self.launch()
        e1.record()
        e1.synchronize()
        self.ms.append(e0.elapsed_time(e1) / launches)

    def median(self):
        return statistics.median(self.ms)

    def report(self, unbound_ms):
        med = self.median()
        line = dict(self.key, ms=round(med, 4), min_ms=round(min(self.ms), 4), spread=round((max(self.ms) - min(self.ms)) / med, 3),
                    ratio=round(med / unbound_ms, 3))
        print(json.dumps(line), flush=True)
        self.es.close()


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    launches = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    for n in (240, 4096):
        for env in ENVS:
            settings = [Setting(env, n, mode) for mode in ("unbound", "frozen", "update", "merge")]
            for _ in range(rounds):
                for s in settings:
                    s.time(launches)
            unbound_ms = settings[0].median()
            for s in settings:
                s.report(unbound_ms)


if __name__ == "__main__":
    main()
