#!/usr/bin/env python3
"""Rollout time of the Walker2D kernels (Walker2DBulletEnv-v0; csrc/ses_walker2d.hip) in SEVERAL BUILDS of the library at once, with
HopperBulletEnv-v0 timed in the same process for scale.  The builds differ in WALKER2D_MLP_WAVES_PER_SIMD (the launch bound of every
kernel of the unit and the plan's wave-shape rule) and in Walker2dDef::PACK_MANIFOLDS:

    SES_OUT=ab/libw2d_w2.so  csrc/build.sh -DSES_WALKER2D_WAVES=2
    SES_OUT=ab/libw2d_w1.so  csrc/build.sh -DSES_WALKER2D_WAVES=1                          (what csrc/build.sh alone builds)
    SES_OUT=ab/libw2d_w2p.so csrc/build.sh -DSES_WALKER2D_WAVES=2 -DW2D_PACK_MANIFOLDS=true
    SES_OUT=ab/libw2d_w1p.so csrc/build.sh -DSES_WALKER2D_WAVES=1 -DW2D_PACK_MANIFOLDS=true

Every build is dlopen'ed into this one process (a HipES handle keeps the library it was made with) and timed on the same
populations: MLP at every lanes-per-env setting (ses_set_tuning box2d_lanes_per_env; 0 = the plan's own rule, which depends on the
waves per SIMD) and GRU, at 96, 256 and 4096 offspring x 5 episodes of up to 1000 steps, once with first-generation policies
(mu = 0 perturbed with conf/walker2d.yaml's init_sigma 0.2) and once with the zero policy.
The candidates ALTERNATE: every round times each setting of each build once, `rounds` rounds; a line carries the median and the
minimum over the rounds and "spread" = (max - min) / median of the same setting's repeats -- a difference between two settings or
builds counts only beyond it.  One JSON line per setting.
usage: time_walker2d.py rounds launches name=lib.so [name=lib.so ...]      (name "shipped" without a path: the tree's library)
profiles/walker2d_timing.txt is its output."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-es_amd"))
from ses import HipES, _lib  # noqa: E402

# env -> (num_state, num_action, max_step, init_sigma of its config)
ENVS = {"Walker2DBulletEnv-v0": (22, 6, 1000, 0.2), "HopperBulletEnv-v0": (15, 3, 1000, 0.2)}
WALKER2D = "Walker2DBulletEnv-v0"
E = 5
SHIPPED = _lib.LIB_PATH


def use_library(path):
    """the next HipES handles are made with this build (ses/_lib.py caches one dlopen; a handle keeps its own)"""
    _lib.LIB_PATH = path
    _lib._lib = None
    _lib.load()


class Setting:
    def __init__(self, build, env, gru, n, lanes=0, zero=False):
        S, A, T, sigma = ENVS[env]
        self.key = dict(build=build, env=env, policy="gru" if gru else "mlp", offspring=n, episodes=E, max_step=T,
                        population="zero" if zero else "first-generation")
        self.es = HipES(env, S, A, False, gru, max_step=T, eval_ep_num=E)
        if not gru:
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
                    fitness_sum=float(self.fit.double().sum().item()), env_steps_per_s=round(total / (med * 1e-3)))
        print(json.dumps(line), flush=True)
        self.es.close()


def main():
    rounds, launches = int(sys.argv[1]), int(sys.argv[2])
    builds = [(a.split("=", 1) + [SHIPPED])[:2] for a in sys.argv[3:]] or [["shipped", SHIPPED]]
    for n in (96, 256, 4096):
        settings = []
        for build, path in builds:
            use_library(os.path.abspath(path))
            for zero in (False, True):
                for lanes in (0, 1, 2, 4, 8, 16, 32, 64):
                    settings.append(Setting(build, WALKER2D, False, n, lanes, zero))
                settings.append(Setting(build, WALKER2D, True, n, 0, zero))
        use_library(SHIPPED)
        for gru in (False, True):
            settings.append(Setting("shipped", "HopperBulletEnv-v0", gru, n))
        for _ in range(rounds):
            for s in settings:
                s.time(launches)
        for s in settings:
            s.report()


if __name__ == "__main__":
    main()
