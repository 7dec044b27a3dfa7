#!/usr/bin/env python3
"""Rollout time of LunarLander-v2 next to LunarLanderContinuous-v2, alternating in one process, at two shapes:
C3 (POMDP GRU, 4096 offspring x 5 episodes x <= 300 steps, sigma 0.168) and conf/lunarlander_v2.yaml's (MLP, 120 x 5 x <= 300,
sigma 2).  Both envs get the same population and the same resets; the world step is shared, the heads differ, and so do the
episodes the policies play -- so each line carries the env steps and the longest episode next to the time.  A third and fourth
block repeat the two shapes with the ZERO policy, under which both envs coast (argmax of equal logits = no-op, tanh(0) = engines
off) through identical trajectories: there the two kernels do the same physics, and what is left is the kernels' own difference.

    python tools/time_lander_discrete.py [alternations=7] [rollouts per sample=5]  >  profiles/lander_discrete_timing.txt

A sample is `rollouts per sample` back-to-back rollouts between two device events; both handles are warmed first."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-es_amd"))
from ses import HipES  # noqa: E402

ALTERNATIONS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
PER_SAMPLE = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def shape(title, gru, pomdp, n, sigma):
    envs = {"LunarLander-v2": True, "LunarLanderContinuous-v2": False}
    hs = {name: HipES(name, 8, 4, disc, gru, pomdp=pomdp, max_step=300, eval_ep_num=5) for name, disc in envs.items()}
    first = next(iter(hs.values()))
    theta = first.perturb(first.zeros(first.P), sigma, 0, 0, 0, n) if sigma > 0 else first.zeros(n, first.P)
    init = first.init_states_uniform(0, 0, 0, n)
    fit = first.empty(n)
    facts = {}
    for name, es in hs.items():                                     # warm-up, and what the policies play
        _, _, steps = es.rollout(theta, init, want_episodes=True)
        es.rollout(theta, init, fitness=fit)
        torch.cuda.synchronize()
        facts[name] = (int(steps.sum().item()), int(steps.max().item()))
    ms = {name: [] for name in hs}
    for _ in range(ALTERNATIONS):
        for name, es in hs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(PER_SAMPLE):
                es.rollout(theta, init, fitness=fit)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / PER_SAMPLE)
    print(f"{title}: {n} offspring x 5 episodes x <= 300 steps; {ALTERNATIONS} alternations, {PER_SAMPLE} rollouts per sample")
    for name in hs:
        t, (total, longest) = ms[name], facts[name]
        med = statistics.median(t)
        print(f"  {name:26s} median {med:8.3f} ms  min {min(t):8.3f}  max {max(t):8.3f}  spread {max(t) - min(t):6.3f} ms   "
              f"env steps {total:8d}  mean episode {total / (n * 5):6.1f}  longest {longest:3d}   {total / (med * 1e-3):.3e} env-steps/s   "
              f"{med / longest * 1e3:7.1f} us per step of the longest episode")
        print("    samples (ms): " + " ".join(f"{x:.3f}" for x in t))
    for es in hs.values():
        es.close()


print(f"device: {torch.cuda.get_device_name(0)}")
shape("C3, POMDP GRU", True, True, 4096, 0.168)
shape("MLP (conf/lunarlander_v2.yaml's shape)", False, False, 120, 2.0)
shape("C3 shape, zero policy (both envs coast: identical trajectories)", True, True, 4096, 0.0)
shape("MLP shape, zero policy (both envs coast: identical trajectories)", False, False, 120, 0.0)
