#!/usr/bin/env python3
"""Rollout time of waterworld (csrc/ses_waterworld.hip) with its 242-wide fc1 on the matrix cores and on the VALU
("waterworld_fc1_mfma" 1 / 0), alternating in one process, at 256 and 4096 offspring x 5 episodes x 500 cycles (one team cycle =
one env-step).  Next to each time: the MFMA issue floor of the shape -- tiles per offspring x 121 k-blocks x 64 cycles per
v_mfma_f32_32x32x2_f32 x cycles of the episode x waves per SIMD, at the engine clock -- and the fraction of it the MFMA form achieves.

    python tools/time_waterworld.py [alternations=5] [rollouts per sample=2]  >  profiles/waterworld_timing.txt

A sample is `rollouts per sample` back-to-back rollouts between two device events; both forms are warmed first and their fitness
vectors compared bit for bit."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "simple-es_amd"))
from ses import HipES  # noqa: E402

ALTERNATIONS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
PER_SAMPLE = int(sys.argv[2]) if len(sys.argv) > 2 else 2
E, CYCLES, TILE_E, KB, MFMA_CYCLES = 5, 500, 6, 121, 64


def engine_clock_hz():
    """(Hz, where it comes from): the clock sampled now if the driver interface answers, else the device's rated peak"""
    try:
        return torch.cuda.clock_rate() * 1e6, "sampled after the timed runs (torch.cuda.clock_rate)"
    except Exception:
        return torch.cuda.get_device_properties(0).clock_rate * 1e3, "the device's rated peak (not sampled)"


def shape(n, sigma):
    forms = {"mfma": 1, "valu": 0}
    hs = {}
    for name, knob in forms.items():
        hs[name] = HipES("waterworld", 242, 2, False, False, max_step=CYCLES, eval_ep_num=E, n_agents=5)
        hs[name].set_tuning("waterworld_fc1_mfma", knob)
    first = hs["mfma"]
    theta = first.perturb(first.zeros(first.P), sigma, 0, 0, 0, n)
    init = first.init_states_uniform(0, 0, 0, n)
    fits = {name: es.rollout(theta, init).clone() for name, es in hs.items()}                # warm-up
    torch.cuda.synchronize()
    same = torch.equal(fits["mfma"].view(torch.int32), fits["valu"].view(torch.int32))
    ms = {name: [] for name in hs}
    fit = first.empty(n)
    for _ in range(ALTERNATIONS):
        for name, es in hs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(PER_SAMPLE):
                es.rollout(theta, init, fitness=fit)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / PER_SAMPLE)
    hz, source = engine_clock_hz()
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    tiles = (E + TILE_E - 1) // TILE_E
    waves = n * tiles
    per_simd = (waves + simds - 1) // simds
    floor_ms = KB * MFMA_CYCLES * CYCLES * per_simd / hz * 1e3
    print(f"{n} offspring x {E} episodes x {CYCLES} cycles (sigma {sigma}); {ALTERNATIONS} alternations, {PER_SAMPLE} rollouts per sample; "
          f"fitness of both forms bit-equal: {same}; mean fitness {fits['mfma'].mean().item():.3f}")
    print(f"  MFMA issue floor: {tiles} tile x {KB} k-blocks x {MFMA_CYCLES} cycles x {CYCLES} cycles of the episode x {per_simd} waves per SIMD "
          f"({waves} waves, {simds} SIMDs) at {hz / 1e6:.0f} MHz ({source}) = {floor_ms:.3f} ms")
    for name in hs:
        t = ms[name]
        med = statistics.median(t)
        print(f"  fc1 on the {name.upper():4s} median {med:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}   "
              f"{n * E * CYCLES / (med * 1e-3):.3e} env-steps/s   {med / CYCLES * 1e3:8.2f} us per cycle"
              + (f"   floor / time = {floor_ms / med:.3f}" if name == "mfma" else ""))
        print("    samples (ms): " + " ".join(f"{x:.3f}" for x in t))
    for es in hs.values():
        es.close()


print(f"device: {torch.cuda.get_device_name(0)}")
shape(256, 0.1)
shape(4096, 0.1)
