#!/usr/bin/env python3
"""Rollout time of pursuit (csrc/ses_pursuit.hip) with its 147-wide fc1 on the matrix cores and on the VALU ("pursuit_fc1_mfma"
1 / 0), alternating in one process, at 256 and 4096 offspring x 5 episodes x 500 cycles with first-generation populations (one
team cycle = one env-step).  Next to each time: the MFMA issue floor of the shape's fc1 -- tiles per offspring x 74 k-blocks x 64
cycles per v_mfma_f32_32x32x2_f32 x cycles of the episode x waves per SIMD, at the engine clock -- and each form's share of it
(floor / time).  The output is headed by the resource usage of the unit's kernels from the compiler's remarks.

    python tools/time_pursuit.py [--alternations 5] [--per-sample 2] [--resources-only | --timing-only]  >  profiles/pursuit_timing.txt

--resources-only needs hipcc and no GPU; --timing-only needs the GPU and no compiler.  A sample is `per-sample` back-to-back
rollouts between two device events; both forms are warmed first and their fitness vectors and step counts compared bit for bit."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
sys.path.insert(0, SRC)

E, CYCLES, TILE_E, KB, MFMA_CYCLES = 5, 500, 4, 74, 64


def resource_lines():
    """VGPRs / LDS / occupancy / scratch of every kernel of ses_pursuit.hip, from the compiler's remarks"""
    build = open(os.path.join(SRC, "csrc", "build.sh")).read()
    flags = re.search(r"FLAGS=\((.*?)\)", build, flags=re.S).group(1).split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(SRC, "csrc", "ses_pursuit.hip"),
                              "-o", os.path.join(tmp, "ses_pursuit.o")], capture_output=True, text=True)
    if out.returncode != 0:
        raise SystemExit(out.stderr)
    lines, name = [], None
    for l in out.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", l)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip().split("(")[0] or m.group(1)
            lines.append([name])
        m = re.search(r"remark:\s+(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|SGPRs Spill|"
                      r"LDS Size \[bytes/block\]): (\d+)", l)
        if m and name:
            lines[-1].append(f"{m.group(1)} {m.group(2)}")
    return ["  " + row[0] + ": " + ", ".join(row[1:]) for row in lines]


def engine_clock_hz(torch):
    """(Hz, where it comes from): the clock sampled now if the driver interface answers, else the device's rated peak"""
    try:
        return torch.cuda.clock_rate() * 1e6, "sampled after the timed runs (torch.cuda.clock_rate)"
    except Exception:
        return torch.cuda.get_device_properties(0).clock_rate * 1e3, "the device's rated peak (not sampled)"


def shape(torch, n, sigma, alternations, per_sample):
    from ses import HipES
    forms = {"mfma": 1, "valu": 0}
    hs = {}
    for name, knob in forms.items():
        hs[name] = HipES("pursuit", 147, 5, True, False, max_step=CYCLES, eval_ep_num=E, n_agents=8)
        hs[name].set_tuning("pursuit_fc1_mfma", knob)
    first = hs["mfma"]
    theta = first.perturb(first.zeros(first.P), sigma, 0, 0, 0, n)
    init = first.init_states_uniform(0, 0, 0, n)
    warm = {name: es.rollout(theta, init, want_episodes=True) for name, es in hs.items()}    # warm-up
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(warm["mfma"], warm["valu"]))
    steps = warm["mfma"][2]
    ms = {name: [] for name in hs}
    fit = first.empty(n)
    for _ in range(alternations):
        for name, es in hs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per_sample):
                es.rollout(theta, init, fitness=fit)
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / per_sample)
    hz, source = engine_clock_hz(torch)
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    tiles = (E + TILE_E - 1) // TILE_E
    waves = n * tiles
    per_simd = (waves + simds - 1) // simds
    floor_ms = KB * MFMA_CYCLES * CYCLES * per_simd / hz * 1e3
    env_steps = int(steps.sum().item())
    print(f"{n} offspring x {E} episodes x {CYCLES} cycles (sigma {sigma}); {alternations} alternations, {per_sample} rollouts per sample; "
          f"results of both forms bit-equal: {same}; mean fitness {warm['mfma'][0].mean().item():.3f}; cycles played {env_steps} of "
          f"{n * E * CYCLES} ({int((steps < CYCLES).sum().item())} episodes ended early)")
    print(f"  MFMA issue floor of fc1: {tiles} tiles x {KB} k-blocks x {MFMA_CYCLES} cycles x {CYCLES} cycles of the episode x {per_simd} waves "
          f"per SIMD ({waves} waves, {simds} SIMDs) at {hz / 1e6:.0f} MHz ({source}) = {floor_ms:.3f} ms")
    for name in hs:
        t = ms[name]
        med = statistics.median(t)
        print(f"  fc1 on the {name.upper():4s} median {med:9.3f} ms  min {min(t):9.3f}  max {max(t):9.3f}   "
              f"{env_steps / (med * 1e-3):.3e} env-steps/s   {med / CYCLES * 1e3:8.2f} us per cycle   floor / time = {floor_ms / med:.3f}")
        print("    samples (ms): " + " ".join(f"{x:.3f}" for x in t))
    for es in hs.values():
        es.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=5)
    ap.add_argument("--per-sample", type=int, default=2)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--timing-only", action="store_true")
    args = ap.parse_args()
    if not args.timing_only:
        print("kernel resource usage, csrc/ses_pursuit.hip for gfx950 (-Rpass-analysis=kernel-resource-usage):")
        print("\n".join(resource_lines()))
    if not args.resources_only:
        import torch
        print(f"device: {torch.cuda.get_device_name(0)}")
        shape(torch, 256, 0.1, args.alternations, args.per_sample)
        shape(torch, 4096, 0.1, args.alternations, args.per_sample)


if __name__ == "__main__":
    main()
