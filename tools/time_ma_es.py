#!/usr/bin/env python3
"""The ma_es tail against the lm_ma_es, sep_cma_es and openai_es tails, and conf/cartpole_ma_es.yaml against
conf/cartpole_lm_ma.yaml.

  tail        end of the rollout -> next population written: ses_maes_generation (M = I + 0.3 randn / sqrt(P), D of the evaluated
              population handed in and D of the next one written, as ses_run_generations calls it), ses_lmma_generation (all m
              vectors active), ses_sepcma_generation and ses_openai_generation on one handle each, whole population, device events
              around a synchronised window of ITERS calls after warm-up; the strategies alternate window by window in this process,
              median and spread over REPS windows.  Two more windows time ses_perturb_maes alone (theta and D of the same
              population) and ses_maes_generation with d_in = NULL (the replicated tail of a sharded run: one more launch).
              Shapes (n, P): (256, 226), (4096, 226), (4096, 932).
  generation  ESLoop.generations() ms per generation, conf/cartpole_ma_es.yaml and conf/cartpole_lm_ma.yaml, alternating, host
              clock around a window that ends in a device synchronise.

Writes profiles/ma_es_timing.txt: the resource usage of the kernels of csrc/ses_maes.hip (compiled here with
-Rpass-analysis=kernel-resource-usage; needs hipcc, not a GPU) followed by the timings (need the GPU).
--tail-only: the tail windows alone, no file (the run to put under `rocprofv3 --kernel-trace --stats`, in a call of its own).
Usage: time_ma_es.py [--out FILE] [--resources-only | --tail-only]"""
import argparse
import contextlib
import io
import math
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
sys.path.insert(0, SRC)

SHAPES = [(256, 226, (4, 2, True, False)), (4096, 226, (4, 2, True, False)), (4096, 932, (24, 4, False, False))]
ITERS, REPS = 200, 9
NAMES = ("ma_es", "lm_ma_es", "sep_cma_es", "openai_es", "perturb_maes", "ma_es_no_d")


def resource_lines():
    """VGPRs / LDS / occupancy / scratch of every kernel of ses_maes.hip, from the compiler's remarks"""
    build = open(os.path.join(SRC, "csrc", "build.sh")).read()
    flags = re.search(r"FLAGS=\((.*?)\)", build, flags=re.S).group(1).split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(SRC, "csrc", "ses_maes.hip"),
                              "-o", os.path.join(tmp, "ses_maes.o")], capture_output=True, text=True)
    if out.returncode != 0:
        raise SystemExit(out.stderr)
    lines, name = [], None
    for l in out.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", l)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip().split("(")[0].replace("void ", "") or m.group(1)
            lines.append([name])
        m = re.search(r"remark:\s+(VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|VGPRs Spill|SGPRs Spill|"
                      r"LDS Size \[bytes/block\]): (\d+)", l)
        if m and name:
            lines[-1].append(f"{m.group(1)} {m.group(2)}")
    return ["  " + row[0] + ": " + ", ".join(row[1:]) for row in lines]


def window(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for g in range(iters):
        fn(g)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3                          # us per call


def tails(n, P, shape):
    import torch
    from ses import HipES, _lib
    from learning_strategies.evolution.offspring_strategies import (lm_ma_constants, lm_ma_params, ma_es_constants, ma_es_params,
                                                                    sep_cma_constants)
    S, A, disc, gru = shape
    hs = {name: HipES(None, S, A, disc, gru) for name in NAMES}
    assert hs["ma_es"].P == P
    fit = torch.rand(n, device=hs["ma_es"].device)
    c, w = sep_cma_constants(n, P, n // 2)
    params = _lib.SesSepcmaParams(c["mu"], 0, c["mueff"], c["c_sigma"], c["d_sigma"], c["c_c"], c["c_1"], c["c_mu"], c["chi"],
                                  0.01, 100.0, 1e-6, 1e6)
    lc, _ = lm_ma_constants(n, P, n // 2)
    lparams, m = lm_ma_params(lc, (1e-6, 1e6)), lc["m"]
    mparams = ma_es_params(ma_es_constants(n, P, n // 2)[0], (1e-6, 1e6))
    weights = torch.from_numpy(w).to(fit.device)
    hsig = 1.0 / (1.0 - (1.0 - c["c_sigma"]) ** 40.0) ** 0.5
    gen = torch.Generator(device="cpu").manual_seed(n + P)
    calls = {}
    for name, es in hs.items():
        if name in ("ma_es", "perturb_maes", "ma_es_no_d"):
            M = (torch.eye(P) + 0.3 * torch.randn(P, P, generator=gen) / math.sqrt(P)).to(es.device)
            a, b = ([es.zeros(P), es.zeros(P), M.clone(), es.zeros(1) + 1.0] for _ in range(2))
            state = {"io": (a, b), "D": (es.zeros(n, P), es.zeros(n, P))}
        elif name == "lm_ma_es":
            a, b = ([es.zeros(P), es.zeros(P), torch.randn(m, P, generator=gen).to(es.device), es.zeros(1) + 1.0] for _ in range(2))
            state = {"io": (a, b)}
        elif name == "sep_cma_es":
            a, b = ([es.zeros(P) for _ in range(4)] + [es.zeros(1)] for _ in range(2))
            a[1].fill_(1.0)
            a[4].fill_(1.0)
            state = {"io": (a, b)}
        else:
            state = {"io": ([es.zeros(P) for _ in range(3)], [es.zeros(P) for _ in range(3)])}
        theta = es.empty(n, P)

        def call(g, name=name, es=es, state=state, theta=theta):
            a, b = state["io"]
            if name in ("ma_es", "ma_es_no_d"):
                d_in, d_out = state["D"]
                es.maes_generation(fit, 1, g, 0.1, mparams, weights, a, b, d_in if name == "ma_es" else None, 0.1, g + 1, 0, n,
                                   theta_next=theta, d_next_out=d_out)
                state["D"] = (d_out, d_in)
            elif name == "perturb_maes":
                es.perturb_maes(a[0], a[2], a[3], 0.1, 1, g, 0, n, out=theta, d_out=state["D"][0])
                return
            elif name == "lm_ma_es":
                es.lmma_generation(fit, 1, g, 0.1, lparams, weights, m, m, a, b, 0.1, g + 1, 0, n, theta_next=theta)
            elif name == "sep_cma_es":
                es.sepcma_generation(fit, 1, g, 0.1, hsig, params, weights, a, b, 0.1, g + 1, 0, n, theta_next=theta)
            else:
                es.openai_generation(fit, 1, g, 0.05, 0.1, 0.05, a, b, 0.1, g + 1, 0, n, theta_next=theta)
            state["io"] = (b, a)
        calls[name] = call
    for call in calls.values():
        window(call, 20)                                                # warm-up: code objects, scratch, the armed rank vector
    ts = {name: [] for name in calls}
    for _ in range(REPS):
        for name, call in calls.items():                                # alternating
            ts[name].append(window(call, ITERS))
    for es in hs.values():
        es.close()
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ts.items()}, m


def generations(gens=400, reps=5):
    import torch
    import yaml
    import builder
    cfgs = {"ma_es": yaml.load(open(os.path.join(SRC, "conf", "cartpole_ma_es.yaml")), Loader=yaml.FullLoader),
            "lm_ma_es": yaml.load(open(os.path.join(SRC, "conf", "cartpole_lm_ma.yaml")), Loader=yaml.FullLoader)}
    loops = {}
    with tempfile.TemporaryDirectory() as tmp:
        cwd = os.getcwd()
        os.chdir(tmp)                                                   # ESLoop makes its logs/ directory where it is built
        try:
            for name, c in cfgs.items():
                with contextlib.redirect_stdout(io.StringIO()):
                    loop = builder.build_loop(c, 1, 1, 5, False, 10 ** 9)
                pop = loop.offspring_strategy.init_offspring(loop.network, loop.env.get_agent_ids())
                loops[name] = [loop, loop.generations(pop, 64)]         # warm-up
            torch.cuda.synchronize()
            ts = {name: [] for name in loops}
            for _ in range(reps):
                for name, item in loops.items():
                    t0 = time.perf_counter()
                    item[1] = item[0].generations(item[1], gens)
                    torch.cuda.synchronize()
                    ts[name].append((time.perf_counter() - t0) / gens * 1e3)
            device_side = {name: item[0].device_side_loop for name, item in loops.items()}
        finally:
            os.chdir(cwd)
    return {name: (statistics.median(v), min(v), max(v), device_side[name]) for name, v in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ma_es_timing.txt"))
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--tail-only", action="store_true")
    args = ap.parse_args()
    if args.tail_only:
        for n, P, shape in SHAPES:
            print(n, P, tails(n, P, shape))
        return
    out = ["kernel resource usage, csrc/ses_maes.hip for gfx950 (-Rpass-analysis=kernel-resource-usage):"] + resource_lines()
    if not args.resources_only:
        import torch
        out += ["", f"device: {torch.cuda.get_device_name(0)}",
                f"tail, us per call (median [min, max] of {REPS} windows of {ITERS} calls, the strategies alternating; lm_ma_es with all m "
                "vectors active; ma_es with D handed in, and with d_in = NULL):"]
        for n, P, shape in SHAPES:
            r, m = tails(n, P, shape)
            out.append(f"  n={n:>5} P={P:>4} (lm_ma_es m={m}):")
            for name in NAMES:
                v = r[name]
                label = {"perturb_maes": "ses_perturb_maes alone", "ma_es_no_d": "ma_es, d_in = NULL"}.get(name, name)
                out.append(f"    {label:<24} {v[0]:8.2f} [{v[1]:.2f}, {v[2]:.2f}]")
            out.append(f"    ma_es / lm_ma_es = {r['ma_es'][0] / r['lm_ma_es'][0]:.3f}   ma_es / openai_es = {r['ma_es'][0] / r['openai_es'][0]:.3f}"
                       f"   lm_ma_es / openai_es = {r['lm_ma_es'][0] / r['openai_es'][0]:.3f}")
        g = generations()
        out += ["", "ESLoop.generations(), conf/cartpole_ma_es.yaml against conf/cartpole_lm_ma.yaml (256 offspring, 5 episodes), "
                    "ms per generation (median [min, max] of 5 windows of 400 generations, alternating):"]
        for name in ("ma_es", "lm_ma_es"):
            v = g[name]
            out.append(f"  {name:<10} {v[0]:.4f} [{v[1]:.4f}, {v[2]:.4f}]   device-side loop: {v[3]}")
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
