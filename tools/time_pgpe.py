#!/usr/bin/env python3
"""The pgpe tail against the openai_es tail, and conf/cartpole_pgpe.yaml against the same config under openai_es.

  tail        end of the rollout -> next population written: ses_pgpe_generation and ses_openai_generation on one handle each,
              whole population, device events around a synchronised window of ITERS calls after warm-up; the two strategies
              alternate window by window in this process, median and spread over REPS windows.  Shapes (n, P): (256, 226),
              (4096, 226), (4096, 6756).
  generation  ESLoop.generations() ms per generation, conf/cartpole_pgpe.yaml and the same file with strategy.name = openai_es,
              alternating, host clock around a window that ends in a device synchronise.

Writes profiles/pgpe_timing.txt: the resource usage of the kernels of csrc/ses_pgpe.hip (compiled here with
-Rpass-analysis=kernel-resource-usage; needs hipcc, not a GPU) followed by the timings (need the GPU).
--tail-only: the tail windows alone, no file (the run to put under `rocprofv3 --kernel-trace --stats`, in a call of its own).
Usage: time_pgpe.py [--out FILE] [--resources-only | --tail-only]"""
import argparse
import contextlib
import io
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

SHAPES = [(256, 226, (4, 2, True, False)), (4096, 226, (4, 2, True, False)), (4096, 6756, (8, 4, False, True))]
ITERS, REPS = 200, 9


def resource_lines():
    """VGPRs / LDS / occupancy / scratch of every kernel of ses_pgpe.hip, from the compiler's remarks"""
    build = open(os.path.join(SRC, "csrc", "build.sh")).read()
    flags = re.search(r"FLAGS=\((.*?)\)", build, flags=re.S).group(1).split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(SRC, "csrc", "ses_pgpe.hip"),
                              "-o", os.path.join(tmp, "ses_pgpe.o")], capture_output=True, text=True)
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
    from ses import HipES
    S, A, disc, gru = shape
    hs = {"pgpe": HipES(None, S, A, disc, gru), "openai_es": HipES(None, S, A, disc, gru), "pgpe_unfolded": HipES(None, S, A, disc, gru)}
    assert hs["pgpe"].P == P
    hs["pgpe_unfolded"].set_tuning("pgpe_fused_apply_perturb", 0)       # the update as a launch of its own (what P > 1024 always does)
    fit = torch.rand(n, device=hs["pgpe"].device)
    calls = {}
    for name, es in hs.items():
        k = 3 if name == "openai_es" else 4
        a, b = [es.zeros(P) for _ in range(k)], [es.zeros(P) for _ in range(k)]
        if name != "openai_es":
            a[3].fill_(1.0)
        theta = es.empty(n, P)
        state = {"io": (a, b)}

        def call(g, name=name, es=es, state=state, theta=theta):
            a, b = state["io"]
            if name != "openai_es":
                es.pgpe_generation(fit, 1, g, 0.1, 0.05, 0.2, 0.2, (0.01, 100.0), a, b, 0.1, g + 1, 0, n, theta_next=theta)
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
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ts.items()}


def generations(gens=400, reps=5):
    import torch
    import yaml
    import builder
    cfg = yaml.load(open(os.path.join(SRC, "conf", "cartpole_pgpe.yaml")), Loader=yaml.FullLoader)
    loops = {}
    with tempfile.TemporaryDirectory() as tmp:
        cwd = os.getcwd()
        os.chdir(tmp)                                                   # ESLoop makes its logs/ directory where it is built
        try:
            for name in ("pgpe", "openai_es"):
                c = {**cfg, "strategy": {k: v for k, v in cfg["strategy"].items() if name == "pgpe" or k != "sigma_learning_rate"}}
                c["strategy"]["name"] = name
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pgpe_timing.txt"))
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--tail-only", action="store_true")
    args = ap.parse_args()
    if args.tail_only:
        for n, P, shape in SHAPES:
            print(n, P, tails(n, P, shape))
        return
    out = ["kernel resource usage, csrc/ses_pgpe.hip for gfx950 (-Rpass-analysis=kernel-resource-usage):"] + resource_lines()
    if not args.resources_only:
        import torch
        out += ["", f"device: {torch.cuda.get_device_name(0)}",
                f"tail, us per call (median [min, max] of {REPS} windows of {ITERS} calls, the strategies alternating):"]
        for n, P, shape in SHAPES:
            r = tails(n, P, shape)
            p, o, u = r["pgpe"], r["openai_es"], r["pgpe_unfolded"]
            out.append(f"  n={n:>5} P={P:>5}: pgpe {p[0]:7.2f} [{p[1]:.2f}, {p[2]:.2f}]   openai_es {o[0]:7.2f} [{o[1]:.2f}, {o[2]:.2f}]"
                       f"   pgpe / openai_es = {p[0] / o[0]:.3f}   (pgpe, update as a launch of its own: {u[0]:.2f} [{u[1]:.2f}, {u[2]:.2f}])")
        g = generations()
        out += ["", "ESLoop.generations(), conf/cartpole_pgpe.yaml (256 offspring, 5 episodes), ms per generation "
                    "(median [min, max] of 5 windows of 400 generations, alternating):"]
        for name in ("pgpe", "openai_es"):
            v = g[name]
            out.append(f"  {name:<10} {v[0]:.4f} [{v[1]:.4f}, {v[2]:.4f}]   device-side loop: {v[3]}")
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
