#!/usr/bin/env python3
"""The ars tail against the pgpe and the openai_es tails, and conf/cartpole_ars.yaml against the same population under openai_es.

  tail        end of the rollout -> next population written: ses_ars_generation (b = m / 2 and b = m / 8, m = n / 2 pairs),
              ses_pgpe_generation and ses_openai_generation on one handle each, whole population, device events around a
              synchronised window of ITERS calls after warm-up; the strategies alternate window by window in this process,
              median and spread over REPS windows.  Shapes (n, P): (256, 226), (4096, 226), (4096, 6756).
  generation  ESLoop.generations() ms per generation, conf/cartpole_ars.yaml and conf/cartpole_pgpe.yaml's openai_es twin
              (the same env, network and population), alternating, host clock around a window that ends in a device synchronise.

Writes profiles/ars_timing.txt: the resource usage of the kernels of csrc/ses_ars.hip (compiled here with
-Rpass-analysis=kernel-resource-usage; needs hipcc, not a GPU) followed by the timings (need the GPU).
Usage: time_ars.py [--out FILE] [--resources-only]"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
sys.path.insert(0, SRC)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_pgpe  # noqa: E402  (window(), SHAPES, ITERS, REPS and the compiler-remark reader)

SHAPES, ITERS, REPS = time_pgpe.SHAPES, time_pgpe.ITERS, time_pgpe.REPS


def resource_lines():
    """VGPRs / LDS / occupancy / scratch of every kernel of ses_ars.hip, from the compiler's remarks"""
    import re
    import subprocess
    build = open(os.path.join(SRC, "csrc", "build.sh")).read()
    flags = re.search(r"FLAGS=\((.*?)\)", build, flags=re.S).group(1).split()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(SRC, "csrc", "ses_ars.hip"),
                              "-o", os.path.join(tmp, "ses_ars.o")], capture_output=True, text=True)
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


def tails(n, P, shape):
    import torch
    from ses import HipES
    S, A, disc, gru = shape
    m = n // 2
    names = ("ars_b=m/2", "ars_b=m/8", "ars_b=m/2_unfolded", "pgpe", "openai_es")
    hs = {name: HipES(None, S, A, disc, gru) for name in names}
    assert hs["pgpe"].P == P
    hs["ars_b=m/2_unfolded"].set_tuning("ars_fused_apply_perturb", 0)   # the update as a launch of its own (what P > 1024 always does)
    fit = torch.rand(n, device=hs["pgpe"].device)
    calls = {}
    for name, es in hs.items():
        k = 1 if name.startswith("ars") else 3 if name == "openai_es" else 4
        a, b = [es.zeros(P) for _ in range(k)], [es.zeros(P) for _ in range(k)]
        if name == "pgpe":
            a[3].fill_(1.0)
        theta = es.empty(n, P)
        state = {"io": (a, b)}
        dirs = m // 8 if name == "ars_b=m/8" else m // 2

        def call(g, name=name, es=es, state=state, theta=theta, dirs=dirs):
            a, b = state["io"]
            if name.startswith("ars"):
                es.ars_generation(fit, dirs, 1, g, 0.1, 0.2, a, b, 0.1, g + 1, 0, n, theta_next=theta)
            elif name == "pgpe":
                es.pgpe_generation(fit, 1, g, 0.1, 0.05, 0.2, 0.2, (0.01, 100.0), a, b, 0.1, g + 1, 0, n, theta_next=theta)
            else:
                es.openai_generation(fit, 1, g, 0.05, 0.1, 0.05, a, b, 0.1, g + 1, 0, n, theta_next=theta)
            state["io"] = (b, a)
        calls[name] = call
    for call in calls.values():
        time_pgpe.window(call, 20)                                      # warm-up: code objects, scratch, the armed rank vector
    ts = {name: [] for name in calls}
    for _ in range(REPS):
        for name, call in calls.items():                                # alternating
            ts[name].append(time_pgpe.window(call, ITERS))
    for es in hs.values():
        es.close()
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ts.items()}


def generations(gens=400, reps=5):
    import torch
    import yaml
    import builder
    cfg = yaml.load(open(os.path.join(SRC, "conf", "cartpole_ars.yaml")), Loader=yaml.FullLoader)
    twin = {**cfg, "strategy": dict(name="openai_es", init_sigma=0.1, sigma_decay=1.0, learning_rate=0.05, offspring_num=256)}
    loops = {}
    with tempfile.TemporaryDirectory() as tmp:
        cwd = os.getcwd()
        os.chdir(tmp)                                                   # ESLoop makes its logs/ directory where it is built
        try:
            for name, c in (("ars", cfg), ("openai_es", twin)):
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ars_timing.txt"))
    ap.add_argument("--resources-only", action="store_true")
    args = ap.parse_args()
    out = ["kernel resource usage, csrc/ses_ars.hip for gfx950 (-Rpass-analysis=kernel-resource-usage):"] + resource_lines()
    if not args.resources_only:
        import torch
        out += ["", f"device: {torch.cuda.get_device_name(0)}",
                f"tail, us per call (median [min, max] of {REPS} windows of {ITERS} calls, the strategies alternating; m = n / 2 pairs):"]
        for n, P, shape in SHAPES:
            r = tails(n, P, shape)
            out.append(f"  n={n:>5} P={P:>5}:")
            for name, v in r.items():
                out.append(f"    {name:<20} {v[0]:7.2f} [{v[1]:.2f}, {v[2]:.2f}]   / pgpe = {v[0] / r['pgpe'][0]:.3f}")
        g = generations()
        out += ["", "ESLoop.generations(), conf/cartpole_ars.yaml against openai_es at the same population (256 offspring, 5 episodes), "
                    "ms per generation (median [min, max] of 5 windows of 400 generations, alternating; the two strategies learn at "
                    "different rates, so their episodes differ in length):"]
        for name in ("ars", "openai_es"):
            v = g[name]
            out.append(f"  {name:<10} {v[0]:.4f} [{v[1]:.4f}, {v[2]:.4f}]   device-side loop: {v[3]}")
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
