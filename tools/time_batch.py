#!/usr/bin/env python3
"""A sweep's trials as one population against one trial after the other.

  tail    end of the rollout -> next populations written, for R trials of n rows: ONE ses_openai_generation_batch call against R
          ses_openai_generation calls, one handle each, device events around a synchronised window of ITERS rounds after warm-up;
          the two forms alternate window by window in this process, median and spread over REPS windows.  Shapes R x n x P:
          16 x 256 x 226, 16 x 96 x 6756, 4 x 1024 x 226 and 1 x 256 x 226 (what the segmented form costs with nothing to batch).
  sweeps  wall time of sweep_main.py --concurrent 16 against --concurrent 1 (the sequential path), alternating, SWEEP_REPS each:
          sweep_config/cartpole_openaies.yaml --count 16, and 16 trials of sweep_config/lunarlander_openaies.yaml cut to 20
          generations.  Process start and the first handle's code-object load are outside: one untimed warm-up sweep first.

Writes profiles/batch_timing.txt.  Usage: time_batch.py [--out FILE] [--tail-only | --sweeps-only]"""
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

SHAPES = [(16, 256, 226, (4, 2, True, False)), (16, 96, 6756, (8, 4, False, True)), (4, 1024, 226, (4, 2, True, False)),
          (1, 256, 226, (4, 2, True, False))]
ITERS, REPS, SWEEP_REPS = 100, 9, 3


def window(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for g in range(iters):
        fn(g)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3                          # us per round of R trials


def tails(R, n, P, shape):
    import numpy as np
    import torch
    from learning_strategies.evolution.batch import TRIAL_DTYPE
    from ses import HipES
    hs = {"batch": HipES(None, *shape), "solo": HipES(None, *shape)}
    es = hs["batch"]
    assert es.P == P
    fit = torch.rand(R * n, device=es.device)
    theta = es.empty(R * n, P)
    io_ = {name: ([h.zeros(R, P) for _ in range(3)], [h.zeros(R, P) for _ in range(3)]) for name, h in hs.items()}
    # the records of ITERS + warm-up generations, uploaded once (BatchedRuns uploads a chunk of generations at a time)
    table = np.zeros((ITERS, R), dtype=TRIAL_DTYPE)
    for g in range(ITERS):
        for r in range(R):
            table[g, r] = (1 + r, g, g + 1, 0.05, np.float32(-(0.05 / (n * 0.1))), np.float32(0.1))
    trials = torch.from_numpy(table.view(np.uint8).reshape(ITERS, R, TRIAL_DTYPE.itemsize)).to(es.device)

    def batch(g):
        a, b = io_["batch"]
        hs["batch"].openai_generation_batch(fit, n, trials[g], a, b, theta_next=theta)
        io_["batch"] = (b, a)

    def solo(g):
        a, b = io_["solo"]
        for r in range(R):
            hs["solo"].openai_generation(fit[r * n:(r + 1) * n], 1 + r, g, 0.05, 0.1, 0.05, [x[r] for x in a], [x[r] for x in b], 0.1,
                                         g + 1, 0, n, theta_next=theta[r * n:(r + 1) * n])
        io_["solo"] = (b, a)

    calls = {"batch": batch, "solo": solo}
    for call in calls.values():
        window(call, 20)                                                # warm-up: code objects, scratch, the armed rank vector
    ts = {name: [] for name in calls}
    for _ in range(REPS):
        for name, call in calls.items():                                # alternating
            ts[name].append(window(call, ITERS))
    for h in hs.values():
        h.close()
    return {name: (statistics.median(v), min(v), max(v)) for name, v in ts.items()}


def sweeps():
    import torch
    import yaml
    import sweep_main
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        files = {}
        for name, source, generations in (("cartpole", "cartpole_openaies.yaml", None), ("lander20", "lunarlander_openaies.yaml", 20)):
            spec = yaml.load(open(os.path.join(SRC, "sweep_config", source)), Loader=yaml.FullLoader)
            spec["parameters"]["cfg-path"]["value"] = os.path.join(SRC, spec["parameters"]["cfg-path"]["value"])
            if generations is not None:
                spec["parameters"]["generation-num"]["value"] = generations
            files[name] = os.path.join(tmp, name + ".yaml")
            with open(files[name], "w") as f:
                yaml.safe_dump(spec, f)
        cwd, argv = os.getcwd(), sys.argv
        os.chdir(tmp)                                                   # the runs make their logs/ directories where they start
        try:
            def run(name, concurrent):
                sys.argv = ["sweep_main.py", "--sweep", files[name], "--count", "16", "--concurrent", str(concurrent)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    sweep_main.main()
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            for name in files:
                run(name, 16)                                           # warm-up, untimed
                ts = {1: [], 16: []}
                for _ in range(SWEEP_REPS):
                    for concurrent in (1, 16):                          # alternating
                        ts[concurrent].append(run(name, concurrent))
                out[name] = {c: (statistics.median(v), min(v), max(v)) for c, v in ts.items()}
        finally:
            os.chdir(cwd)
            sys.argv = argv
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_timing.txt"))
    ap.add_argument("--tail-only", action="store_true")
    ap.add_argument("--sweeps-only", action="store_true")
    args = ap.parse_args()
    import torch
    out = [f"device: {torch.cuda.get_device_name(0)}"]
    if not args.sweeps_only:
        out += ["", f"tail of R trials of n rows, us per round (median [min, max] of {REPS} windows of {ITERS} rounds, the forms alternating):",
                "  batch = one ses_openai_generation_batch call, solo = R ses_openai_generation calls"]
        for R, n, P, shape in SHAPES:
            r = tails(R, n, P, shape)
            b, s = r["batch"], r["solo"]
            out.append(f"  R={R:>2} n={n:>4} P={P:>4}: batch {b[0]:8.2f} [{b[1]:.2f}, {b[2]:.2f}]   solo {s[0]:8.2f} [{s[1]:.2f}, {s[2]:.2f}]"
                       f"   batch / solo = {b[0] / s[0]:.3f}")
    if not args.tail_only:
        out += ["", f"whole sweeps of 16 trials, wall seconds (median [min, max] of {SWEEP_REPS} runs each, alternating, after one untimed run):"]
        what = {"cartpole": "sweep_config/cartpole_openaies.yaml --count 16 (256 offspring, 30 generations, 5 episodes)",
                "lander20": "sweep_config/lunarlander_openaies.yaml --count 16, 20 generations (96 offspring, 5 episodes)"}
        for name, r in sweeps().items():
            a, b = r[1], r[16]
            out.append(f"  {what[name]}:")
            out.append(f"    --concurrent 1  {a[0]:8.3f} [{a[1]:.3f}, {a[2]:.3f}]   --concurrent 16 {b[0]:8.3f} [{b[1]:.3f}, {b[2]:.3f}]"
                       f"   sequential / concurrent = {a[0] / b[0]:.2f}")
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
