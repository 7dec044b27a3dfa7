#!/usr/bin/env python3
"""A sweep's ars trials as one population against one trial after the other.

  tail    end of the rollout -> next populations written, for R trials: ONE ses_ars_generation_batch call (4 launches; 5 above 1024
          parameters) against R ses_ars_generation calls (R x 4 or R x 5 launches: what a sequential sweep issues per generation),
          one handle each, the calls issued from Python, device events around a synchronised window of ITERS rounds after warm-up;
          the two forms alternate window by window in this process, median and spread over REPS windows.  Shapes R x n x P:
          16 x 256 x 226 (conf/cartpole_ars.yaml), 16 x 96 x 6756 (the LunarLander GRU policy), 4 x 1024 x 226, and 1 x 256 x 226,
          where nothing is batched.  elite_num differs per trial.
  sweep   wall time of sweep_main.py --sweep sweep_config/cartpole_ars_grid.yaml (16 trials) --concurrent 16 against
          --concurrent 1 (the sequential path), alternating, SWEEP_REPS each.  Process start and the first handle's code-object load
          are outside: one untimed warm-up sweep of each first.

Writes profiles/batch_ars_timing.txt.  Usage: time_batch_ars.py [--out FILE] [--tail-only | --sweep-only] [--append]"""
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

CARTPOLE, LANDER_GRU = (4, 2, True, False), (8, 4, True, True)
SHAPES = [(16, 256, CARTPOLE), (16, 96, LANDER_GRU), (4, 1024, CARTPOLE), (1, 256, CARTPOLE)]       # (R, n, policy shape)
ITERS, REPS, SWEEP_REPS = 100, 9, 3
SWEEP, SWEEP_R = "cartpole_ars_grid.yaml", 16


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


def elite_nums(R, n):
    """n // 4 (the default) first, then other selections: the trials of a sweep over elite_num"""
    return [max(1, n // (4, 2, 32, 8)[r % 4]) for r in range(R)]


def tails(R, n, shape):
    import numpy as np
    import torch
    from learning_strategies.evolution.batch import ARS_TRIAL_DTYPE
    from ses import HipES
    hs = {"batch": HipES(None, *shape), "solo": HipES(None, *shape)}
    es = hs["batch"]
    P = es.P
    bs = elite_nums(R, n)
    lrs = [0.05 * (1 + r % 4) for r in range(R)]
    fit = torch.rand(R * n, device=es.device)
    theta = es.empty(R * n, P)
    state = {key: [(h.zeros(R, P),), (h.zeros(R, P),)] for key, h in hs.items()}
    # the records of ITERS generations, uploaded once (BatchedRuns uploads a chunk of generations at a time)
    table = np.zeros((ITERS, R), dtype=ARS_TRIAL_DTYPE)
    for g in range(ITERS):
        for r in range(R):
            table[g, r] = (1 + r, g, g + 1, lrs[r], np.float32(0.1), bs[r])
    trials = torch.from_numpy(table.view(np.uint8).reshape(ITERS, R, ARS_TRIAL_DTYPE.itemsize)).to(es.device)

    def batch(g):
        a, b = state["batch"]
        hs["batch"].ars_generation_batch(fit, n, bs, trials[g], a, b, theta_next=theta)
        state["batch"] = [b, a]

    def solo(g):
        h = hs["solo"]
        a, b = state["solo"]
        for r in range(R):
            h.ars_generation(fit[r * n:(r + 1) * n], bs[r], 1 + r, g, 0.1, lrs[r], (a[0][r],), (b[0][r],), 0.1, g + 1, 0, n,
                             theta_next=theta[r * n:(r + 1) * n])
        state["solo"] = [b, a]

    calls = {"batch": batch, "solo": solo}
    for call in calls.values():
        window(call, 20)                                                # warm-up: code objects, scratch
    ts = {key: [] for key in calls}
    for _ in range(REPS):
        for key, call in calls.items():                                 # alternating
            ts[key].append(window(call, ITERS))
    for h in hs.values():
        h.close()
    return P, {key: (statistics.median(v), min(v), max(v)) for key, v in ts.items()}


def sweep():
    import torch
    import yaml
    import sweep_main
    with tempfile.TemporaryDirectory() as tmp:
        spec = yaml.load(open(os.path.join(SRC, "sweep_config", SWEEP)), Loader=yaml.FullLoader)
        spec["parameters"]["cfg-path"]["value"] = os.path.join(SRC, spec["parameters"]["cfg-path"]["value"])
        path = os.path.join(tmp, SWEEP)
        with open(path, "w") as f:
            yaml.safe_dump(spec, f)
        cwd, argv = os.getcwd(), sys.argv
        os.chdir(tmp)                                                   # the runs make their logs/ directories where they start
        try:
            def run(concurrent):
                sys.argv = ["sweep_main.py", "--sweep", path, "--concurrent", str(concurrent)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    sweep_main.main()
                torch.cuda.synchronize()
                print(f"--concurrent {concurrent}: {time.perf_counter() - t0:.3f} s", file=sys.stderr, flush=True)
                return time.perf_counter() - t0

            run(SWEEP_R)                                                # warm-up, untimed
            run(1)
            ts = {1: [], SWEEP_R: []}
            for _ in range(SWEEP_REPS):
                for concurrent in (1, SWEEP_R):                         # alternating
                    ts[concurrent].append(run(concurrent))
            return {c: (statistics.median(v), min(v), max(v)) for c, v in ts.items()}
        finally:
            os.chdir(cwd)
            sys.argv = argv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_ars_timing.txt"))
    ap.add_argument("--tail-only", action="store_true")
    ap.add_argument("--sweep-only", action="store_true")
    ap.add_argument("--append", action="store_true", help="add to FILE instead of replacing it (the parts run as separate jobs)")
    args = ap.parse_args()
    import torch
    out = [] if args.append else [f"device: {torch.cuda.get_device_name(0)}"]
    if not args.sweep_only:
        out += ["", f"ars tail of R trials, us per round (median [min, max] of {REPS} windows of {ITERS} rounds, the forms alternating):",
                "  batch = one ses_ars_generation_batch call (4 launches; 5 above 1024 parameters), solo = R x ses_ars_generation "
                "(R x 4; R x 5)"]
        for R, n, shape in SHAPES:
            P, r = tails(R, n, shape)
            b, s = r["batch"], r["solo"]
            ahead = b[2] < s[1]                                         # every batch window under every solo window
            out.append(f"  R={R:>2} n={n:>4} P={P:>4}: batch {b[0]:8.2f} [{b[1]:.2f}, {b[2]:.2f}]   solo {s[0]:8.2f} [{s[1]:.2f}, {s[2]:.2f}]"
                       f"   batch / solo = {b[0] / s[0]:.3f}" + ("" if ahead else "   (not ahead by more than the repeat spread)"))
    if not args.tail_only:
        r = sweep()
        a, b = r[1], r[SWEEP_R]
        out += ["", f"whole sweep, wall seconds (median [min, max] of {SWEEP_REPS} runs each, alternating, after one untimed run of each):",
                f"  sweep_config/{SWEEP} (16 trials: ars, 256 offspring, 20 generations, 5 episodes):",
                f"    --concurrent 1  {a[0]:8.3f} [{a[1]:.3f}, {a[2]:.3f}]   --concurrent {SWEEP_R:<2} {b[0]:8.3f} [{b[1]:.3f}, {b[2]:.3f}]"
                f"   sequential / concurrent = {a[0] / b[0]:.2f}"]
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
