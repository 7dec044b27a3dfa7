#!/usr/bin/env python3
"""A sweep's simple_evolution / simple_genetic trials as one ragged population against one trial after the other.

  tail    end of the rollout -> next populations written, for R trials: ONE ses_elite_generation_batch call against R times the solo
          sequence of a per-generation run (rank_center, elite_select, perturb of the elite rows, [elite_mean], perturb of the next
          population), one handle each, device events around a synchronised window of ITERS rounds after warm-up; the two forms
          alternate window by window in this process, median and spread over REPS windows.  Shapes: simple_evolution 16 x 97 x 226
          (conf/cartpole.yaml), simple_genetic 16 x {95, 90, 90, 80, ...} x P of the walker MLP (sweep_config/bipedal_genetic.yaml's
          elite_num 5 / 10 / 15 / 20 at 96 offspring), and both at R = 1, where nothing is batched.
  sweeps  wall time of sweep_main.py --concurrent R against --concurrent 1 (the sequential path), alternating, SWEEP_REPS each:
          sweep_config/cartpole_genetic_grid.yaml (6 trials, --concurrent 6), and 16 trials of sweep_config/bipedal_genetic.yaml
          cut to 20 generations (--concurrent 16).  Process start and the first handle's code-object load are outside: one untimed
          warm-up sweep first.

Writes profiles/batch_elite_timing.txt.  Usage: time_batch_elite.py [--out FILE] [--tail-only | --sweeps-only] [--append]"""
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

CARTPOLE, WALKER = (4, 2, True, False), (24, 4, False, False)
# (strategy name, offspring_num, elite_num per trial, policy shape)
SHAPES = [("simple_evolution", 96, (10,) * 16, CARTPOLE), ("simple_genetic", 96, (5, 10, 15, 20) * 4, WALKER),
          ("simple_evolution", 96, (10,), CARTPOLE), ("simple_genetic", 96, (10,), WALKER)]
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


def tails(name, N, ks, shape):
    import numpy as np
    import torch
    from learning_strategies.evolution.batch import ELITE_STRATEGIES, ELITE_TRIAL_DTYPE
    from ses import BatchEliteLayout, HipES
    hs = {"batch": HipES(None, *shape), "solo": HipES(None, *shape)}
    es = hs["batch"]
    lay = BatchEliteLayout(ELITE_STRATEGIES[name], N, ks)
    R, P = lay.R, es.P
    fit = torch.rand(lay.rows_total, device=es.device)
    theta = es.empty(lay.rows_total, P)
    parents = {key: [h.zeros(lay.parents_total, P), h.zeros(lay.parents_total, P)] for key, h in hs.items()}
    alias = {key: (torch.ones(R, dtype=torch.int32, device=es.device) if lay.evolution else None) for key in hs}
    maps = [torch.from_numpy(lay.parent_map(r)).to(es.device) for r in range(R)]
    # the records of ITERS generations, uploaded once (BatchedRuns uploads a chunk of generations at a time)
    table = np.zeros((ITERS, R), dtype=ELITE_TRIAL_DTYPE)
    for g in range(ITERS):
        for r in range(R):
            table[g, r] = (1 + r, g, g + 1, np.float32(0.1), np.float32(0.1), lay.row0[r], lay.n[r], lay.elite_num[r], lay.parent0[r])
    trials = torch.from_numpy(table.view(np.uint8).reshape(ITERS, R, ELITE_TRIAL_DTYPE.itemsize)).to(es.device)

    def batch(g):
        a, b = parents["batch"]
        hs["batch"].elite_generation_batch(fit, lay, trials[g], a, b, alias_state=alias["batch"], theta_next=theta)
        parents["batch"] = [b, a]

    def solo(g):
        h = hs["solo"]
        a, b = parents["solo"]
        for r in range(R):
            row0, n, k, p0 = int(lay.row0[r]), int(lay.n[r]), int(lay.elite_num[r]), int(lay.parent0[r])
            rows_p = 1 if lay.evolution else k
            rank, _ = h.rank_center(fit[row0:row0 + n], want_weights=False)
            ids, sel, flags = h.elite_select(rank, k, maps[r], alias["solo"][r:r + 1] if lay.evolution else None)
            rows = h.perturb(a[p0:p0 + rows_p], 0.1, 1 + r, g, 0, k, parent_idx=sel, row_ids=ids, idx_in_range=True)
            new = h.elite_mean(rows, flags).view(1, -1) if lay.evolution else rows
            h.perturb(new, 0.1, 1 + r, g + 1, 0, n, parent_idx=maps[r], out=theta[row0:row0 + n], idx_in_range=True)

    calls = {"batch": batch, "solo": solo}
    for call in calls.values():
        window(call, 20)                                                # warm-up: code objects, scratch
    ts = {key: [] for key in calls}
    for _ in range(REPS):
        for key, call in calls.items():                                 # alternating
            ts[key].append(window(call, ITERS))
    for h in hs.values():
        h.close()
    return lay, P, {key: (statistics.median(v), min(v), max(v)) for key, v in ts.items()}


SWEEPS = {"cartpole": ("cartpole_genetic_grid.yaml", None, None, 6,
                       "sweep_config/cartpole_genetic_grid.yaml (6 trials: simple_evolution, 97 rows, 20 generations, 5 episodes)"),
          "walker20": ("bipedal_genetic.yaml", 20, 16, 16,
                       "sweep_config/bipedal_genetic.yaml --count 16, 20 generations (simple_genetic, 96 offspring: 80 .. 95 rows, 5 episodes)")}


def sweeps(names):
    import torch
    import yaml
    import sweep_main
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        files = {}
        for name in names:
            source, generations = SWEEPS[name][:2]
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
                count = SWEEPS[name][2]
                sys.argv = (["sweep_main.py", "--sweep", files[name], "--concurrent", str(concurrent)]
                            + (["--count", str(count)] if count else []))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    sweep_main.main()
                torch.cuda.synchronize()
                print(f"{name} --concurrent {concurrent}: {time.perf_counter() - t0:.3f} s", file=sys.stderr, flush=True)
                return time.perf_counter() - t0

            for name in names:
                R = SWEEPS[name][3]
                run(name, R)                                            # warm-up, untimed
                ts = {1: [], R: []}
                for _ in range(SWEEP_REPS):
                    for concurrent in (1, R):                           # alternating
                        ts[concurrent].append(run(name, concurrent))
                out[name] = {c: (statistics.median(v), min(v), max(v)) for c, v in ts.items()}
        finally:
            os.chdir(cwd)
            sys.argv = argv
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_elite_timing.txt"))
    ap.add_argument("--tail-only", action="store_true")
    ap.add_argument("--sweeps-only", action="store_true")
    ap.add_argument("--sweep", action="append", choices=sorted(SWEEPS), help="time this sweep only (repeatable)")
    ap.add_argument("--append", action="store_true", help="add to FILE instead of replacing it (the parts run as separate jobs)")
    args = ap.parse_args()
    import torch
    out = [] if args.append else [f"device: {torch.cuda.get_device_name(0)}"]
    if not args.sweeps_only:
        out += ["", f"tail of R ragged trials, us per round (median [min, max] of {REPS} windows of {ITERS} rounds, the forms alternating):",
                "  batch = one ses_elite_generation_batch call (3 launches), solo = R x (rank_center, elite_select, perturb, [elite_mean], perturb)"]
        for name, N, ks, shape in SHAPES:
            lay, P, r = tails(name, N, ks, shape)
            b, s = r["batch"], r["solo"]
            rows = f"{lay.n_max}" if lay.n_max == int(lay.n.min()) else f"{int(lay.n.min())}..{lay.n_max}"
            out.append(f"  {name:<16} R={lay.R:>2} n={rows:>6} rows={lay.rows_total:>4} P={P:>4}: batch {b[0]:8.2f} [{b[1]:.2f}, {b[2]:.2f}]"
                       f"   solo {s[0]:8.2f} [{s[1]:.2f}, {s[2]:.2f}]   batch / solo = {b[0] / s[0]:.3f}")
    if not args.tail_only:
        names = args.sweep or list(SWEEPS)
        out += ["", f"whole sweeps, wall seconds (median [min, max] of {SWEEP_REPS} runs each, alternating, after one untimed run):"]
        for name, r in sweeps(names).items():
            R = SWEEPS[name][3]
            a, b = r[1], r[R]
            out.append(f"  {SWEEPS[name][4]}:")
            out.append(f"    --concurrent 1  {a[0]:8.3f} [{a[1]:.3f}, {a[2]:.3f}]   --concurrent {R:<2} {b[0]:8.3f} [{b[1]:.3f}, {b[2]:.3f}]"
                       f"   sequential / concurrent = {a[0] / b[0]:.2f}")
    text = "\n".join(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
