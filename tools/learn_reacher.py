#!/usr/bin/env python3
"""Learning curves on ReacherBulletEnv-v0 (csrc/ses_f64_envs.hip): the best and the population-mean return of every generation,
against the idle policy's 0.  Runs conf/reacher.yaml, conf/reacher_sep_cma.yaml and conf/reacher_ars.yaml, one seed each, 5 episodes per offspring,
generation by generation (SES_BATCH_GENERATIONS=0, so that every generation's fitness vector can be read); further arguments
`init_sigma:learning_rate` add runs of conf/reacher.yaml with those two keys changed (what was tried when tuning it),
`ars:init_sigma:learning_rate:elite_num` runs of conf/reacher_ars.yaml with those three, `ars` alone that config only;
`obs_norm` runs conf/reacher.yaml, conf/reacher_openai_norm.yaml, conf/reacher_ars.yaml and conf/reacher_ars_v2.yaml (each config
beside the same config with network.obs_normalizer) and nothing else, `obs_norm:init_sigma` the two normalised configs with
that init_sigma (profiles/obs_norm_learning.txt).  One line
per generation of conf/reacher.yaml itself: `config generation best mean`; after EVERY run a summary line with the final mean
(the mean of the last ten generations' population means), the first generation whose population mean passes half of it, and
the population mean of every 50th generation -- the other runs are recorded by their summaries alone.
usage: learn_reacher.py [generations] [seed] [init_sigma:learning_rate ...]
profiles/reacher_learning.txt is its output; profiles/ars_learning.txt holds the ars runs."""
import contextlib
import copy
import io
import os
import sys
import tempfile

os.environ["SES_BATCH_GENERATIONS"] = "0"
import yaml  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
sys.path.insert(0, SRC)
import builder  # noqa: E402


def load(conf):
    return yaml.load(open(os.path.join(SRC, "conf", conf + ".yaml")), Loader=yaml.FullLoader)


def run(label, cfg, generations, seed, per_generation=False):
    cfg = copy.deepcopy(cfg)
    cfg["strategy"]["seed"] = seed
    cfg["env"]["seed"] = seed
    loop = builder.build_loop(cfg, generations, 1, 5, False, 10 ** 9)
    means = []
    rollout = loop.rollout

    def recording(population):
        fitness = rollout(population)
        means.append(fitness.mean())                                    # stays on the device until the run is over
        return fitness

    loop.rollout = recording
    with contextlib.redirect_stdout(io.StringIO()):
        loop.run()
    best = [b for b, _ in loop.history]
    means = [float(m) for m in means]
    if per_generation:
        for g, (b, m) in enumerate(zip(best, means)):
            print(f"{label} {g} {b:.3f} {m:.3f}")
    final = sum(means[-10:]) / len(means[-10:])
    half = next((g for g, m in enumerate(means) if m > 0.5 * final), None) if final > 0.0 else None
    print(f"# {label}: idle 0; mean of generation 0 {means[0]:.3f}, final mean (last ten generations) {final:.3f}, first generation with "
          f"mean > half of it: {half}; max best {max(best):.3f}, last best {best[-1]:.3f}; mean of every 50th generation "
          + " ".join(f"{m:.2f}" for m in means[::50]) + "; best of every 50th generation " + " ".join(f"{b:.2f}" for b in best[::50]),
          flush=True)


def main():
    generations = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    os.chdir(tempfile.mkdtemp())                                        # the loop writes its metrics and checkpoints here
    base = load("reacher")
    args = sys.argv[3:]
    if any(a.startswith("obs_norm") for a in args):
        for arg in args:
            if arg == "obs_norm":
                for conf in ("reacher", "reacher_openai_norm", "reacher_ars", "reacher_ars_v2"):
                    run(conf, load(conf), generations, seed)
            elif arg.startswith("obs_norm:"):
                sigma = float(arg.split(":")[1])
                for conf in ("reacher_openai_norm", "reacher_ars_v2"):
                    cfg = load(conf)
                    cfg["strategy"]["init_sigma"] = sigma
                    run(f"{conf}[init_sigma={sigma:g}]", cfg, generations, seed)
        return
    if "ars" not in args:
        run("reacher", base, generations, seed, per_generation=True)
        run("reacher_sep_cma", load("reacher_sep_cma"), generations, seed)
    if "ars" in args or not args:
        run("reacher_ars", load("reacher_ars"), generations, seed, per_generation="ars" in args)
    for arg in args:
        if arg == "ars":
            continue
        if arg.startswith("ars:"):
            sigma, lr, b = arg.split(":")[1:]
            cfg = load("reacher_ars")
            cfg["strategy"].update(init_sigma=float(sigma), learning_rate=float(lr), elite_num=int(b))
            run(f"reacher_ars[init_sigma={sigma},learning_rate={lr},elite_num={b}]", cfg, generations, seed)
            continue
        sigma, lr = (float(v) for v in arg.split(":"))
        cfg = copy.deepcopy(base)
        cfg["strategy"]["init_sigma"], cfg["strategy"]["learning_rate"] = sigma, lr
        run(f"reacher[init_sigma={sigma:g},learning_rate={lr:g}]", cfg, generations, seed)


if __name__ == "__main__":
    main()
