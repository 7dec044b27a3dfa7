#!/usr/bin/env python3
"""Learning curves on the inverted-pendulum family (csrc/ses_f64_envs.hip): the best and the mean return of every generation.
Runs the seven conf/pendulum_swingup*.yaml (openai_es, pgpe, sep_cma_es, lm_ma_es, ma_es, ars, and ars with the observation
normaliser: pendulum_swingup_ars_v2, profiles/obs_norm_learning.txt), simple_evolution and simple_genetic
on the same env, network and population (256 offspring, the 32 best kept), and conf/inverted_pendulum.yaml and
conf/double_pendulum.yaml, one seed each, 5 episodes per offspring, generation by generation (SES_BATCH_GENERATIONS=0, so that
every generation's fitness vector can be read).  One line per generation: `config generation best mean`; after each run a
summary line `# config: first generation with best > 0 / >= 1000, the last best`.
Further arguments name the runs to make (e.g. `pendulum_swingup_ars`; none: all of them); `pendulum_swingup_ars:init_sigma:
learning_rate:elite_num` is that config with the three keys changed (what was tried when choosing them).
usage: learn_pendula.py [generations] [seed] [run ...]
profiles/pendula_learning.txt is its output; profiles/ars_learning.txt holds the ars runs."""
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

SWINGUP = ("pendulum_swingup", "pendulum_swingup_pgpe", "pendulum_swingup_sep_cma", "pendulum_swingup_lm_ma", "pendulum_swingup_ma_es",
           "pendulum_swingup_ars", "pendulum_swingup_ars_v2")
ELITE = {"simple_evolution": dict(name="simple_evolution", init_sigma=0.5, sigma_decay=0.999, elite_num=32, offspring_num=256),
         "simple_genetic": dict(name="simple_genetic", init_sigma=0.5, sigma_decay=0.999, elite_num=32, offspring_num=256)}


def load(conf):
    return yaml.load(open(os.path.join(SRC, "conf", conf + ".yaml")), Loader=yaml.FullLoader)


def run(label, cfg, generations, seed):
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
    for g, (b, m) in enumerate(zip(best, means)):
        print(f"{label} {g} {b:.3f} {float(m):.3f}")
    up = next((g for g, b in enumerate(best) if b > 0.0), None)
    full = next((g for g, b in enumerate(best) if b >= 1000.0), None)
    print(f"# {label}: first generation with best > 0: {up}, with best >= 1000: {full}, max best {max(best):.3f}, last best {best[-1]:.3f}, "
          f"last mean {float(means[-1]):.3f}", flush=True)


def main():
    generations = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    only = sys.argv[3:]
    os.chdir(tempfile.mkdtemp())                                        # the loop writes its metrics and checkpoints here
    for conf in SWINGUP:
        if not only or conf in only:
            run(conf, load(conf), generations, seed)
    base = load("pendulum_swingup")
    for name, strategy in ELITE.items():
        if not only or "pendulum_swingup_" + name in only:
            run("pendulum_swingup_" + name, dict(base, strategy=strategy), generations, seed)
    for conf in ("inverted_pendulum", "double_pendulum"):
        if not only or conf in only:
            run(conf, load(conf), generations, seed)
    for arg in only:
        if arg.startswith("pendulum_swingup_ars:"):
            sigma, lr, b = arg.split(":")[1:]
            cfg = load("pendulum_swingup_ars")
            cfg["strategy"].update(init_sigma=float(sigma), learning_rate=float(lr), elite_num=int(b))
            run(f"pendulum_swingup_ars[init_sigma={sigma},learning_rate={lr},elite_num={b}]", cfg, generations, seed)


if __name__ == "__main__":
    main()
