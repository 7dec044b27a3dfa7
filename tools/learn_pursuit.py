#!/usr/bin/env python3
"""Learning curves of conf/pursuit.yaml (csrc/ses_pursuit.hip): openai_es, 256 offspring x 5 episodes x 500 cycles, the best and the
mean return of every generation, for four (init_sigma, learning_rate) pairs, generation by generation (SES_BATCH_GENERATIONS=0, so
that every generation's fitness vector can be read).  The pair the config carries is the one with the highest mean return over
the last ten generations.
usage: learn_pursuit.py [generations=40] [seed=0]  >  profiles/pursuit_learning.txt"""
import contextlib
import copy
import io
import os
import sys
import tempfile

os.environ["SES_BATCH_GENERATIONS"] = "0"
import torch  # noqa: E402
import yaml  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
sys.path.insert(0, SRC)
import builder  # noqa: E402

PAIRS = ((0.1, 0.05), (0.1, 0.2), (0.5, 0.05), (0.5, 0.2))


def run(cfg, generations, seed, sigma, lr):
    cfg = copy.deepcopy(cfg)
    cfg["strategy"].update(init_sigma=sigma, learning_rate=lr, seed=seed)
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
    print(f"\ninit_sigma {sigma}, learning_rate {lr}, sigma_decay {cfg['strategy']['sigma_decay']}")
    print("  gen   best return   mean return")
    for g, (b, m) in enumerate(zip(best, means)):
        print(f"  {g:3d}  {b:12.3f}  {m:12.3f}")
    tail = sum(means[-10:]) / len(means[-10:])
    print(f"  mean return, first generation {means[0]:.3f}, mean of the last ten {tail:.3f}; best return, first {best[0]:.3f}, last {best[-1]:.3f}",
          flush=True)
    return tail


def main():
    generations = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    cfg = yaml.load(open(os.path.join(SRC, "conf", "pursuit.yaml")), Loader=yaml.FullLoader)
    os.chdir(tempfile.mkdtemp())                                        # the loop writes its metrics and checkpoints here
    print(f"device: {torch.cuda.get_device_name(0)}")
    print(f"conf/pursuit.yaml: openai_es, 256 offspring x 5 episodes x 500 cycles, {generations} generations; return = the team's undiscounted sum "
          "over an episode (an idle team gets -0.8 a cycle: -400)")
    print("ESLoop.run() of the config per (init_sigma, learning_rate) pair; best = the generation's best fitness (loop.history), mean = the mean "
          "of the fitness vector its rollout returned.")
    tails = {pair: run(cfg, generations, seed, *pair) for pair in PAIRS}
    pick = max(tails, key=tails.get)
    print(f"\nhighest mean return over the last ten generations: init_sigma {pick[0]}, learning_rate {pick[1]} ({tails[pick]:.3f}); "
          f"the config carries init_sigma {cfg['strategy']['init_sigma']}, learning_rate {cfg['strategy']['learning_rate']}")


if __name__ == "__main__":
    main()
