#!/usr/bin/env python3
"""Learning curves on HopperBulletEnv-v0 (csrc/ses_hopper.hip): conf/hopper.yaml, conf/hopper_ars.yaml and conf/hopper_sep_cma.yaml,
one seed each, 5 episodes per offspring, generation by generation (SES_BATCH_GENERATIONS=0, so that every generation's fitness
vector can be read).  Per run one summary line: the population mean and the best return at generations 0 / 50 / 150 / last, and
what the final mean policy (the strategy's elite model) does in one playback episode on the wrapper: its return, its length and
the distance its torso travels (the first float of the state blob is the torso's x).
For scale: the zero policy stands for 32 - 77 steps and collects about +0.8 per step (alive 1, joints at limit -0.2).
usage: learn_hopper.py [generations] [seed] [config ...]
profiles/hopper_learning.txt is its output."""
import contextlib
import copy
import io
import os
import sys
import tempfile

os.environ["SES_BATCH_GENERATIONS"] = "0"
import numpy as np  # noqa: E402
import yaml  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")
sys.path.insert(0, SRC)
import builder  # noqa: E402


def load(conf):
    return yaml.load(open(os.path.join(SRC, "conf", conf + ".yaml")), Loader=yaml.FullLoader)


def playback(env, net):
    """one episode of the reference's test.py loop on the wrapper: (return, steps, torso x at the end)"""
    net.eval()
    net.reset()
    obs = env.reset()
    done, total, steps = False, 0.0, 0
    while not done:
        obs, r, done, _ = env.step({"0": net(obs["0"]["state"][np.newaxis, ...])})
        total += r
        steps += 1
    x = float(env.state_blob().cpu().numpy().view(np.float32)[0, 0])
    return total, steps, x


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
    means = [float(m) for m in means]
    at = sorted({g for g in (0, 50, 150, generations - 1) if g < generations})
    ret, steps, x = playback(builder.build_env(cfg["env"]), loop.offspring_strategy.get_elite_model())
    print(f"# {label}: " + "; ".join(f"generation {g}: mean {means[g]:.2f} best {best[g]:.2f}" for g in at) +
          f"; max best {max(best):.2f}; final mean policy, one episode: return {ret:.2f}, {steps} steps, torso x {x:+.3f} m", flush=True)


def main():
    generations = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    os.chdir(tempfile.mkdtemp())                                        # the loop writes its metrics and checkpoints here
    for conf in sys.argv[3:] or ("hopper", "hopper_ars", "hopper_sep_cma"):
        run(conf, load(conf), generations, seed)


if __name__ == "__main__":
    main()
