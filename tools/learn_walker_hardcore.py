#!/usr/bin/env python3
"""Learning curves on BipedalWalkerHardcore-v3 (csrc/ses_walker_hardcore.hip): conf/bipedalwalker_hardcore.yaml, _sep_cma.yaml and
_pgpe.yaml, one seed each, 5 episodes per offspring, generation by generation (SES_BATCH_GENERATIONS=0, so that every generation's
fitness vector can be read).  Per run one summary line: the population mean and the best return at generations 0 / 50 / 150 / last,
and what the final mean policy (the strategy's elite model) does in one playback episode on the wrapper: its return, its length and
where its hull ends (the first float of the state blob is the hull's x; it starts at 4.67 m, the first obstacle at 9.33 m).
For scale: the first line of the output is the zero policy's return over the first-generation init rows of the seed.
usage: learn_walker_hardcore.py [generations] [seed] [config ...]
profiles/walker_hardcore_learning.txt is its output."""
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
    """one episode of the reference's test.py loop on the wrapper: (return, steps, hull x at the end)"""
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
          f"; max best {max(best):.2f}; final mean policy, one episode: return {ret:.2f}, {steps} steps, hull x {x:.2f} m", flush=True)


def zero_policy(seed):
    """the zero policy on 96 x 5 init rows of the env's stream: mean, minimum and maximum return and episode length"""
    from ses import HipES
    es = HipES("BipedalWalkerHardcore-v3", 24, 4, False, False, max_step=300, eval_ep_num=5)
    _, ret96, steps96 = es.rollout(es.zeros(96, es.P), es.init_states_uniform(seed, 0, 0, 96), want_episodes=True)
    print(f"# zero policy, 96 x 5 init rows of seed {seed}: return mean {float(ret96.mean()):.2f} min {float(ret96.min()):.2f} "
          f"max {float(ret96.max()):.2f}; steps mean {float(steps96.double().mean()):.1f} min {int(steps96.min())} max {int(steps96.max())}", flush=True)
    es.close()


def main():
    generations = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    os.chdir(tempfile.mkdtemp())                                        # the loop writes its metrics and checkpoints here
    zero_policy(seed)
    for conf in sys.argv[3:] or ("bipedalwalker_hardcore", "bipedalwalker_hardcore_sep_cma", "bipedalwalker_hardcore_pgpe"):
        run(conf, load(conf), generations, seed)


if __name__ == "__main__":
    main()
