"""Headless checkpoint playback: python test.py --cfg-path conf/cartpole.yaml --ckpt-path logs/.../ep_10.pt

Counterpart of the reference's test.py (test.py:20-68): loads a state_dict written by either code base, plays 100
episodes and prints `reward: ... ep_step: ...` per episode.  The 100 episodes are ONE launch of the fused rollout kernel
(a population of one offspring with eval_ep_num = 100).

With --save-gif the episodes are played step by step over the wrapper instead, as the reference plays them, and every episode
is written to test_gif/<run_num>/ep_<i>.gif (run_num = the third path component from the end of --ckpt-path, as in the
reference): the frames are drawn on the device, one render() call per episode (csrc/ses_render.hip, DESIGN.md section 19;
the scenes are this build's own depictions of CartPole, LunarLander, BipedalWalker and simple_spread -- other envs have none
and the flag is refused for them).  Writing the files needs PIL.
"""
import argparse
import os
from copy import deepcopy

import numpy as np
import torch
import yaml

import builder
from ses import HipES


def bind_obs_normalizer(dev, network):
    """Playback runs on what the policy was trained with: a network that carries the observation normaliser has its affine
    bound to the rollout handle, frozen (update off).  (The --save-gif branch plays over network.forward, which normalises
    itself.)"""
    if getattr(network, "obs_normalizer", False):
        dev.obs_norm_bind(torch.from_numpy(network.obs_norm_stats.numpy().copy()).to(dev.device),
                          torch.from_numpy(network.obs_norm_affine()).to(dev.device), update=False)


def play_and_save_gifs(args, env, network, seed):
    """The reference's playback loop (test.py:41-68) over the wrapper: a model copy per agent, env.step, the reward summed.  The
    state blob after every step is kept ON THE DEVICE; at the end of an episode all of its frames are drawn by one render() call
    (a scene launch and a raster launch for the whole episode) and written to test_gif/<run_num>/ep_<i>.gif."""
    from ses.render import write_gif
    run_num = args.ckpt_path.split("/")[-3]
    save_dir = f"test_gif/{run_num}/"
    os.makedirs(save_dir, exist_ok=True)
    agent_ids = env.get_agent_ids()
    env.seed_env = seed
    env._device().render_size()                            # an env without a scene stops here, before anything is played
    for i in range(args.episodes):
        models = {}
        for agent_id in agent_ids:
            models[agent_id] = deepcopy(network)
            models[agent_id].eval()
            models[agent_id].reset()
        obs = env.reset()
        done = False
        episode_reward = 0
        ep_step = 0
        blobs = []
        while not done:
            actions = {}
            for k, model in models.items():
                s = obs[k]["state"][np.newaxis, ...]
                actions[k] = model(s)
            obs, r, done, _ = env.step(actions)
            blobs.append(env.state_blob())
            episode_reward += r
            ep_step += 1
        print("reward: ", episode_reward, "ep_step: ", ep_step)
        frames = env._device().render(torch.cat(blobs))
        write_gif(save_dir + f"ep_{i}.gif", frames, fps=30)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--cfg-path", type=str, default="conf/cartpole.yaml")
    parser.add_argument("--ckpt-path", type=str, required=True)
    parser.add_argument("--episodes", type=int, default=100)
    parser.add_argument("--seed", type=int, default=None, help="env seed (default: env.seed of the config, else 0)")
    parser.add_argument("--save-gif", action="store_true")
    args = parser.parse_args()

    with open(args.cfg_path) as f:
        config = yaml.load(f, Loader=yaml.FullLoader)
    env = builder.build_env(config["env"])
    seed = args.seed if args.seed is not None else int(config["env"].get("seed", 0))
    network = builder.build_network(config["network"], config["env"]["name"])
    network.load_state_dict(torch.load(args.ckpt_path))
    if args.save_gif:
        return play_and_save_gifs(args, env, network, seed)

    dev = HipES(env.name, network.num_state, network.num_action, network.discrete_action, network.use_gru,
                pomdp=env.pomdp, max_step=env.horizon, eval_ep_num=args.episodes, n_agents=getattr(env, "n_agents", 1),
                physics64=getattr(env, "physics64", False))       # replay on the dynamics the policy was trained on
    theta = torch.from_numpy(network.flat()[None, :]).to(dev.device)
    bind_obs_normalizer(dev, network)
    init = dev.init_states_uniform(seed, 0, 0, 1)
    fit, ep_ret, ep_steps = dev.rollout(theta, init, want_episodes=True)
    rets = ep_ret[0].cpu().tolist()
    steps = ep_steps[0].cpu().tolist() if ep_steps is not None else [env.horizon] * args.episodes
    for r, s in zip(rets, steps):
        print("reward: ", r, "ep_step: ", s)
    print(f"mean reward over {args.episodes} episodes: {float(fit[0]):.3f}")


if __name__ == "__main__":
    main()
