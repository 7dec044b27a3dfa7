"""ses.envs -- one record per env NAME with what only the Python side knows.  Pure data: no torch, no library.

What the library knows about an env -- init rows, observation width, state bytes, the action layout -- is in its env table
(csrc/ses_env_table.h) and is read with ses_env_info (_lib.env_info), never restated here.  ses.device, both wrappers and builder.py
derive their module-level tables from REGISTRY.  A new env is its own unit in csrc/, one table row there and one record here.
"""
from typing import NamedTuple, Optional, Tuple

from ._lib import (ENV_ACROBOT, ENV_BIPEDALWALKER, ENV_BIPEDALWALKER_HARDCORE, ENV_CARTPOLE, ENV_DOUBLE_PENDULUM, ENV_HOPPER, ENV_INVERTED_PENDULUM, ENV_LUNARLANDER,
                   ENV_MOUNTAINCAR, ENV_MOUNTAINCAR_CONT, ENV_NONE, ENV_PENDULUM, ENV_PENDULUM_SWINGUP, ENV_PURSUIT, ENV_REACHER,
                   ENV_SIMPLE_SPREAD, ENV_WALKER2D, ENV_WATERWORLD)


class Env(NamedTuple):
    env_id: int
    num_state: int                    # per agent; times n_agents where state_per_agent
    num_action: int
    discrete: bool
    time_limit: int                   # gym's TimeLimit / pettingzoo's max_cycles
    wrapper: str = "gym"              # "gym" (envs/gym_wrapper.py) | "pettingzoo" (envs/pettingzoo_wrapper.py)
    # a name whose third-party physics is restated here without a pin says so at run time (ESLoop prints it, metrics.jsonl records
    # it): returns are the build's own, not the original's bit for bit
    variant: Optional[str] = None
    family: Optional[str] = None      # the name lists the wrappers export
    pomdp: bool = False               # env.pomdp exists
    obs_normalizer: bool = False      # network.obs_normalizer serves it: the float64 control envs (include/ses.h, ses_obs_norm_bind)
    state_per_agent: bool = False
    n_agents: int = 1                 # default ...
    n_agents_allowed: Tuple[int, ...] = (1,)     # ... and what env.n_agents may say
    n_agents_error: str = ""
    agent_prefix: str = ""
    action_scale: Optional[float] = None         # the wrapper multiplies every agent's action by it, in place (the reference does)

    def state_width(self, n_agents):
        return self.num_state * n_agents if self.state_per_agent else self.num_state


def _classic(env_id, S, A, discrete, limit):
    return Env(env_id, S, A, discrete, limit, variant="classic-control-restated", family="classic-control", obs_normalizer=True)


def _pybullet(env_id, S, A, limit, family):
    return Env(env_id, S, A, False, limit, variant="pybullet-restated", family=family, obs_normalizer=True)


REGISTRY = {
    "CartPole-v1": Env(ENV_CARTPOLE, 4, 2, True, 500, pomdp=True),
    "CartPole-v0": Env(ENV_CARTPOLE, 4, 2, True, 200, pomdp=True),
    # pettingzoo MPE simple_spread: the reference hard-codes N=2; 3 is served as well
    "simple_spread": Env(ENV_SIMPLE_SPREAD, 6, 5, True, 25, wrapper="pettingzoo", state_per_agent=True, n_agents=2,
                         n_agents_allowed=(2, 3), n_agents_error="simple_spread kernels are instantiated for 2 or 3 agents",
                         agent_prefix="agent"),
    # gym's two landers restated on a Box2D-style world (csrc/ses_lander.h, ses_b2.h): one world step and one env id, two action
    # spaces -- SesConfig.discrete_action tells them apart (csrc/ses_lander_discrete.hip: the argmax head)
    "LunarLanderContinuous-v2": Env(ENV_LUNARLANDER, 8, 4, False, 1000, variant="box2d-restated", pomdp=True),
    "LunarLander-v2": Env(ENV_LUNARLANDER, 8, 4, True, 1000, variant="box2d-restated", pomdp=True),
    # gym's env restated on the same world (csrc/ses_walker.h)
    "BipedalWalker-v3": Env(ENV_BIPEDALWALKER, 24, 4, False, 1600, variant="box2d-restated"),
    # gym 0.21's classic-control envs restated in float64 in gym's order of operations (csrc/ses_classic.h); the two continuous
    # members: one tanh output, clipped by the env
    "Acrobot-v1": _classic(ENV_ACROBOT, 6, 3, True, 500),
    "MountainCar-v0": _classic(ENV_MOUNTAINCAR, 2, 3, True, 200),
    "Pendulum-v1": _classic(ENV_PENDULUM, 3, 1, False, 200),
    "MountainCarContinuous-v0": _classic(ENV_MOUNTAINCAR_CONT, 2, 1, False, 999),
    # the build's own float64 definition modelled on waterworld_v3.env() with its defaults (csrc/ses_waterworld.h)
    "waterworld": Env(ENV_WATERWORLD, 242, 2, False, 500, wrapper="pettingzoo", variant="waterworld-restated", n_agents=5,
                      n_agents_allowed=(5,), n_agents_error="waterworld has five pursuers", agent_prefix="pursuer",
                      action_scale=0.001),
    # the inverted-pendulum family modelled on pybullet_envs: the build's own float64 definitions (csrc/ses_pendula.h, DESIGN.md
    # 7) -- one tanh output, clipped by the env
    "InvertedPendulumBulletEnv-v0": _pybullet(ENV_INVERTED_PENDULUM, 5, 1, 1000, "pybullet-pendula"),
    "InvertedPendulumSwingupBulletEnv-v0": _pybullet(ENV_PENDULUM_SWINGUP, 5, 1, 1000, "pybullet-pendula"),
    "InvertedDoublePendulumBulletEnv-v0": _pybullet(ENV_DOUBLE_PENDULUM, 9, 1, 1000, "pybullet-pendula"),
    # the build's own integer definition modelled on pursuit_v3.env() with its defaults (csrc/ses_pursuit.h)
    "pursuit": Env(ENV_PURSUIT, 147, 5, True, 500, wrapper="pettingzoo", variant="pettingzoo-restated", n_agents=8,
                   n_agents_allowed=(8,), n_agents_error="pursuit has eight pursuers", agent_prefix="pursuer"),
    # pybullet's Reacher restated the same way (csrc/ses_reacher.h): two tanh outputs, a target drawn per episode;
    # never terminates, the registered TimeLimit is 150 steps
    "ReacherBulletEnv-v0": _pybullet(ENV_REACHER, 9, 2, 150, "pybullet-reacher"),
    # pybullet's planar hopper as the build's own float32 definition on the Box2D-style world (csrc/ses_hopper_env.h):
    # three tanh outputs; the observation normaliser serves the float64 envs only
    "HopperBulletEnv-v0": Env(ENV_HOPPER, 15, 3, False, 1000, variant="pybullet-restated", family="pybullet-hopper"),
    # pybullet's Walker2D the same way (csrc/ses_walker2d_env.h): the hopper's leg twice on one torso, six tanh outputs
    "Walker2DBulletEnv-v0": Env(ENV_WALKER2D, 22, 6, False, 1000, variant="pybullet-restated", family="pybullet-walker2d"),
    # gym's hardcore walker as the build's own definition (csrc/ses_walker_hardcore_env.h): BipedalWalker-v3's body on
    # stumps, pits and stairs; gym registers it with 2000 steps
    "BipedalWalkerHardcore-v3": Env(ENV_BIPEDALWALKER_HARDCORE, 24, 4, False, 2000, variant="box2d-restated"),
}
# pettingzoo names that have no kernel: builder.py still routes them to the pettingzoo wrapper, which refuses them (multiwalker needs
# polygon-polygon contacts)
PETTINGZOO_UNBUILT = ("multiwalker",)
# name -> env id; None: a handle without an env (it serves the strategies and ses_policy_forward)
ENV_IDS = {**{name: e.env_id for name, e in REGISTRY.items()}, None: ENV_NONE}


def names(**where):
    """the registry's names, in its order, whose record has every given field value: names(wrapper="gym")"""
    return tuple(n for n, e in REGISTRY.items() if all(getattr(e, k) == v for k, v in where.items()))
