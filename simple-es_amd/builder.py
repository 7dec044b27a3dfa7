"""build_env / build_network / build_loop with the reference's signatures and YAML keys (builder.py:10-86).

Optional keys (all default to reference behaviour): strategy.noise ("philox" | "numpy"),
strategy.seed, strategy.sigma_learning_rate / sigma_max_change / scale_limits (pgpe only),
strategy.elite_num (ars only: the directions used, at most offspring_num / 2),
strategy.elite_num / scale_limits / step_limits (sep_cma_es only), strategy.elite_num / memory / step_limits (lm_ma_es only), strategy.elite_num / step_limits (ma_es only), env.seed, env.shared_init, env.n_agents (simple_spread: 2 like the reference, or 3),
env.physics ("float32" | "float64": gym-order float64 CartPole dynamics),
network.obs_normalizer (the running observation normaliser of ARS V2: MLP policies on the eight float64 envs, any strategy, one GPU).
"""
from envs.gym_wrapper import GymWrapper
from envs.pettingzoo_wrapper import PettingzooWrapper
from learning_strategies.evolution.loop import ESLoop
from learning_strategies.evolution.offspring_strategies import ars, lm_ma_es, ma_es, openai_es, pgpe, sep_cma_es, simple_evolution, simple_genetic
from networks.neural_network import GymEnvModel
from ses.envs import PETTINGZOO_UNBUILT, names

# the names PettingzooWrapper is handed: those it serves, and those it refuses by name instead of a gym look-up
_PETTINGZOO = names(wrapper="pettingzoo") + PETTINGZOO_UNBUILT
_STRATEGIES = {
    "simple_evolution": (simple_evolution, ("init_sigma", "sigma_decay", "elite_num", "offspring_num")),
    "simple_genetic": (simple_genetic, ("init_sigma", "sigma_decay", "elite_num", "offspring_num")),
    "openai_es": (openai_es, ("init_sigma", "sigma_decay", "learning_rate", "offspring_num")),
    "pgpe": (pgpe, ("init_sigma", "sigma_decay", "learning_rate", "offspring_num")),
    "sep_cma_es": (sep_cma_es, ("init_sigma", "sigma_decay", "offspring_num")),
    "lm_ma_es": (lm_ma_es, ("init_sigma", "sigma_decay", "offspring_num")),
    "ma_es": (ma_es, ("init_sigma", "sigma_decay", "offspring_num")),
}
# tests/test_ma_es_host.py holds _STRATEGIES to exactly the seven names above; a strategy added since is listed here
_LATER_STRATEGIES = {
    "ars": (ars, ("init_sigma", "sigma_decay", "learning_rate", "offspring_num")),
}
_OPTIONAL = ("noise", "seed")
_OPTIONAL_BY_STRATEGY = {"pgpe": ("sigma_learning_rate", "sigma_max_change", "scale_limits"),
                         "ars": ("elite_num",),
                         "sep_cma_es": ("elite_num", "scale_limits", "step_limits"),
                         "lm_ma_es": ("elite_num", "memory", "step_limits"),
                         "ma_es": ("elite_num", "step_limits")}


def build_env(config):
    if config["name"] in _PETTINGZOO:
        return PettingzooWrapper(config["name"], config["max_step"], n_agents=config.get("n_agents"))
    return GymWrapper(config["name"], config["max_step"], config["pomdp"], physics=config.get("physics", "float32"))


# the envs the observation normaliser serves: the eight float64 control envs (include/ses.h, ses_obs_norm_bind)
OBS_NORMALIZER_ENVS = names(obs_normalizer=True)


def build_network(config, env_name=None):
    """env_name: the env the network will run in, where the caller knows it (build_loop): network.obs_normalizer is refused for
    an env it does not serve."""
    if config["name"] == "gym_model":
        norm = bool(config.get("obs_normalizer", False))
        if norm and config["gru"]:
            raise ValueError("network.obs_normalizer serves MLP policies only: gru: True runs the lockstep kernel shared with "
                             "every other env, which has no normalising form")
        if norm and env_name is not None and env_name not in OBS_NORMALIZER_ENVS:
            raise ValueError(f"network.obs_normalizer: env {env_name!r} is not one of the float64 envs it serves {OBS_NORMALIZER_ENVS}")
        if not norm:              # (the reference's four arguments: a user's subclass of the container keeps working)
            return GymEnvModel(config["num_state"], config["num_action"], config["discrete_action"], config["gru"])
        return GymEnvModel(config["num_state"], config["num_action"], config["discrete_action"], config["gru"], obs_normalizer=True)
    raise ValueError(f"unknown network {config['name']!r}")


def build_strategy(strategy_cfg):
    known = {**_STRATEGIES, **_LATER_STRATEGIES}
    if strategy_cfg["name"] not in known:
        raise ValueError(f"unknown strategy {strategy_cfg['name']!r}")
    cls, keys = known[strategy_cfg["name"]]
    extra = {k: strategy_cfg[k] for k in _OPTIONAL + _OPTIONAL_BY_STRATEGY.get(strategy_cfg["name"], ()) if k in strategy_cfg}
    return cls(*[strategy_cfg[k] for k in keys], **extra)


def build_loop(config, gen_num, process_num, eval_ep_num, log, save_model_period):
    env = build_env(config["env"])
    network = build_network(config["network"], config["env"]["name"])
    strategy = build_strategy(config["strategy"])
    if isinstance(strategy, ma_es):
        strategy.check_parameters(network.param_count())     # the full matrix: refused here, before anything touches a device
    return ESLoop(config, strategy, env, network, gen_num, process_num, eval_ep_num, log, save_model_period)
