"""The configs the env-table tests walk (test_env_table_host.py, test_gpu_env_table.py): every name of the registry with its
default team, simple_spread with three agents as well.  LunarLander comes under both heads through its two names."""
from ses.envs import REGISTRY

CASES = [(name, e.n_agents) for name, e in REGISTRY.items()] + [("simple_spread", 3)]
IDS = [f"{name}-{n}" for name, n in CASES]


def config(name, n_agents, **change):
    """the keyword arguments of _lib.env_info / the fields of SesConfig for this case, MLP policy, one episode"""
    e = REGISTRY[name]
    kw = dict(env_id=e.env_id, num_state=e.state_width(n_agents), num_action=e.num_action, discrete_action=int(e.discrete), gru=0,
              pomdp=0, eval_ep_num=1, n_agents=n_agents, physics64=0)
    kw.update(change)
    return kw
