"""Each row of the library's env table reaches its own unit: for every case of env_table_cases.CASES a handle's state bytes and
observation width are ses_env_info's, a reset of two envs, one step with a zero action of the layout ses_env_info names and a
rollout of two rows run and return finite tensors of the shapes it says.  Nothing about values: the per-env parity suites hold those."""
import pytest
import torch

from env_table_cases import CASES, IDS, config

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,n_agents", CASES, ids=IDS)
def test_the_rows_pointers_reach_the_envs_unit(name, n_agents):
    from ses import HipES, _lib
    kw = config(name, n_agents)
    want = _lib.env_info(**kw)
    es = HipES(name, kw["num_state"], kw["num_action"], bool(kw["discrete_action"]), False, max_step=4, eval_ep_num=1, n_agents=n_agents)
    assert es.env_state_bytes() == want.state_bytes and es.env_obs_width() == want.obs_width
    assert (es.init_dim, es.init_range) == (want.init_width, (want.init_lo, want.init_hi))
    init = es.init_states_uniform(3, 0, 0, 2)                                      # [2, 1, init width]
    state, obs = es.env_reset(init[:, 0].contiguous())
    assert tuple(state.shape) == (2, want.state_bytes) and tuple(obs.shape) == (2, want.obs_width) and torch.isfinite(obs).all()
    shape = {_lib.ACTION_I32_N: (2,), _lib.ACTION_I32_N_AGENTS: (2, want.agents), _lib.ACTION_F32_N_A: (2, want.num_action),
             _lib.ACTION_F32_N_AGENTS_A: (2, want.agents, want.num_action)}[want.action_layout]
    integer = want.action_layout in (_lib.ACTION_I32_N, _lib.ACTION_I32_N_AGENTS)
    action = torch.zeros(shape, dtype=torch.int32 if integer else torch.float32, device=es.device)
    obs, reward, done = es.env_step_generic(state, action)
    assert tuple(obs.shape) == (2, want.obs_width) and tuple(reward.shape) == (2,) and tuple(done.shape) == (2,)
    assert torch.isfinite(obs).all() and torch.isfinite(reward).all()
    theta = torch.zeros(2, es.P, device=es.device)
    fitness, ep_return, ep_steps = es.rollout(theta, init, want_episodes=True)
    assert tuple(fitness.shape) == (2,) and torch.isfinite(fitness).all() and torch.isfinite(ep_return).all()
    assert (ep_steps is not None) == bool(want.has_ep_steps)
    es.close()
