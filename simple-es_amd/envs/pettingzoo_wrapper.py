"""PettingzooWrapper -- the reference's multi-agent env adapter (envs/pettingzoo_wrapper.py:6-64) backed by
the device simple_spread, waterworld and pursuit kernels.

The reference hard-codes `simple_spread_v2.env(N=2)` (pettingzoo_wrapper.py:9); `n_agents` keeps that
default and also allows 3 (BASELINE.json configs[4]).  waterworld is the build's own float64 definition modelled on
`waterworld_v3.env()` with its defaults (csrc/ses_waterworld.h; parity with pettingzoo unpinned): five
pursuers `pursuer_0..4`, 242 observations and two continuous actions each, 500 cycles.  pursuit is likewise the build's own
definition modelled on `pursuit_v3.env()` with its defaults (csrc/ses_pursuit.h; parity unpinned): eight
pursuers `pursuer_0..7`, a 7 x 7 x 3 window (147 observations) and one of five moves each, 500 cycles, done when the last of the 30
evaders is caught.  multiwalker needs polygon-polygon contacts and is not built: it raises instead of falling back to a CPU env.

As with GymWrapper, the population rollout never steps this object: ESLoop hands the whole shard to the
fused kernel.  reset() / step() keep the reference's dict protocol for single-team use (the reference's test.py
loop): one-lane launches of ses_env_reset / ses_env_step_generic, the same device functions the fused rollouts call.
"""
import numpy as np
import torch

from ses.envs import REGISTRY, names

NAMES = names(wrapper="pettingzoo")
# views of the registry (ses/envs.py)
MAX_CYCLES = REGISTRY["simple_spread"].time_limit             # pettingzoo mpe default max_cycles: every agent is done after 25 cycles
WATERWORLD_CYCLES = REGISTRY["waterworld"].time_limit         # waterworld_v3's default max_cycles
WATERWORLD_OBS, WATERWORLD_PURSUERS = REGISTRY["waterworld"].num_state, REGISTRY["waterworld"].n_agents
PURSUIT_CYCLES = REGISTRY["pursuit"].time_limit               # pursuit_v3's default max_cycles
PURSUIT_OBS, PURSUIT_PURSUERS = REGISTRY["pursuit"].num_state, REGISTRY["pursuit"].n_agents


class PettingzooWrapper:
    def __init__(self, name, max_step=None, n_agents=None):
        if name not in NAMES:
            raise NotImplementedError(f"env {name!r} has no gfx950 kernel in this build (available: {', '.join(NAMES)}); "
                                      "there is no CPU/pettingzoo fallback")
        self.spec = spec = REGISTRY[name]
        if n_agents is None:
            n_agents = spec.n_agents
        if n_agents not in spec.n_agents_allowed:
            raise NotImplementedError(spec.n_agents_error)
        self.name = name
        self.max_step = max_step
        self.n_agents = n_agents
        self.pomdp = False
        self.variant = spec.variant
        cycles = spec.time_limit
        self.horizon = cycles if max_step in (None, "None") else min(int(max_step), cycles)
        self.agents = [f"{spec.agent_prefix}_{i}" for i in range(n_agents)]
        self.curr_step = 0
        self.seed_env = 0
        self._episode = 0
        self._dev = None
        self._state = None

    def get_agent_ids(self):
        return list(self.agents)

    def _device(self):
        if self._dev is None:
            from ses import HipES
            sp = self.spec
            self._dev = HipES(self.name, sp.state_width(self.n_agents), sp.num_action, sp.discrete, False, max_step=self.horizon,
                              eval_ep_num=1, n_agents=self.n_agents)
        return self._dev

    def _transitions(self, obs):
        per = obs.view(self.n_agents, -1).cpu().numpy()
        return {agent: {"state": per[i].copy()} for i, agent in enumerate(self.agents)}

    def reset(self):
        """pettingzoo_wrapper.py:22-31: {agent: {"state": obs}}; positions from row (seed_env, episode) of the ENV_INIT stream."""
        dev = self._device()
        self.curr_step = 0
        init = dev.init_states_uniform(self.seed_env, self._episode, 0, 1)[:, 0].contiguous()
        self._episode += 1
        self._state, obs = dev.env_reset(init)
        return self._transitions(obs[0])

    def step(self, action):
        """pettingzoo_wrapper.py:33-58: every agent's action is set, the world advances one cycle; per-agent transitions,
        the TEAM reward (sum over the agents) and done = all agents done or curr_step >= max_step."""
        dev = self._device()
        self.curr_step += 1
        if self.spec.action_scale is not None:
            for a in self.agents:
                act = action[a]
                act *= np.float32(self.spec.action_scale)   # pettingzoo_wrapper.py:37-38: in place, on the caller's float32 array
        # one team's actions in the env's action layout (ses_env_info): float32[1, agents, A] or int32[1, agents]
        shape = dev.action_shape(1)
        if len(shape) == 3:
            acts = torch.from_numpy(np.stack([np.asarray(action[a], np.float32).reshape(shape[2]) for a in self.agents])[None]).to(dev.device)
        else:
            acts = torch.tensor([[int(np.asarray(action[a])) for a in self.agents]], dtype=torch.int32, device=dev.device)
        obs, reward, done = dev.env_step_generic(self._state, acts)
        total_r, d = float(reward[0].item()), bool(int(done[0].item()))
        out = self._transitions(obs[0])
        for tr in out.values():
            # per-agent rewards of a cycle are equal shares of local + global terms in the fused kernel's accounting; the
            # protocol's consumers (loop.py:123, test.py:61) use the team total returned below
            tr.update(reward=total_r / self.n_agents, done=d, info={})
        if self.max_step != "None" and self.max_step is not None:
            if self.curr_step >= int(self.max_step) or d:
                d = True
        return out, total_r, d, {}

    def state_blob(self):
        """A clone of the current device state (uint8[1, state_bytes]): what HipES.render draws, many at a time."""
        if self._state is None:
            raise RuntimeError("state_blob() before the first reset()")
        return self._state.clone()

    def render(self):
        """pettingzoo_wrapper.py:63-64: the rgb_array of the current state, uint8[H, W, 3] -- the device scene of this env
        rasterised (csrc/ses_render.hip).  An env without a scene (waterworld, pursuit) raises NotImplementedError naming the
        ones that have one."""
        from ses.render import to_rgb
        dev = self._device()
        dev.render_size()
        if self._state is None:
            raise RuntimeError("render() before the first reset()")
        return to_rgb(dev.render(self._state)[0])
