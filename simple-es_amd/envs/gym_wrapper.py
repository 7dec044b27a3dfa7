"""GymWrapper -- the reference's env adapter (envs/gym_wrapper.py:7-54) backed by the device env kernels.

The reference wraps a gym env object; gym's physics is third-party Python.  Here the env IS a gfx950
kernel: the population rollout never calls this object step by step (ESLoop hands the whole shard to the
fused rollout kernel), it only reads `name / max_step / pomdp`.  `reset()` / `step()` keep the reference's
dict protocol for single-env use (checkpoint playback, the reference's test.py loop) for EVERY supported env:
one-lane launches of ses_env_reset / ses_env_step_generic, i.e. the same device functions the fused rollouts call.
"""
import numpy as np
import torch

from ses.envs import REGISTRY, names

# views of the registry (ses/envs.py) for the names this wrapper serves
SUPPORTED = {name: dict(num_state=e.num_state, num_action=e.num_action, discrete=e.discrete, time_limit=e.time_limit)
             for name, e in REGISTRY.items() if e.wrapper == "gym"}
CLASSIC_CONTROL = names(family="classic-control")
PYBULLET_PENDULA = names(family="pybullet-pendula")
PYBULLET_RESTATED = names(variant="pybullet-restated")


class GymWrapper:
    def __init__(self, name, max_step=None, pomdp=False, physics="float32"):
        if name not in SUPPORTED:
            raise NotImplementedError(
                f"env {name!r} has no gfx950 kernel in this build (available: {sorted(SUPPORTED)}); "
                "there is no CPU/gym fallback")
        if pomdp and not REGISTRY[name].pomdp:
            raise AssertionError(f"{name} doesn't support POMDP.")
        self.name = name
        self.pomdp = bool(pomdp)
        if physics not in ("float32", "float64"):
            raise ValueError("env.physics must be 'float32' (default) or 'float64' (gym-order CartPole dynamics)")
        self.physics64 = physics == "float64"
        self.spec = SUPPORTED[name]
        self.variant = REGISTRY[name].variant
        # YAML `max_step: None` is the STRING "None" in the reference (gym_wrapper.py:37); accept both.
        limit = self.spec["time_limit"]
        self.max_step = max_step
        self.horizon = limit if max_step in (None, "None") else min(int(max_step), limit)
        self.curr_step = 0
        self.seed_env = 0
        self._episode = 0
        self._dev = None
        self._state = None

    def get_agent_ids(self):
        return ["0"]

    # ---- single-env protocol (playback) ---------------------------------------------------------
    def _device(self):
        if self._dev is None:
            from ses import HipES
            sp = self.spec
            # (env.physics: float64 exists in the fused rollouts only: the library refuses a step-wise reset of such a handle)
            self._dev = HipES(self.name, sp["num_state"], sp["num_action"], sp["discrete"], False, pomdp=self.pomdp,
                              max_step=self.horizon, eval_ep_num=1, physics64=self.physics64)
        return self._dev

    def reset(self):
        """gym_wrapper.py:23-30: {"0": {"state": obs}}; the reset distribution is this library's (the reference never seeds
        its env): episode k of this object draws row (seed_env, k) of the ENV_INIT Philox stream."""
        dev = self._device()
        self.curr_step = 0
        init = dev.init_states_uniform(self.seed_env, self._episode, 0, 1)[:, 0].contiguous()     # [1, init_dim]
        self._episode += 1
        self._state, obs = dev.env_reset(init)
        return {"0": {"state": obs[0].cpu().numpy()}}

    def step(self, action):
        """gym_wrapper.py:32-45: ({"0": transition}, r, done, info); done = env done or curr_step >= max_step."""
        dev = self._device()
        self.curr_step += 1
        a = np.asarray(action["0"])
        if self.spec["discrete"]:
            act = torch.tensor([int(a)], dtype=torch.int32, device=dev.device)
        else:
            act = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(1, -1)).to(dev.device)
        obs, reward, done = dev.env_step_generic(self._state, act)
        s, r, d = obs[0].cpu().numpy(), float(reward[0].item()), bool(int(done[0].item()))
        if self.max_step != "None" and self.max_step is not None:
            if self.curr_step >= int(self.max_step) or d:
                d = True
        if self.curr_step >= self.spec["time_limit"]:          # gym's own TimeLimit wrapper around the registered env
            d = True
        tr = {"state": s, "reward": r, "done": d, "info": {}}
        return {"0": tr}, r, d, {}

    def state_blob(self):
        """A clone of the current device state (uint8[1, state_bytes]): what HipES.render draws, many at a time."""
        if self._state is None:
            raise RuntimeError("state_blob() before the first reset()")
        return self._state.clone()

    def render(self):
        """gym_wrapper.py:50-51: the rgb_array of the current state, uint8[H, W, 3] -- the device scene of this env rasterised
        (csrc/ses_render.hip).  An env without a scene raises NotImplementedError naming the ones that have one."""
        from ses.render import to_rgb
        dev = self._device()
        dev.render_size()
        if self._state is None:
            raise RuntimeError("render() before the first reset()")
        return to_rgb(dev.render(self._state)[0])

    def close(self):
        if self._dev is not None:
            self._dev.close()
            self._dev = None
