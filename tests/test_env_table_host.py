"""The library's env table (csrc/ses_env_table.h, ses_env_info) against the Python registry (ses/envs.py) and the numpy
restatements, on the host: no device, no kernel.  For every case of env_table_cases.CASES the table's row and the registry's record
must describe one env, ses_create must take the registry's config and refuse every single wrong field by name."""
import ctypes

import pytest

import classic_control_cont_np
import classic_control_np
import pendula_np
import pursuit_np
import reacher_np
import waterworld_np
from env_table_cases import CASES, IDS, config
from ses import _lib
from ses.envs import REGISTRY

INVALID, NO_DEVICE = -1, -4
# what the rows refuse, said here independently of both tables
GRU_REFUSED = {"BipedalWalker-v3", "waterworld", "pursuit"}
PHYSICS64_ACCEPTED = {"CartPole-v1", "CartPole-v0"}
EPISODE_CAP = {"waterworld": 16, "pursuit": 16}
EITHER_HEAD = {"LunarLander-v2", "LunarLanderContinuous-v2"}
# name -> (init width, init range or None where the restatement states the width only)
INIT_ROWS = {name: (e["init_dim"], e["init_range"])
             for envs in (classic_control_np.ENVS, classic_control_cont_np.ENVS, pendula_np.ENVS) for name, e in envs.items()}
INIT_ROWS["ReacherBulletEnv-v0"] = (reacher_np.INIT_DIM, reacher_np.INIT_RANGE)
INIT_ROWS["waterworld"] = (waterworld_np.INIT_W, None)
INIT_ROWS["pursuit"] = (pursuit_np.INIT_W, None)


def _cfg(kw):
    return _lib.SesConfig(kw["env_id"], kw["num_state"], kw["num_action"], kw["discrete_action"], kw["gru"], kw["pomdp"], 4,
                          kw["eval_ep_num"], 0, 0, kw["n_agents"], kw["physics64"])


def info(kw):
    """(rc, message, SesEnvInfo) of ses_env_info on the raw config"""
    lib, cfg, out = _lib.load(), _cfg(kw), _lib.SesEnvInfo()
    rc = lib.ses_env_info(ctypes.byref(cfg), ctypes.byref(out))
    return rc, (lib.ses_last_error().decode() if rc != _lib.SES_OK else ""), out


def create(kw):
    """(rc, message) of ses_create on the raw config"""
    lib, cfg, h = _lib.load(), _cfg(kw), ctypes.c_void_p()
    rc = lib.ses_create(ctypes.byref(cfg), None, ctypes.byref(h))
    msg = lib.ses_last_error().decode() if rc != _lib.SES_OK else ""
    if rc == _lib.SES_OK:
        lib.ses_destroy(h)
    return rc, msg


@pytest.mark.parametrize("name,n_agents", CASES, ids=IDS)
def test_the_row_describes_the_registrys_env(name, n_agents):
    e, kw = REGISTRY[name], config(name, n_agents)
    rc, msg, got = info(kw)
    assert rc == _lib.SES_OK, msg
    if name in INIT_ROWS:
        width, rng = INIT_ROWS[name]
        assert got.init_width == width
        assert rng is None or (got.init_lo, got.init_hi) == rng
    assert got.init_width >= 1 and got.init_lo < got.init_hi
    assert got.obs_width == e.state_width(n_agents) * n_agents and got.agents == n_agents and got.num_action == e.num_action
    assert got.state_bytes > 0
    team = e.wrapper == "pettingzoo"
    assert got.action_layout == {(True, False): _lib.ACTION_I32_N, (True, True): _lib.ACTION_I32_N_AGENTS,
                                 (False, False): _lib.ACTION_F32_N_A, (False, True): _lib.ACTION_F32_N_AGENTS_A}[(e.discrete, team)]
    assert bool(got.has_ep_steps) == (name != "simple_spread") and bool(got.is_f64) == e.obs_normalizer
    assert create(kw)[0] in (_lib.SES_OK, NO_DEVICE)


@pytest.mark.parametrize("name,n_agents", CASES, ids=IDS)
def test_ses_create_refuses_each_single_wrong_field_by_name(name, n_agents):
    e, ok = REGISTRY[name], config(name, n_agents)
    wrong = [("num_state", ok["num_state"] + 1), ("num_state", ok["num_state"] - 1), ("num_action", ok["num_action"] + 1)]
    right = []
    (right if name in EITHER_HEAD else wrong).append(("discrete_action", 1 - ok["discrete_action"]))
    (wrong if name in GRU_REFUSED else right).append(("gru", 1))
    wrong.append(("gru", 2))
    (right if e.pomdp else wrong).append(("pomdp", 1))
    (right if name in PHYSICS64_ACCEPTED else wrong).append(("physics64", 1))
    if e.wrapper == "pettingzoo":
        wrong += [("n_agents", max(e.n_agents_allowed) + 1), ("n_agents", min(e.n_agents_allowed) - 1)]
    if name in EPISODE_CAP:
        right.append(("eval_ep_num", EPISODE_CAP[name]))
        wrong.append(("eval_ep_num", EPISODE_CAP[name] + 1))
    for field, value in right:
        assert create(dict(ok, **{field: value}))[0] in (_lib.SES_OK, NO_DEVICE), (field, value)
    for field, value in wrong:
        for rc, msg in (create(dict(ok, **{field: value})), info(dict(ok, **{field: value}))[:2]):
            assert rc == INVALID and field in msg, (field, value, rc, msg)
    if name in EPISODE_CAP:
        assert f"1 .. {EPISODE_CAP[name]}" in create(dict(ok, eval_ep_num=EPISODE_CAP[name] + 1))[1]


def test_an_id_outside_the_table_is_refused():
    ok = config("CartPole-v1", 1)
    for env_id in (len(set(e.env_id for e in REGISTRY.values())), 99, -2):
        for rc, msg in (create(dict(ok, env_id=env_id)), info(dict(ok, env_id=env_id))[:2]):
            assert rc == INVALID and "env_id" in msg, (env_id, rc, msg)
    assert info(dict(ok, env_id=_lib.ENV_NONE))[0] == INVALID                # no env: nothing to describe ...
    assert create(dict(ok, env_id=_lib.ENV_NONE))[0] in (_lib.SES_OK, NO_DEVICE)     # ... but a handle for the strategies


def test_records_and_rows_name_the_same_ids():
    ok = config("CartPole-v1", 1)
    rows = {env_id for env_id in range(-8, 64) if env_id != _lib.ENV_NONE and "unknown env_id" not in info(dict(ok, env_id=env_id))[1]}
    assert rows == {e.env_id for e in REGISTRY.values()}
    named = {getattr(_lib, k) for k in dir(_lib) if k.startswith("ENV_")} - {_lib.ENV_NONE}
    assert rows == named
