"""numpy restatement of the running observation normaliser (include/ses.h: ses_obs_norm_bind / ses_obs_norm_merge).
Imports no product code: the envs are the host restatements the rollout tests already use, the policy is the C oracle's forward.

Normalised rollout.  The host loops of classic_control_np, classic_control_cont_np, pendula_np and reacher_np, entered through
their `policy` argument: the policy wrapper sees the RAW observation of every env whose step is about to be taken, records it,
and hands fl(fl(obs - shift) * scale) (numpy float32: one rounding per operation) to the oracle's forward.  The loops are run
with one episode per row (row = env, its index carried in an extra column of theta that the wrapper strips), so the wrapper
knows which env an observation belongs to; envs are independent, so the returns are those of the [N, E] population.

Accumulation per env, in step order, float64:  s1[k] += obs[k];  s2[k] += obs[k] * obs[k] (exact: 24-bit factors);  steps += 1.
partials = float64[2 S + 1, n_env]: row 0 the step counts, rows 1 .. S s1, rows S + 1 .. 2 S s2.

Reduction over envs (reduce_envs): lane l of 256 adds x[l], x[l + 256], ... ascending to +0.0; then x[l] = x[l] + x[l + s] for
s = 128, 64, ..., 1.  A function of n_env alone.

Merge (merge_component), numpy float64 scalars, one rounding per operation, in the order of the contract:
    n_b == 0: unchanged.  mb = S1 / n_b;  M2b = max(S2 - S1 * mb, 0);  N = n + n_b;  f = n_b / N;  d = mb - mean;
    mean' = mean + d * f;  M2' = (M2 + M2b) + (d * d) * (n * f);  std = sqrt(M2' / (N - 1)) if N >= 2 else 1;
    shift = float32(mean');  scale = 0 if std < 1e-7 else float32(1 / std).
"""
import numpy as np

import classic_control_cont_np as ccc
import classic_control_np as cc
import pendula_np as pn
import reacher_np as rn
from oracle import c_oracle as co

LANES = 256
STD_FLOOR = np.float64(1e-7)

# name -> (S, A, discrete action)
SHAPES = {
    "Acrobot-v1": (6, 3, True), "MountainCar-v0": (2, 3, True), "Pendulum-v1": (3, 1, False),
    "MountainCarContinuous-v0": (2, 1, False), "InvertedPendulumBulletEnv-v0": (5, 1, False),
    "InvertedPendulumSwingupBulletEnv-v0": (5, 1, False), "InvertedDoublePendulumBulletEnv-v0": (9, 1, False),
    "ReacherBulletEnv-v0": (9, 2, False),
}


def fresh(S):
    """(stats float64[S, 3], affine float32[2, S]) of a new run"""
    affine = np.zeros((2, S), np.float32)
    affine[1] = 1.0
    return np.zeros((S, 3), np.float64), affine


def normalise(obs, affine):
    obs = np.asarray(obs, np.float32)
    d = obs - affine[0].astype(np.float32)                              # float32 arrays: each operation rounds once
    return d * affine[1].astype(np.float32)


def _host_rollout(name, theta, init, max_step, policy):
    if name in cc.ENVS:
        return cc.rollout(name, theta, init, 1, max_step, policy)
    if name in ccc.ENVS:
        return ccc.rollout(name, theta, init, 1, max_step, policy)
    if name in pn.ENVS:
        return pn.rollout(name, theta, init, 1, max_step, policy)
    assert name == "ReacherBulletEnv-v0", name
    return rn.rollout(theta, init, 1, max_step, policy)


def rollout(name, theta, init, E, max_step, affine, record_seen=False):
    """theta float32[N, P], init float32[N or 1, E, W], affine float32[2, S] (frozen for the rollout).
    Returns (fitness float32[N], ep_return float64[N, E], ep_steps int32[N, E], partials float64[2 S + 1, N E]).
    record_seen: accumulate what the policy SEES instead of the raw observation -- what the device must NOT do (the tests
    show that the two differ on their data)."""
    S, A, discrete = SHAPES[name]
    theta = np.asarray(theta, np.float32)
    N, P = theta.shape
    n_env = N * E
    assert n_env < 2 ** 24                                              # the env index rides in a float32 column
    init = np.broadcast_to(init, (N, E, init.shape[-1])).reshape(n_env, 1, -1)
    aug = np.concatenate([np.repeat(theta, E, axis=0), np.arange(n_env, dtype=np.float32)[:, None]], axis=1)
    s1 = np.zeros((S, n_env), np.float64)
    s2 = np.zeros((S, n_env), np.float64)
    count = np.zeros(n_env, np.float64)

    def policy(th, obs, h):
        ids = th[:, P].astype(np.int64)
        raw = (normalise(obs, affine) if record_seen else np.asarray(obs, np.float32)).astype(np.float64)
        s1[:, ids] = s1[:, ids] + raw.T                                 # (every env at most once per step)
        s2[:, ids] = s2[:, ids] + raw.T * raw.T
        count[ids] += 1.0
        action, _, act, _ = co.policy_forward(S, A, discrete, False, np.ascontiguousarray(th[:, :P]), normalise(obs, affine), None)
        return (action if discrete else act), None

    _, ep_ret, ep_steps = _host_rollout(name, aug, init, max_step, policy)
    ep_ret = ep_ret.reshape(N, E)
    ep_steps = ep_steps.reshape(N, E)
    assert np.array_equal(count, ep_steps.reshape(-1).astype(np.float64))
    fit = np.zeros(N)
    for e in range(E):
        fit = fit + ep_ret[:, e]
    return (fit / E).astype(np.float32), ep_ret, ep_steps, np.concatenate([count[None], s1, s2])


def reduce_envs(x):
    """the fixed-order sum of x float64[n_env]"""
    x = np.asarray(x, np.float64)
    lanes = np.zeros(LANES, np.float64)
    for lo in range(0, len(x), LANES):                                  # lane l: x[l], x[l + 256], ... ascending
        part = x[lo:lo + LANES]
        lanes[:len(part)] = lanes[:len(part)] + part
    s = LANES // 2
    while s >= 1:
        lanes[:s] = lanes[:s] + lanes[s:2 * s]
        s //= 2
    return np.float64(lanes[0])


def merge_component(n, mean, M2, nb, S1, S2):
    """-> (n', mean', M2', shift, scale), or None when the batch is empty (nothing is written)"""
    n, mean, M2, nb, S1, S2 = (np.float64(v) for v in (n, mean, M2, nb, S1, S2))
    if nb == 0.0:
        return None
    mb = S1 / nb
    M2b = max(S2 - S1 * mb, np.float64(0.0))
    N = n + nb
    f = nb / N
    d = mb - mean
    mean_new = mean + d * f
    M2_new = (M2 + M2b) + (d * d) * (n * f)
    std = np.sqrt(M2_new / (N - np.float64(1.0))) if N >= 2.0 else np.float64(1.0)
    shift = np.float32(mean_new)
    scale = np.float32(0.0) if std < STD_FLOOR else np.float32(np.float64(1.0) / std)
    return N, mean_new, M2_new, shift, scale


def merge(stats, affine, partials):
    """the merge launch: (stats', affine') from partials float64[2 S + 1, n_env]; the inputs are left alone"""
    stats = np.array(stats, np.float64)
    affine = np.array(affine, np.float32)
    S = stats.shape[0]
    assert partials.shape[0] == 2 * S + 1
    nb = reduce_envs(partials[0])
    for k in range(S):
        out = merge_component(stats[k, 0], stats[k, 1], stats[k, 2], nb, reduce_envs(partials[1 + k]), reduce_envs(partials[1 + S + k]))
        if out is not None:
            stats[k] = out[:3]
            affine[0, k], affine[1, k] = out[3], out[4]
    return stats, affine


def partials_of(x):
    """partials float64[3, n] of one component whose n envs took one step each with observation x[i] (crafted merges)"""
    x = np.asarray(x, np.float64)
    return np.stack([np.ones_like(x), x, x * x])
