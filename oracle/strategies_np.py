"""numpy restatement of the reference's offspring strategies and Adam.

TEST INFRASTRUCTURE (oracle).  Each individual is ONE flat float32 vector in
`parameters()` order (networks/neural_network.py:46-56) instead of a
torch module; every arithmetic statement keeps the reference's numpy dtypes
and in-place semantics, so under the numpy installed here (2.2, NEP 50
promotion) the results are bit-identical to the reference -- this is pinned by
tests/test_oracle_golden.py against fixtures produced by importing the
reference (tests/golden/make_golden.py).

Restates (file:line into /root/reference/learning_strategies):
  simple_genetic     evolution/offspring_strategies.py:11-134
  simple_evolution   evolution/offspring_strategies.py:137-267
  openai_es          evolution/offspring_strategies.py:270-434
  Adam               optimizers.py:7-57

Object identity matters in the reference: a population slot is a
reference to a module, several slots can be the SAME module, and
`simple_evolution.evaluate` sums elites in place into elite[0].  Individuals
are therefore kept as numpy array objects and combined with the same in-place
operators, which reproduces the aliasing without special cases.

`noise` hook: callable(P, i) -> float64[P] standard normals for the i-th draw;
default draws from the global legacy numpy generator exactly like the
reference (`np.random.normal(size=shape)` per tensor == one flat stream).
"""
import numpy as np


def _np_noise(P, _i):
    return np.random.normal(size=P)


def rank_desc(rewards, stable=False):
    """np.flip(np.argsort(rewards)) (offspring_strategies.py:112,234,380).

    stable=True is the tie rule the device kernels implement
    (reward descending, then index descending); for tie-free input both agree."""
    r = np.array(rewards)
    return np.flip(np.argsort(r, kind="stable" if stable else None))


def centered_ranks(rewards, stable=False):
    """offspring_strategies.py:380-398 -> float64[n] shaped rewards."""
    order = rank_desc(rewards, stable)
    n = len(rewards)
    reward_array = np.zeros(n)
    for idx in reversed(range(n)):
        reward_array[order[idx]] = ((n - 1 - idx) / (n - 1)) - 0.5
    r_std = reward_array.std()
    return (reward_array - reward_array.mean()) / r_std


def episode_fitness(ep_return):
    """float64[n, E] per-episode returns -> float32[n] fitness: the sequential float64 sum over the episodes, / E, rounded
    once (loop.py:124; the device's episode-mean kernel and the fused tails that form the mean themselves)."""
    ep = np.asarray(ep_return, dtype=np.float64)
    total = np.zeros(ep.shape[0])
    for e in range(ep.shape[1]):
        total += ep[:, e]
    return (total / ep.shape[1]).astype(np.float32)


def stable_rank(rewards):
    """int32[n]: rank[i] = position of offspring i in rank_desc(rewards, stable=True) (0 = best)."""
    order = rank_desc(rewards, stable=True)
    rank = np.empty(len(order), np.int32)
    rank[order] = np.arange(len(order), dtype=np.int32)
    return rank


def elite_select(rank, k, parent_map, alias_state=None):
    """The elite bookkeeping of one generation (include/ses.h ses_elite_select): (ids[k], parent_idx[k], alias_first[k] or
    None, the new alias state or None).  alias_state is simple_evolution's "population slots 0 and 1 are the same module
    object" (offspring_strategies.py:234-248 sums the elites into elite 0 in place)."""
    rank = np.asarray(rank)
    ids = np.empty(k, np.int32)
    for i in np.flatnonzero(rank < k):
        ids[rank[i]] = i
    pidx = np.asarray(parent_map, np.int32)[ids]
    if alias_state is None:
        return ids, pidx, None, None
    first = int(ids[0])
    alias = np.zeros(k, np.int32)
    if alias_state and first in (0, 1):
        alias[1:] = [1 if int(j) in (0, 1) and int(j) != first else 0 for j in ids[1:]]
    state = int(first == 0 or (first == 1 and bool(alias_state)))
    return ids, pidx, alias, state


def elite_mean(rows, alias_first=None):
    """The reference's in-place float32 elite sum, / k (offspring_strategies.py:241-248): an elite flagged in alias_first is
    the same object as elite 0, so `mu += elite` doubles the running sum there."""
    rows = np.asarray(rows, np.float32)
    mean = rows[0].copy()
    for j in range(1, rows.shape[0]):
        mean += mean if (alias_first is not None and alias_first[j]) else rows[j]
    mean /= rows.shape[0]
    return mean


ES_CHUNK = 1024                    # rows per gradient workgroup (csrc/ses_strategy.hip ES_CHUNK)
ES_THREADS = 256                   # threads per gradient workgroup: rows c, c + 256, ... of a chunk; an LDS tree over them
F32_U = 2.0 ** -24                 # unit roundoff of float32
WEIGHT_ATOL = 1e-12                # |device closed-form weight - centered_ranks| (k_rank_weights; tests/test_gpu_parity.py)


def es_grad_rounding_count(n):
    """K: the most roundings any one term w_i * z_ip meets on its way into the device's float32 gradient.

    per thread: ES_CHUNK / ES_THREADS = 4 fmas (a term enters at one of them and is rounded by it and every later one);
    the LDS tree: log2(ES_THREADS) = 8 additions; the ordered sum of the chunk partials: `chunks` additions (chunks - 1
    would do; one is spare); 3 more: the float cast of the weight, the float cast of uf and the final multiply."""
    chunks = -(-n // ES_CHUNK)
    return ES_CHUNK // ES_THREADS + int(np.log2(ES_THREADS)) + chunks + 3


def es_grad_tolerance(n, uf, s_abs, z_abs):
    """tol[P] for |grad_device - g64| from the float64 magnitudes of the sum (see es_grad_f64)."""
    K = es_grad_rounding_count(n)
    gamma = K * F32_U / (1.0 - K * F32_U)
    return gamma * s_abs + (1.0 + gamma) * abs(uf) * WEIGHT_ATOL * z_abs


def es_chunk_sums_f64(weights, seed, gen, P, skip_row0=True, noise=None, threads=None):
    """Per-chunk float64 sums of the ES gradient: (S[chunks, P], A[chunks, P], Z[chunks, P]) with, over the rows i of chunk c,
    S = sum w_i z_ip, A = sum |w_i z_ip|, Z = sum |z_ip|; row 0 contributes nothing when skip_row0.

    z = noise(seed, gen, first_row, n_rows, P) (default: the C oracle's Philox normals, bit-identical to the device's),
    generated one chunk at a time (never more than a 1024 x P block per worker), on a few threads: the C call and the
    matrix products release the GIL."""
    if noise is None:
        from oracle import c_oracle
        noise = c_oracle.noise
    w = np.asarray(weights, dtype=np.float64)
    n = len(w)
    chunks = -(-n // ES_CHUNK)

    def one(c):
        r0, r1 = c * ES_CHUNK, min(n, (c + 1) * ES_CHUNK)
        z = noise(seed, gen, r0, r1 - r0, P).astype(np.float64)
        if skip_row0 and r0 == 0:
            z[0] = 0.0
        az = np.abs(z)
        return w[r0:r1] @ z, np.abs(w[r0:r1]) @ az, az.sum(axis=0)

    if threads is None:
        import os
        threads = max(1, min(8, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 1))
    if threads > 1 and chunks > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(threads) as ex:
            parts = list(ex.map(one, range(chunks)))
    else:
        parts = [one(c) for c in range(chunks)]
    return tuple(np.stack([p[k] for p in parts]) for k in range(3))


def es_grad_f64(fitness, seed, gen, P, lr, sigma, skip_row0=True, noise=None):
    """The openai_es gradient in float64 and a rigorous bound on the device's float32 error: (g64[P], s_abs[P], tol[P]).

        g64_p   = uf * sum_{i >= skip_row0} w_i z_ip,     uf = -lr / (n * sigma)     (offspring_strategies.py:401-414)
        s_abs_p = |uf| * sum_{i >= skip_row0} |w_i z_ip|
        tol_p   = gamma_K * s_abs_p + (1 + gamma_K) * |uf| * 1e-12 * sum_i |z_ip|,   gamma_K = K u / (1 - K u), u = 2^-24

    w = centered_ranks(fitness, stable=True) (the reference's definition, ties by index descending), z the Philox normals of
    (seed, gen, row, parameter).

    Derivation.  The device (k_es_grad_partial[_ranked] + k_es_apply / its fused forms) evaluates
        g = fl(fl(uf) * fl(sum over chunks in ascending order of fl(tree over 256 threads of fl(fma chain over <= 4 rows))))
    with float32 products fl(w_i) * z_ip where z_ip is bit-identical to the oracle's float32 normal.  Every operation is one
    float32 rounding, x (1 + d) with |d| <= u, and by the standard argument for recursive summation (Higham, Accuracy and
    Stability of Numerical Algorithms, 2nd ed., Lemma 3.1 and section 4.2) the computed value is
        sum_i uf * w'_i * z_ip * prod_{k <= K_i} (1 + d_ik),     K_i <= K = es_grad_rounding_count(n),
    and |prod (1 + d) - 1| <= gamma_K.  So |g - uf * sum w'_i z_ip| <= gamma_K * |uf| * sum |w'_i z_ip|.  The weights w'_i the
    device uses are its closed form of the rank grid, |w'_i - w_i| <= 1e-12; that moves the exact sum by at most
    |uf| * 1e-12 * sum |z_ip|, and the same rounding factors at most (1 + gamma_K) times that.  Evaluating g64 itself in float64
    adds at most ~n * 2^-53 * s_abs, below 1e-5 of gamma_K * s_abs for every n this library accepts: ignored.
    A kernel that is right can never exceed tol; one that adds a term too many, too few or a wrong term does so as soon as
    that term is larger than tol -- tests/test_es_grad_bound.py measures how often."""
    fitness = np.asarray(fitness, dtype=np.float32)
    n = len(fitness)
    w = centered_ranks(fitness, stable=True)
    S, A, Z = es_chunk_sums_f64(w, seed, gen, P, skip_row0=skip_row0, noise=noise)
    uf = lr / (n * sigma)
    uf *= -1.0
    g64 = uf * S.sum(axis=0)
    s_abs = abs(uf) * A.sum(axis=0)
    return g64, s_abs, es_grad_tolerance(n, uf, s_abs, Z.sum(axis=0))


class AdamNP:
    """optimizers.py:30-57 on one flat vector (beta1 = 0.99 as in the reference)."""

    def __init__(self, theta, stepsize, beta1=0.99, beta2=0.999, epsilon=1e-08):
        self.theta = theta              # float32[P], updated in place
        self.stepsize = stepsize
        self.beta1 = beta1
        self.beta2 = beta2
        self.epsilon = epsilon
        self.t = 0
        self.m = np.zeros_like(theta)
        self.v = np.zeros_like(theta)

    def step_scale(self):
        return self.stepsize * np.sqrt(1 - self.beta2 ** self.t) / (1 - self.beta1 ** self.t)

    def update(self, grad):
        self.t += 1
        a = self.step_scale()
        self.m = self.beta1 * self.m + (1 - self.beta1) * grad
        self.v = self.beta2 * self.v + (1 - self.beta2) * (grad * grad)
        step = -a * self.m / (np.sqrt(self.v) + self.epsilon)
        self.theta += step
        return step


class OpenAIESNP:
    def __init__(self, P, init_sigma, sigma_decay, learning_rate, offspring_num, noise=_np_noise, stable_rank=False):
        self.P = P
        self.offspring_num = offspring_num
        self.sigma_decay = sigma_decay
        self.learning_rate = learning_rate
        self.curr_sigma = init_sigma
        self.noise = noise
        self.stable_rank = stable_rank
        self.mu = np.zeros(P, dtype=np.float32)          # zero_init, loop.py:31
        self.optimizer = AdamNP(self.mu, learning_rate)
        self.epsilons = []
        self.draws = 0
        self.population = self._gen()

    def _gen(self):
        self.epsilons = [self.mu.copy()]                 # :303-308 "zero" net keeps mu's values
        pop = [self.mu.copy()]                           # :310 member 0 = mu
        for _ in range(self.offspring_num - 1):
            epsilon = self.noise(self.P, self.draws)
            self.draws += 1
            eps_param = self.mu.copy()                   # :316 deepcopy(zero_net_param_list)
            perturb = self.mu.copy()
            eps_param += epsilon                         # :321
            perturb += epsilon * self.curr_sigma         # :322
            pop.append(perturb)
            self.epsilons.append(eps_param)
        return pop

    def theta(self):
        return np.stack(self.population)

    def evaluate(self, rewards):
        best_reward = max(rewards)
        reward_array = centered_ranks(rewards, self.stable_rank)
        grad = np.zeros(self.P, dtype=np.float32)        # :401-404
        update_factor = self.learning_rate / (len(self.epsilons) * self.curr_sigma)
        update_factor *= -1.0
        for offs_idx, offs in enumerate(self.epsilons):
            grad += offs * reward_array[offs_idx]        # :412
        grad *= update_factor                            # :414
        self.last_grad = grad.copy()
        self.last_weights = reward_array
        self.optimizer.update(grad)                      # :416
        self.curr_sigma *= self.sigma_decay              # :418
        self.population = self._gen()
        return best_reward, self.curr_sigma


class SimpleEvolutionNP:
    def __init__(self, P, init_sigma, sigma_decay, elite_num, offspring_num, noise=_np_noise, stable_rank=False):
        self.P = P
        self.elite_num = elite_num
        self.offspring_num = offspring_num
        self.sigma_decay = sigma_decay
        self.curr_sigma = init_sigma
        self.noise = noise
        self.stable_rank = stable_rank
        self.draws = 0
        net = np.zeros(P, dtype=np.float32)
        self.elite_models = [net for _ in range(elite_num)]   # :201 same object k times
        self.mu_model = self.elite_models[0]
        self.population = self._gen()

    def _gen(self):
        pop = [self.mu_model, self.elite_models[0]]      # :166-167 references, no copy
        for _ in range(self.offspring_num - 1):
            child = self.mu_model.copy()
            epsilon = self.noise(self.P, self.draws) * self.curr_sigma   # normal(0, sigma) = sigma * z
            self.draws += 1
            child += epsilon                             # :174
            pop.append(child)
        return pop

    def theta(self):
        return np.stack(self.population)

    def evaluate(self, rewards):
        elite_ids = rank_desc(rewards, self.stable_rank)[: self.elite_num]
        best_reward = max(rewards)
        self.elite_ids = np.array(elite_ids)
        self.elite_models = [self.population[i] for i in elite_ids]
        new_mu = self.elite_models[0]                    # :241 views of elite[0]: in-place sum
        for elite in self.elite_models[1:]:
            new_mu += elite                              # :245 (aliasing doubles when elite is elite[0])
        new_mu /= self.elite_num                         # :248
        # :250 apply_param copies the values into mu_model (which keeps its own identity)
        if self.mu_model is not new_mu:
            self.mu_model[...] = new_mu
        self.curr_sigma *= self.sigma_decay              # :251
        self.population = self._gen()
        return best_reward, self.curr_sigma


class SimpleGeneticNP:
    def __init__(self, P, init_sigma, sigma_decay, elite_num, offspring_num, noise=_np_noise, stable_rank=False):
        self.P = P
        self.elite_num = elite_num
        self.offspring_num = offspring_num
        self.sigma_decay = sigma_decay
        self.curr_sigma = init_sigma
        self.noise = noise
        self.stable_rank = stable_rank
        self.draws = 0
        net = np.zeros(P, dtype=np.float32)
        self.elite_models = [net for _ in range(elite_num)]   # :84
        self.population = self._gen()

    def _gen(self):
        pop = []
        for p in self.elite_models:
            pop.append(p)                                # :51 the elite itself
            for _ in range((self.offspring_num // self.elite_num) - 1):
                child = p.copy()
                child += self.noise(self.P, self.draws) * self.curr_sigma   # :57-58
                self.draws += 1
                pop.append(child)
        return pop

    def theta(self):
        return np.stack(self.population)

    def evaluate(self, rewards):
        elite_ids = rank_desc(rewards, self.stable_rank)[: self.elite_num]
        best_reward = max(rewards)
        self.elite_ids = np.array(elite_ids)
        self.elite_models = [self.population[i] for i in elite_ids]
        self.population = self._gen()                    # :117 uses the un-decayed sigma
        self.curr_sigma *= self.sigma_decay              # :124 decay AFTER regeneration
        return best_reward, self.curr_sigma
