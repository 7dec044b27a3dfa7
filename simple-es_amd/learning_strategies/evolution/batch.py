"""BatchedRuns -- R runs of one strategy that differ in a few scalars, advanced in lockstep as ONE device population.

A hyper-parameter sweep runs many short trials of one config; a single trial of 96 or 256 offspring uses a small fraction of the
chip, and the trials are independent.  Here the R trials' populations sit one behind the other in a [R n, P] matrix:

    per generation   one ses_rollout over all R n rows (rows are independent in every rollout kernel)
                     one ses_openai_generation_batch (csrc/ses_batch.hip): rank, gradient, Adam, next population per trial

and every trial computes, bit for bit, what builder.build_loop(config_r, ...).run() computes for it alone
(tests/test_gpu_batch.py).  What may differ between the trials: strategy.init_sigma, sigma_decay, learning_rate, seed and
env.seed.  Per trial the host keeps what openai_es keeps, by the same expressions (TrialSchedule); everything the device needs
of it is a function of the generation number, so it is computed and uploaded a chunk of generations ahead, like the env resets.
No blocking copy and no synchronisation per generation: the best rewards arrive in pinned memory and are read one generation
late.

simple_evolution and simple_genetic runs are batched the same way (ses_elite_generation_batch, csrc/ses_batch_elite.hip), but their
batch is RAGGED: strategy.elite_num may differ as well, and under simple_genetic it sets a trial's row count, so the trials sit at
the offsets of a BatchEliteLayout (row0, n, parent0) instead of a fixed stride.  EliteSchedule keeps what simple_genetic /
simple_evolution keep on the host, by their expressions; the yardstick is again the solo run (tests/test_gpu_batch_elite.py).
"""
import copy
import json
import math
import os
from datetime import datetime

import numpy as np
import torch

from learning_strategies.optimizers import Adam
from ses import BatchEliteLayout, HipES, MODE_EPISODIC, MODE_FIXED_LENGTH, _lib, param_count
from ses.parallel import world_size

# the keys that may differ between the trials of one batch; everything else of a config must be equal
VARYING = {"strategy": ("init_sigma", "sigma_decay", "learning_rate", "seed"), "env": ("seed",)}
ELITE_VARYING = {"strategy": ("init_sigma", "sigma_decay", "elite_num", "seed"), "env": ("seed",)}      # the elite strategies
SEPCMA_VARYING = {"strategy": ("init_sigma", "sigma_decay", "elite_num", "scale_limits", "step_limits", "seed"), "env": ("seed",)}
ARS_VARYING = {"strategy": ("init_sigma", "sigma_decay", "learning_rate", "elite_num", "seed"), "env": ("seed",)}
ELITE_STRATEGIES = {"simple_evolution": _lib.STRATEGY_SIMPLE_EVOLUTION, "simple_genetic": _lib.STRATEGY_SIMPLE_GENETIC}
BATCHED_STRATEGIES = ("openai_es",) + tuple(ELITE_STRATEGIES) + ("sep_cma_es", "ars")
_DEFAULTS = {("strategy", "noise"): "philox"}
_MISSING = object()

TRIAL_DTYPE = np.dtype(_lib.SesBatchTrial)      # ses_batch_trial of include/ses.h
ELITE_TRIAL_DTYPE = np.dtype(_lib.SesBatchEliteTrial)    # ses_batch_elite_trial
SEPCMA_TRIAL_DTYPE = np.dtype(_lib.SesBatchSepcmaTrial)  # ses_batch_sepcma_trial
SEPCMA_CONSTS_DTYPE = np.dtype(_lib.SesBatchSepcmaConsts)    # ses_batch_sepcma_consts
ARS_TRIAL_DTYPE = np.dtype(_lib.SesBatchArsTrial)        # ses_batch_ars_trial


def check_batchable(configs):
    """Raise ValueError, naming the key, unless the configs are runs of ONE batched strategy (openai_es, simple_evolution,
    simple_genetic, sep_cma_es, ars) that differ only in what may differ for it: VARYING, ELITE_VARYING, SEPCMA_VARYING, ARS_VARYING.
    A config with network.obs_normalizer is refused whatever the strategy: one population cannot share R normalisers."""
    if not configs:
        raise ValueError("BatchedRuns: no configs")
    first = configs[0]
    name = first.get("strategy", {}).get("name")
    varying = (ELITE_VARYING if name in ELITE_STRATEGIES else SEPCMA_VARYING if name == "sep_cma_es" else
               ARS_VARYING if name == "ars" else VARYING)
    for k, cfg in enumerate(configs):
        strategy = cfg.get("strategy", {})
        if strategy.get("name") != name:
            raise ValueError(f"BatchedRuns: trial {k} has strategy.name = {strategy.get('name')!r}, trial 0 has {name!r}; the trials of "
                             "a batch share one strategy")
        if name not in BATCHED_STRATEGIES:
            raise ValueError(f"BatchedRuns: trial {k} has strategy.name = {name!r}; only " + ", ".join(BATCHED_STRATEGIES)
                             + " runs are batched")
        if strategy.get("noise", "philox") != "philox":
            raise ValueError(f"BatchedRuns: trial {k} has strategy.noise = {strategy.get('noise')!r}; batched runs draw Philox noise")
        if (cfg.get("network") or {}).get("obs_normalizer", False):
            raise ValueError(f"BatchedRuns: trial {k} has network.obs_normalizer set; every run keeps a normaliser of its own and one "
                             "population cannot share R normalisers: such trials run one after the other")
        for block in sorted(set(first) | set(cfg)):
            a, b = first.get(block, _MISSING), cfg.get(block, _MISSING)
            if not (isinstance(a, dict) and isinstance(b, dict)):
                if a != b:
                    raise ValueError(f"BatchedRuns: trial {k} differs from trial 0 in {block}")
                continue
            for key in sorted(set(a) | set(b)):
                if key in varying.get(block, ()):
                    continue
                default = _DEFAULTS.get((block, key), _MISSING)
                if a.get(key, default) != b.get(key, default):
                    raise ValueError(f"BatchedRuns: trial {k} differs from trial 0 in {block}.{key} "
                                     f"({b.get(key)!r} against {a.get(key)!r}); only "
                                     + ", ".join(f"{blk}.{nm}" for blk, names in varying.items() for nm in names)
                                     + f" may differ between the {name} trials of a batch")


class TrialSchedule:
    """The host scalars of one openai_es run, stepped by the expressions of openai_es._generation: curr_sigma a Python float
    multiplied by sigma_decay after every evaluation, Adam's step scale from Adam.next_step_scale(), the Philox generation key
    bumped per population."""

    def __init__(self, strategy_cfg, pi=None):
        self.seed = int(strategy_cfg.get("seed", 0))
        self.learning_rate = strategy_cfg["learning_rate"]
        self.sigma_decay = strategy_cfg["sigma_decay"]
        self.init_sigma = strategy_cfg["init_sigma"]
        self.curr_sigma = self.init_sigma
        self.offspring_num = int(strategy_cfg["offspring_num"])
        self.optimizer = Adam(torch.zeros(0) if pi is None else pi, self.learning_rate)
        self.gen = 1                    # the key of the NEXT population; the initial one was drawn with key 0

    @property
    def t(self):
        return self.optimizer.t

    def step(self):
        """One evaluation: (the ses_batch_trial record of this generation, the sigma the evaluated population was drawn with)."""
        a = self.optimizer.next_step_scale()
        sigma = self.curr_sigma
        self.curr_sigma *= self.sigma_decay
        uf = self.learning_rate / (float(self.offspring_num) * sigma)      # offspring_strategies.py:406-408
        uf *= -1.0
        record = (self.seed & 0xFFFFFFFFFFFFFFFF, self.gen - 1, self.gen, a, np.float32(uf), np.float32(self.curr_sigma))
        self.gen += 1
        return record, sigma


def build_trial_table(schedules, gens, dtype=TRIAL_DTYPE):
    """Advance every schedule by `gens` generations: (ses_batch_trial records [gens, R], curr_sigma after each generation
    [gens][R]).  Every entry is a function of the generation number alone."""
    table = np.zeros((gens, len(schedules)), dtype=dtype)
    sigmas = []
    for g in range(gens):
        for r, s in enumerate(schedules):
            record, _ = s.step()
            table[g, r] = record
        sigmas.append([s.curr_sigma for s in schedules])
    return table, sigmas


class EliteSchedule:
    """The host scalars of one simple_genetic / simple_evolution run, stepped by the expressions of their evaluate_async: curr_sigma a
    Python float multiplied by sigma_decay once per evaluation -- simple_genetic draws the next population with the UNDECAYED value
    and decays afterwards, simple_evolution decays first -- and the Philox generation key bumped per population.  pop_sigma is the
    value the population under evaluation was drawn with: the elite rows are rebuilt with it."""
    t = 0                               # these strategies count no optimizer steps

    def __init__(self, strategy_cfg):
        self.name = strategy_cfg["name"]
        self.seed = int(strategy_cfg.get("seed", 0))
        self.sigma_decay = strategy_cfg["sigma_decay"]
        self.init_sigma = strategy_cfg["init_sigma"]
        self.curr_sigma = self.init_sigma
        self.pop_sigma = self.init_sigma        # the initial population: key 0, init_sigma
        self.elite_num = int(strategy_cfg["elite_num"])
        self.offspring_num = int(strategy_cfg["offspring_num"])
        self.gen = 1                    # the key of the NEXT population

    def step(self):
        """One evaluation: ((seed, gen, next_gen, pop_sigma, next_sigma) of ses_batch_elite_trial, pop_sigma as the Python float)."""
        pop_sigma = self.pop_sigma
        if self.name == "simple_genetic":
            next_sigma = self.curr_sigma                 # pop = self._offsprings_at(self.curr_sigma)
            self.curr_sigma *= self.sigma_decay          # decays AFTER regeneration
        else:
            self.curr_sigma *= self.sigma_decay
            next_sigma = self.curr_sigma                 # self._offsprings_at(self.curr_sigma)
        record = (self.seed & 0xFFFFFFFFFFFFFFFF, self.gen - 1, self.gen, np.float32(pop_sigma), np.float32(next_sigma))
        self.pop_sigma = next_sigma
        self.gen += 1
        return record, pop_sigma


def build_elite_trial_table(schedules, layout, gens):
    """Advance every schedule by `gens` generations: (ses_batch_elite_trial records [gens, R] with the layout's offsets, curr_sigma
    after each generation [gens][R])."""
    table = np.zeros((gens, len(schedules)), dtype=ELITE_TRIAL_DTYPE)
    sigmas = []
    for g in range(gens):
        for r, s in enumerate(schedules):
            record, _ = s.step()
            table[g, r] = record + (layout.row0[r], layout.n[r], layout.elite_num[r], layout.parent0[r])
        sigmas.append([s.curr_sigma for s in schedules])
    return table, sigmas


class SepCmaSchedule:
    """The host scalars of one sep_cma_es run, stepped by the expressions of sep_cma_es._generation: the update counter t, curr_sigma
    a Python float whose product with sigma_decay draws the next population, hsig_scale(t), the Philox generation key bumped per
    population.  Everything that adapts -- mu, C, the paths, the step -- lives on the device.  The class itself checks the block
    (offspring_num >= 4, elite_num in [1, n], the limits, Philox noise) and supplies its defaults: elite_num = n // 2."""

    def __init__(self, strategy_cfg, P):
        import builder
        from .offspring_strategies import sep_cma_constants
        checked = builder.build_strategy(strategy_cfg)          # no device is touched before init_offspring
        self.seed = checked.seed
        self.sigma_decay = checked.sigma_decay
        self.init_sigma = checked.init_sigma
        self.curr_sigma = self.init_sigma
        self.offspring_num, self.elite_num = checked.offspring_num, checked.elite_num
        self.scale_limits, self.step_limits = checked.scale_limits, checked.step_limits
        self.P = int(P)
        self.constants, _ = sep_cma_constants(self.offspring_num, self.P, self.elite_num)
        self.t = 0                      # updates done
        self.gen = 1                    # the key of the NEXT population; the initial one was drawn with key 0

    def hsig_scale(self, t):
        """1 / sqrt(1 - (1 - c_sigma)^(2 t)) of update t (from 1): sep_cma_es.hsig_scale"""
        return 1.0 / math.sqrt(1.0 - (1.0 - self.constants["c_sigma"]) ** (2.0 * float(t)))

    def step(self):
        """One evaluation: (the ses_batch_sepcma_trial record of this generation, the sigma the evaluated population was drawn with)."""
        t, sigma, next_sigma = self.t + 1, self.curr_sigma, self.curr_sigma * self.sigma_decay
        record = (self.seed & 0xFFFFFFFFFFFFFFFF, self.gen - 1, self.gen, self.hsig_scale(t), np.float32(sigma), np.float32(next_sigma))
        self.t, self.curr_sigma = t, next_sigma
        self.gen += 1
        return record, sigma


def build_sepcma_trial_table(schedules, gens):
    """build_trial_table for SepCmaSchedules: (ses_batch_sepcma_trial records [gens, R], curr_sigma after each generation [gens][R])"""
    return build_trial_table(schedules, gens, SEPCMA_TRIAL_DTYPE)


class ArsSchedule:
    """The host scalars of one ars run, stepped by the expressions of ars._generation: curr_sigma a Python float multiplied by
    sigma_decay after every evaluation, the Philox generation key bumped per population.  mu lives on the device and the step is
    formed there.  The class itself checks the block (offspring_num even and >= 4, elite_num in [1, n / 2], Philox noise) and supplies
    its default: elite_num = max(1, n // 4)."""
    t = 0                               # ars counts no optimizer steps

    def __init__(self, strategy_cfg):
        import builder
        checked = builder.build_strategy(strategy_cfg)          # no device is touched before init_offspring
        self.seed = checked.seed
        self.sigma_decay = checked.sigma_decay
        self.init_sigma = checked.init_sigma
        self.curr_sigma = self.init_sigma
        self.learning_rate = checked.learning_rate
        self.offspring_num, self.elite_num = checked.offspring_num, checked.elite_num
        self.gen = 1                    # the key of the NEXT population; the initial one was drawn with key 0

    def step(self):
        """One evaluation: (the ses_batch_ars_trial record of this generation, the sigma the evaluated population was drawn with)."""
        sigma = self.curr_sigma
        self.curr_sigma *= self.sigma_decay
        record = (self.seed & 0xFFFFFFFFFFFFFFFF, self.gen - 1, self.gen, self.learning_rate, np.float32(self.curr_sigma),
                  self.elite_num)
        self.gen += 1
        return record, sigma


def build_ars_trial_table(schedules, gens):
    """build_trial_table for ArsSchedules: (ses_batch_ars_trial records [gens, R], curr_sigma after each generation [gens][R])"""
    return build_trial_table(schedules, gens, ARS_TRIAL_DTYPE)


def sepcma_consts_record(c, P, scale_limits, step_limits):
    """One ses_batch_sepcma_consts block from sep_cma_constants' dict: the host expressions of ses_sepcma_generation
    (csrc/ses_sepcma.hip) in double, cast once; the limits pass through float32 like ses_sepcma_params' fields, the variance limits are
    float32 products."""
    f32 = np.float32
    P = float(P)
    scale_lo, scale_hi = f32(scale_limits[0]), f32(scale_limits[1])
    return (
        (1.4 + 2.0 / (P + 1.0)) * c["chi"],                                              # hsig_thr
        c["c_sigma"] / c["d_sigma"],                                                     # cs_over_ds
        c["chi"],
        f32(1.0 - c["c_sigma"]),                                                         # a_s
        f32(math.sqrt(c["c_sigma"] * (2.0 - c["c_sigma"]) * c["mueff"])),                # b_s
        f32(1.0 - c["c_c"]),                                                             # a_c
        f32(math.sqrt(c["c_c"] * (2.0 - c["c_c"]) * c["mueff"])),                        # hb1
        f32(c["c_1"]), f32(c["c_mu"]),                                                   # c1f, cmuf
        f32(1.0 - c["c_1"] - c["c_mu"] + 0.0),                                           # k0_h1
        f32(1.0 - c["c_1"] - c["c_mu"] + c["c_1"] * c["c_c"] * (2.0 - c["c_c"])),        # k0_h0
        scale_lo * scale_lo, scale_hi * scale_hi,                                        # var_lo, var_hi: float32 products
        f32(step_limits[0]), f32(step_limits[1]),
        int(c["mu"]), 0,
    )


def sepcma_batch_tables(n, P, elite_nums, scale_limits, step_limits):
    """The tables ses_sepcma_generation_batch reads besides the per-generation records, for trials of n rows and P parameters that
    select elite_nums[r] rows inside scale_limits[r] / step_limits[r]: (ses_batch_sepcma_consts blocks [R], the weight table
    float32[R, n] -- row r holds trial r's elite_nums[r] weights of sep_cma_constants, then zeros --, the constants dicts)."""
    from .offspring_strategies import sep_cma_constants
    R = len(elite_nums)
    consts = np.zeros(R, dtype=SEPCMA_CONSTS_DTYPE)
    weights = np.zeros((R, n), dtype=np.float32)
    dicts = []
    for r, mu in enumerate(elite_nums):
        c, w = sep_cma_constants(n, P, int(mu))
        consts[r] = sepcma_consts_record(c, P, scale_limits[r], step_limits[r])
        weights[r, :len(w)] = w
        dicts.append(c)
    return consts, weights, dicts


class BatchedRuns:
    K_MAX = 64                          # generations whose resets and trial records are prepared at once

    def __init__(self, configs, generation_num, eval_ep_num, save=True):
        configs = [copy.deepcopy(c) for c in configs]
        check_batchable(configs)
        if world_size() > 1:
            raise RuntimeError("BatchedRuns runs on one GPU: start it without torch.distributed.run")
        import builder
        from .loop import _rollout_device
        self.configs = configs
        self.R = len(configs)
        self.generation_num = int(generation_num)
        self.eval_ep_num = int(eval_ep_num)
        cfg = configs[0]
        self.n = int(cfg["strategy"]["offspring_num"])
        self.strategy_name = cfg["strategy"]["name"]
        self.layout = None                                  # the elite strategies: where the ragged trials sit
        if self.strategy_name in ELITE_STRATEGIES:
            try:
                self.layout = BatchEliteLayout(ELITE_STRATEGIES[self.strategy_name], self.n,
                                               [c["strategy"]["elite_num"] for c in configs])
            except _lib.SesError as e:
                raise ValueError(f"BatchedRuns: {e}") from None
        elif self.strategy_name == "sep_cma_es":
            if not _lib.BATCH_SEPCMA_MIN_N <= self.n <= _lib.BATCH_SEPCMA_MAX_N or self.R * self.n > _lib.BATCH_MAX_ROWS:
                raise ValueError(f"BatchedRuns: {self.R} trials of strategy.offspring_num = {self.n}; a sep_cma_es batch takes "
                                 f"{_lib.BATCH_SEPCMA_MIN_N} .. {_lib.BATCH_SEPCMA_MAX_N} rows per trial and {_lib.BATCH_MAX_ROWS} "
                                 "rows in all")
        elif self.strategy_name == "ars":
            if (not _lib.BATCH_ARS_MIN_N <= self.n <= _lib.BATCH_ARS_MAX_N or self.n % 2
                    or self.R * self.n > _lib.BATCH_MAX_ROWS):
                raise ValueError(f"BatchedRuns: {self.R} trials of strategy.offspring_num = {self.n}; an ars batch takes an even "
                                 f"number of {_lib.BATCH_ARS_MIN_N} .. {_lib.BATCH_ARS_MAX_N} rows per trial and "
                                 f"{_lib.BATCH_MAX_ROWS} rows in all")
        elif not 2 <= self.n <= _lib.BATCH_MAX_N or self.R * self.n > _lib.BATCH_MAX_ROWS:
            raise ValueError(f"BatchedRuns: {self.R} trials of strategy.offspring_num = {self.n}; a batch takes 2 .. "
                             f"{_lib.BATCH_MAX_N} rows per trial and {_lib.BATCH_MAX_ROWS} rows in all")
        self.env = builder.build_env(cfg["env"])
        self.network = builder.build_network(cfg["network"])
        self.network.zero_init()
        self.env_seeds = [int(c["env"].get("seed", 0)) for c in configs]
        self.shared_init = bool(cfg["env"].get("shared_init", False))
        self.mode = MODE_FIXED_LENGTH if cfg["env"].get("fixed_length", False) else MODE_EPISODIC
        net = self.network
        self.P = param_count(net.num_state, net.num_action, net.use_gru)
        if self.strategy_name == "sep_cma_es":
            self.schedules = [SepCmaSchedule(c["strategy"], self.P) for c in configs]
        elif self.strategy_name == "ars":
            self.schedules = [ArsSchedule(c["strategy"]) for c in configs]
        else:
            self.schedules = [(EliteSchedule if self.layout else TrialSchedule)(c["strategy"]) for c in configs]
        # two handles, like a solo run: the rollout's (env, horizon, episodes) and the tail's own scratch
        self.dev = _rollout_device(self.env, self.network, self.eval_ep_num)
        self.tail = HipES(None, net.num_state, net.num_action, net.discrete_action, net.use_gru)
        self.history = [[] for _ in range(self.R)]          # best reward per generation
        self.sigma_history = [[] for _ in range(self.R)]    # curr_sigma after each generation
        self.save_dirs = [self._make_save_dir() for _ in range(self.R)] if save else [None] * self.R
        self.mu = self.m = self.v = None
        self.parents_all = self.alias_state = None          # the elite strategies: [parents_total, P], int32[R] (evolution)
        self.C = self.p_sigma = self.p_c = self.step = None  # sep_cma_es: [R, P] and the step [R], next to mu

    # ---- what a solo run reports at its end -----------------------------------------------------------------
    @property
    def t(self):
        return [s.t for s in self.schedules]

    @property
    def curr_sigma(self):
        return [s.curr_sigma for s in self.schedules]

    def _make_save_dir(self):
        """logs/<env>/<timestamp>[_k], a directory of its own per trial (ESLoop.__init__)"""
        stamp = datetime.now().strftime("%Y%m%d%H%M%S")
        base, k = f"logs/{self.env.name}/{stamp}", 0
        while True:
            save_dir = base if k == 0 else f"{base}_{k}"
            try:
                os.makedirs(save_dir + "/saved_models/", exist_ok=False)
                return save_dir
            except FileExistsError:
                k += 1

    # ---- a chunk of generations ahead ------------------------------------------------------------------------
    def _prepare_chunk(self, gen0, gens):
        """The env resets [gens, R n, E, W] and the trial records [gens, R] of generations gen0 .. gen0 + gens - 1: each trial's
        resets are those of its own run (env seed, generation, row within the trial), a shared reset materialised per row."""
        if self.layout is not None:
            return self._prepare_elite_chunk(gen0, gens)
        dev, R, n = self.dev, self.R, self.n
        init = dev.empty(gens, R * n, dev.E, dev.init_dim)
        for r, seed in enumerate(self.env_seeds):
            own = dev.init_states_uniform_gens(seed, gen0, gens, 0, 1 if self.shared_init else n, shared=self.shared_init)
            init[:, r * n:(r + 1) * n] = own             # (a shared reset [gens, 1, E, W] broadcasts over the trial's rows)
        build = {"sep_cma_es": build_sepcma_trial_table, "ars": build_ars_trial_table}.get(self.strategy_name, build_trial_table)
        table, sigmas = build(self.schedules, gens)
        trials = torch.from_numpy(table.view(np.uint8).reshape(gens, R, table.dtype.itemsize)).to(dev.device)
        return gen0, init, trials, sigmas

    def _prepare_elite_chunk(self, gen0, gens):
        """The same for a ragged batch: trial r's resets are those of its own run of n_r rows, laid out at row0_r"""
        dev, lay = self.dev, self.layout
        init = dev.empty(gens, lay.rows_total, dev.E, dev.init_dim)
        for r, seed in enumerate(self.env_seeds):
            row0, n = int(lay.row0[r]), int(lay.n[r])
            own = dev.init_states_uniform_gens(seed, gen0, gens, 0, 1 if self.shared_init else n, shared=self.shared_init)
            init[:, row0:row0 + n] = own
        table, sigmas = build_elite_trial_table(self.schedules, lay, gens)
        trials = torch.from_numpy(table.view(np.uint8).reshape(gens, self.R, ELITE_TRIAL_DTYPE.itemsize)).to(dev.device)
        return gen0, init, trials, sigmas

    def _chunk_len(self, done):
        rows = self.layout.rows_total if self.layout is not None else self.R * self.n
        per_gen = rows * self.dev.E * self.dev.init_dim * 4
        return max(1, min(self.K_MAX, (32 << 20) // per_gen, self.generation_num - done))

    # ---- the run ------------------------------------------------------------------------------------------------
    def run(self):
        if self.layout is not None:
            return self._run_elite()
        if self.strategy_name == "sep_cma_es":
            return self._run_sepcma()
        if self.strategy_name == "ars":
            return self._run_ars()
        R, n, P, tail = self.R, self.n, self.P, self.tail
        state = [tuple(tail.zeros(R, P) for _ in range(3)), tuple(tail.empty(R, P) for _ in range(3))]
        theta = tail.empty(R * n, P)
        fitness = tail.empty(R * n)
        # the initial populations: row 0 of a trial is its (zero) mean, the others mean + init_sigma * noise of key 0
        idx = torch.zeros(n, dtype=torch.int32)
        idx[0] = -1
        idx = idx.to(tail.device)
        for r, s in enumerate(self.schedules):
            tail.perturb(state[0][0][r:r + 1], s.init_sigma, s.seed, 0, 0, n, parent_idx=idx, out=theta[r * n:(r + 1) * n],
                         idx_in_range=True)
        ring = [torch.full((R,), float("nan"), dtype=torch.float32).pin_memory() for _ in range(4)]
        cur, pending, chunk = 0, None, None
        for g in range(self.generation_num):
            if chunk is None or g >= chunk[0] + chunk[1].shape[0]:
                chunk = self._prepare_chunk(g, self._chunk_len(g))
            k = g - chunk[0]
            self.dev.rollout(theta, chunk[1][k], mode=self.mode, fitness=fitness)
            slot = ring[g % len(ring)]
            slot.fill_(float("nan"))                     # armed: the gradient kernel stores the trials' best rewards here
            tail.openai_generation_batch(fitness, n, chunk[2][k], state[cur], state[cur ^ 1], theta_next=theta, best=slot)
            cur ^= 1
            if pending is not None:
                self._collect(*pending)
            pending = (slot, chunk[3][k])
        if pending is not None:
            self._collect(*pending)
        torch.cuda.synchronize(tail.device)
        self.mu, self.m, self.v = state[cur]
        self._write_results()
        return self

    def _run_elite(self):
        """simple_evolution / simple_genetic: per generation one rollout over rows_total rows and one ses_elite_generation_batch"""
        lay, P, tail = self.layout, self.P, self.tail
        parents = [tail.zeros(lay.parents_total, P), tail.empty(lay.parents_total, P)]
        theta = tail.empty(lay.rows_total, P)
        fitness = tail.empty(lay.rows_total)
        alias = torch.ones(self.R, dtype=torch.int32, device=tail.device) if lay.evolution else None
        # the initial populations: zero parents, key 0, init_sigma, each trial's closed-form map into its own slice
        for r, s in enumerate(self.schedules):
            row0, n, p0 = int(lay.row0[r]), int(lay.n[r]), int(lay.parent0[r])
            rows = 1 if lay.evolution else int(lay.elite_num[r])
            idx = torch.from_numpy(lay.parent_map(r)).to(tail.device)
            tail.perturb(parents[0][p0:p0 + rows], s.init_sigma, s.seed, 0, 0, n, parent_idx=idx, out=theta[row0:row0 + n],
                         idx_in_range=True)
        ring = [torch.full((self.R,), float("nan"), dtype=torch.float32).pin_memory() for _ in range(4)]
        cur, pending, chunk = 0, None, None
        for g in range(self.generation_num):
            if chunk is None or g >= chunk[0] + chunk[1].shape[0]:
                chunk = self._prepare_chunk(g, self._chunk_len(g))
            k = g - chunk[0]
            self.dev.rollout(theta, chunk[1][k], mode=self.mode, fitness=fitness)
            slot = ring[g % len(ring)]
            slot.fill_(float("nan"))                     # armed: the rank kernel stores the trials' best rewards here
            tail.elite_generation_batch(fitness, lay, chunk[2][k], parents[cur], parents[cur ^ 1], alias_state=alias,
                                        theta_next=theta, best=slot)
            cur ^= 1
            if pending is not None:
                self._collect(*pending)
            pending = (slot, chunk[3][k])
        if pending is not None:
            self._collect(*pending)
        torch.cuda.synchronize(tail.device)
        self.parents_all, self.alias_state = parents[cur], alias
        self._write_results()
        return self

    def _run_sepcma(self):
        """sep_cma_es: per generation one rollout over R n rows and one ses_sepcma_generation_batch"""
        R, n, P, tail, sch = self.R, self.n, self.P, self.tail, self.schedules
        consts, weights, _ = sepcma_batch_tables(n, P, [s.elite_num for s in sch], [s.scale_limits for s in sch],
                                                 [s.step_limits for s in sch])
        consts = torch.from_numpy(consts.view(np.uint8).reshape(R, SEPCMA_CONSTS_DTYPE.itemsize)).to(tail.device)
        weights = torch.from_numpy(weights).to(tail.device)
        mus = [s.elite_num for s in sch]
        # (mu, C, p_sigma, p_c, step): zero mean, unit variances, zero paths, unit step
        state = [(tail.zeros(R, P), tail.zeros(R, P) + 1.0, tail.zeros(R, P), tail.zeros(R, P), tail.zeros(R) + 1.0),
                 tuple(tail.empty(R, P) for _ in range(4)) + (tail.empty(R),)]
        theta = tail.empty(R * n, P)
        fitness = tail.empty(R * n)
        # the initial populations: key 0, init_sigma, each trial's rows counted from its own first row
        mu0, C0, _, _, step0 = state[0]
        for r, s in enumerate(sch):
            tail.perturb_sepcma(mu0[r], C0[r], step0[r:r + 1], s.init_sigma, s.seed, 0, 0, n, out=theta[r * n:(r + 1) * n])
        ring = [torch.full((R,), float("nan"), dtype=torch.float32).pin_memory() for _ in range(4)]
        cur, pending, chunk = 0, None, None
        for g in range(self.generation_num):
            if chunk is None or g >= chunk[0] + chunk[1].shape[0]:
                chunk = self._prepare_chunk(g, self._chunk_len(g))
            k = g - chunk[0]
            self.dev.rollout(theta, chunk[1][k], mode=self.mode, fitness=fitness)
            slot = ring[g % len(ring)]
            slot.fill_(float("nan"))                     # armed: the sums kernel stores the trials' best rewards here
            tail.sepcma_generation_batch(fitness, n, mus, chunk[2][k], consts, weights, state[cur], state[cur ^ 1], theta_next=theta,
                                         best=slot)
            cur ^= 1
            if pending is not None:
                self._collect(*pending)
            pending = (slot, chunk[3][k])
        if pending is not None:
            self._collect(*pending)
        torch.cuda.synchronize(tail.device)
        self.mu, self.C, self.p_sigma, self.p_c, self.step = state[cur]
        self._write_results()
        return self

    def _run_ars(self):
        """ars: per generation one rollout over R n rows and one ses_ars_generation_batch"""
        R, n, P, tail, sch = self.R, self.n, self.P, self.tail, self.schedules
        bs = [s.elite_num for s in sch]
        state = [(tail.zeros(R, P),), (tail.empty(R, P),)]   # (mu,): the zero network
        theta = tail.empty(R * n, P)
        fitness = tail.empty(R * n)
        # the initial populations: key 0, init_sigma, a scale of ones, each trial's pairs counted from its own first row
        ones = torch.ones(P, dtype=torch.float32, device=tail.device)
        for r, s in enumerate(sch):
            tail.perturb_mirrored(state[0][0][r], ones, s.init_sigma, s.seed, 0, 0, n, out=theta[r * n:(r + 1) * n])
        ring = [torch.full((R,), float("nan"), dtype=torch.float32).pin_memory() for _ in range(4)]
        cur, pending, chunk = 0, None, None
        for g in range(self.generation_num):
            if chunk is None or g >= chunk[0] + chunk[1].shape[0]:
                chunk = self._prepare_chunk(g, self._chunk_len(g))
            k = g - chunk[0]
            self.dev.rollout(theta, chunk[1][k], mode=self.mode, fitness=fitness)
            slot = ring[g % len(ring)]
            slot.fill_(float("nan"))                     # armed: each trial's sigma_R workgroup stores its best reward here
            tail.ars_generation_batch(fitness, n, bs, chunk[2][k], state[cur], state[cur ^ 1], theta_next=theta, best=slot)
            cur ^= 1
            if pending is not None:
                self._collect(*pending)
            pending = (slot, chunk[3][k])
        if pending is not None:
            self._collect(*pending)
        torch.cuda.synchronize(tail.device)
        self.mu, = state[cur]
        self._write_results()
        return self

    def parents(self, r):
        """trial r's parents after the run: mu[P] (simple_evolution) or elites[elite_num, P], best first (simple_genetic)"""
        lay = self.layout
        p0 = int(lay.parent0[r])
        return self.parents_all[p0] if lay.evolution else self.parents_all[p0:p0 + int(lay.elite_num[r])]

    def _collect(self, slot, sigmas):
        """the best rewards of a generation whose successor is already enqueued"""
        host = slot.numpy()
        spins = 0
        while np.isnan(host).any():
            spins += 1
            if spins > 2000000:                          # give up polling, wait for the device (a NaN best means NaN returns)
                torch.cuda.synchronize(self.tail.device)
                break
        for r in range(self.R):
            self.history[r].append(float(host[r]))
            self.sigma_history[r].append(sigmas[r])

    def elite_model(self, r):
        """trial r's mean as a network (openai_es.get_elite_model, sep_cma_es's, ars's, simple_evolution's: mu), or its best elite
        (simple_genetic's)"""
        if self.layout is not None:
            vec = self.parents_all[int(self.layout.parent0[r])]
        else:
            vec = self.mu[r]
        return copy.deepcopy(self.network).load_flat(vec.detach().cpu().numpy())

    def _write_results(self):
        """per trial: metrics.jsonl and the final checkpoint, in the reference's .pt format (ESLoop's writer: the elite's state_dict)"""
        for r, save_dir in enumerate(self.save_dirs):
            if save_dir is None:
                continue
            with open(save_dir + "/metrics.jsonl", "a") as f:
                best = self.history[r]
                for g, (b, sigma) in enumerate(zip(best, self.sigma_history[r])):
                    tail = best[max(0, g - 4):g + 1]
                    f.write(json.dumps({"episode": g + 1, "best_reward": b, "curr_sigma": sigma,
                                        "ep5_mean_reward": sum(tail) / len(tail)}) + "\n")
            torch.save(self.elite_model(r).state_dict(), save_dir + "/saved_models" + f"/ep_{self.generation_num}.pt")

    def close(self):
        self.dev.close()
        self.tail.close()
