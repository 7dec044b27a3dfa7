"""simple_genetic / simple_evolution / openai_es with the reference's constructor signatures and methods
(learning_strategies/evolution/offspring_strategies.py:11-434), re-designed around a device-resident
population:

  reference                                    here
  -----------------------------------------    -----------------------------------------------------------
  list of N {agent_id: torch module}           Population: float32[N_local, P] on the GPU (+ lazy module view)
  deepcopy + np.random.normal per offspring    one Philox perturbation kernel over the shard (ses_perturb)
  python argsort / rank loop / z-score         ses_rank_center (exact counting rank, float64 weights)
  python sum over N modules + numpy Adam       ses_es_update_* (ES gradient + Adam fused)
  in-place elite sum over modules              ses_elite_ids / ses_perturb(row_ids) / ses_elite_mean

Population layouts and quirks are kept: openai_es has N members with member 0 = mu;
simple_evolution has N+1 = [mu, elite0, N-1 children] and its elite "mean" reproduces the reference's
in-place aliasing; simple_genetic has k*(N//k) members and decays sigma AFTER regenerating.

noise="philox" (default): counter-based device noise; any GPU count gives the same population.
noise="numpy": the reference's own stream -- float64 draws from the global numpy generator, uploaded and
applied on the device with the reference's float64->float32 rounding; with the same seed the populations
and parent updates are bit-identical to the reference (single process only).
"""
import math

import numpy as np
import torch

from learning_strategies.optimizers import Adam
from ses import HipES
from ses.parallel import Shard, attach_comm

from .abstracts import BaseOffspringStrategy
from .utils import wrap_agentid


class Population:
    """The offspring group handed from a strategy to ESLoop.  Device view: `theta` (this rank's rows);
    sequence view (len / index / iterate) materialises {agent_id: module} dicts like the reference's list."""

    def __init__(self, theta, shard, network, agent_ids, gen):
        self.theta = theta            # float32[n_local, P] on the device
        self.shard = shard
        self.gen = gen                # generation counter (keys the env-init Philox stream in ESLoop)
        self._network = network
        self._agent_ids = agent_ids

    def __len__(self):
        return self.shard.n_global

    def __getitem__(self, i):
        if not 0 <= i < self.shard.n_global:
            raise IndexError(i)
        j = i - self.shard.first
        if not 0 <= j < self.shard.n_local:
            raise IndexError(f"offspring {i} lives on another rank")
        import copy
        net = copy.deepcopy(self._network).load_flat(self.theta[j].cpu().numpy())
        return wrap_agentid(self._agent_ids, net)

    def __iter__(self):
        return (self[i] for i in range(self.shard.first, self.shard.first + self.shard.n_local))


class PendingReward:
    """best_reward of a generation, read back without stalling the thread that enqueues the next one and without an
    event in the launch stream: the kernel that finds the maximum stores it straight into pinned host memory, which
    the host pre-set to NaN when it enqueued the generation; result() polls until the value is there (falling back to
    a stream synchronisation if it does not appear -- a NaN maximum would mean NaN returns)."""

    def __init__(self, host):
        self._host, self._value = host, None

    def result(self):
        if self._value is None:
            v = float(self._host[0])
            spins = 0
            while v != v:
                spins += 1
                if spins > 2000000:                     # ~seconds: give up polling, wait for the device
                    torch.cuda.synchronize()
                    v = float(self._host[0])
                    break
                v = float(self._host[0])
            self._value = v
        return self._value


class _ReadbackRing:
    """`depth` pinned host floats reused round-robin (the loop keeps at most two generations in flight).  `best` is the
    slot the current generation's kernels write -- host memory the GPU can store to, so neither a copy nor an event sits
    in the launch stream (a queued 4-byte device-to-host copy cost ~10 us of stream time per generation, an event ~5)."""

    def __init__(self, device, depth=4):
        self.slots = [torch.full((1,), float("nan"), dtype=torch.float32).pin_memory() for _ in range(depth)]
        self.k = 0

    @property
    def best(self):
        return self.slots[self.k]

    def arm(self):
        """call BEFORE enqueueing the kernels that write `best`: marks the slot as pending"""
        self.slots[self.k][0] = float("nan")
        return self.slots[self.k]

    def push(self):
        host = self.slots[self.k]
        self.k = (self.k + 1) % len(self.slots)
        return PendingReward(host)


class _DeviceStrategy(BaseOffspringStrategy):
    # What ses_run_generations has to know of a strategy it serves; the class declares it in its OWN body (a subclass that does
    # not repeat _STRATEGY may have changed evaluate() and stays on the per-generation path: loop.py, _GenerationBatch.eligible)
    _STRATEGY = None                   # the _lib.STRATEGY_* name of ses_gen_state.strategy
    # (snapshot key, attribute, ses_gen_state field) of every state vector, the one whose field is `parents` first: the ping-pong of
    # evaluate_async, snapshot / restore and the C loop's buffers (loop.py: _GenerationBatch) all follow this table
    _STATE = ()
    _C_LOOP_ONE_GPU = False            # True: ses_run_generations has no multi-GPU form of this tail
    t = 0                              # updates done; a strategy that counts none reports 0 and gets 0 back

    def __init__(self, init_sigma, sigma_decay, offspring_num, noise, seed):
        if noise not in ("philox", "numpy"):
            raise ValueError("noise must be 'philox' or 'numpy'")
        self.offspring_num = offspring_num
        self.init_sigma = init_sigma
        self.sigma_decay = sigma_decay
        self.curr_sigma = init_sigma
        self.noise = noise
        self.seed = int(seed)
        self.gen = 0                  # bumped by every _gen_offsprings: Philox generation key
        self.dev = None
        self._elite_ids_dev = None
        self._spare = None            # the buffers evaluate_async writes the next state vectors into
        self._maps = {}               # _const_map
        self._idx_cache = None        # _materialise: (this rank's slice of the parent map, its device copy, the map)
        self._map_dev = None          # _select_elites: (the parent map, its device copy)

    # ---- plumbing -----------------------------------------------------------------------------
    def _bind(self, network, agent_ids):
        self.agent_ids = agent_ids
        self.network = network
        network.zero_init()           # every strategy starts from the zero network (offspring_strategies.py:83,200,348)
        self.dev = HipES(None, network.num_state, network.num_action, network.discrete_action, network.use_gru)
        # multi-GPU: the shard form of the openai_es tail exchanges its chunk partials over the transports ESLoop attached
        # (attach_comm there is the collective one).  Here: reuse only -- a strategy built on some ranks never starts a rendezvous
        attach_comm(self.dev, create=False)
        self.P = self.dev.P
        self._ring = _ReadbackRing(self.dev.device)
        self._shards = {}

    def _shard(self, n):
        sh = self._shards.get(n)
        if sh is None:
            sh = self._shards[n] = Shard(n)
        return sh

    def _const_map(self, key, build):
        """The parent map of a strategy depends only on (elite_num, offspring_num): built once, so that the identity
        checks of the upload caches below hit every generation."""
        if key not in self._maps:
            self._maps[key] = build()
        return self._maps[key]

    def evaluate(self, rewards):
        """(offspring_group, best_reward, curr_sigma) like the reference; best_reward is read back here."""
        pop, best, sigma = self.evaluate_async(rewards)
        return pop, best.result(), sigma

    # ---- the state vectors: ONE dev.*_generation call per generation moves them between two sets of buffers ----------------
    def _state(self):
        return tuple(getattr(self, attr) for _, attr, _ in self._STATE)

    def _set_state(self, vectors):
        for (_, attr, _), x in zip(self._STATE, vectors):
            setattr(self, attr, x)

    def _gen_state_constants(self):
        """{ses_gen_state field: value} of what the C loop needs besides the state vectors and the public attributes
        (learning_rate, sigma_decay, seed); a tensor stands for its address"""
        return {}

    def _loop_parent_map(self):
        """the host parent map of the populations ses_run_generations draws, which _last["idx_host"] holds after a hand-back"""
        return self._last["idx_host"]

    def _generation(self, fit, state_in, state_out, shard, best):
        """the one dev.*_generation call and the host scalars that move with it; returns theta of the next population"""
        raise NotImplementedError

    def evaluate_async(self, rewards):
        """evaluate() without the read-back: best_reward comes as a PendingReward (result() waits for it).  On a sharded run
        every rank gets the gathered fitness and computes the same update (the replicated tail); theta covers its own rows."""
        fit = self._fitness_tensor(rewards)
        state_in = self._state()
        if self._spare is None:
            self._spare = tuple(torch.empty_like(x) for x in state_in)
        state_out = self._spare
        shard = self._shard(self.offspring_num)
        theta = self._generation(fit, state_in, state_out, shard, self._ring.arm())
        best = self._ring.push()
        self._spare = state_in
        self._set_state(state_out)
        return self._population(theta, shard, self.curr_sigma, self._last["idx_host"]), best, self.curr_sigma

    def _population(self, theta, shard, sigma, parent_idx_host):
        """`theta` as the current population: this rank's rows of (the state vectors, the parent map, sigma, self.gen)"""
        self._last = {"parents": getattr(self, self._STATE[0][1]).view(-1, self.P), "idx_host": parent_idx_host, "sigma": sigma,
                      "gen": self.gen, "shard": shard}
        pop = Population(theta, shard, self.network, self.agent_ids, self.gen)
        self.gen += 1
        return pop

    def _population_size(self):
        raise NotImplementedError

    def _materialise(self, parents, parent_idx_host, sigma):
        """Build this rank's rows of the population described by (parents[K,P], parent_idx[N])."""
        n = len(parent_idx_host)
        shard = self._shard(n)
        if self.noise == "numpy" and shard.world != 1:
            raise RuntimeError("noise='numpy' reproduces the reference's single global stream: run it on one process")
        lo, hi = shard.first, shard.first + shard.n_local
        cached = self._idx_cache                       # the parent map is the same every generation: upload it once
        if cached is None or cached[2] is not parent_idx_host:
            local_idx = np.ascontiguousarray(parent_idx_host[lo:hi], dtype=np.int32)
            if cached is None or cached[0].shape != local_idx.shape or not np.array_equal(cached[0], local_idx):
                cached = (local_idx.copy(), torch.from_numpy(local_idx).to(self.dev.device), parent_idx_host)
            else:
                cached = (cached[0], cached[1], parent_idx_host)
            self._idx_cache = cached
        idx = cached[1]
        self._last = {"parents": parents, "idx_host": parent_idx_host, "sigma": sigma, "gen": self.gen, "shard": shard}
        if shard.n_local == 0:                      # more ranks than offspring: this rank idles through the rollout
            theta = self.dev.empty(0, self.P)
        elif self.noise == "philox":
            theta = self.dev.perturb(parents, sigma, self.seed, self.gen, lo, shard.n_local, parent_idx=idx)
        else:
            eps = np.zeros((n, self.P))
            for i in range(n):                     # the reference draws only for perturbed members, in order
                if parent_idx_host[i] >= 0:
                    eps[i] = np.random.normal(size=self.P)
            eps64 = torch.from_numpy(eps).to(self.dev.device)
            theta, store = self.dev.perturb_host_noise(parents, eps64, sigma, parent_idx=idx, want_eps_store=True)
            self._last["eps_store"] = store
            self._last["theta"] = theta
        pop = Population(theta, shard, self.network, self.agent_ids, self.gen)
        self.gen += 1
        return pop

    def _rows(self, ids_host):
        """Parameter rows of the CURRENT population for global ids (any rank can rebuild any row)."""
        last = self._last
        ids = np.asarray(ids_host, dtype=np.int32)
        if self.noise == "numpy":
            return self.dev.gather_rows(last["theta"], torch.from_numpy(ids).to(self.dev.device))
        sel = np.ascontiguousarray(last["idx_host"][ids])
        K = last["parents"].shape[0] if last["parents"].dim() == 2 else 1
        if sel.size and (sel.max() >= K or sel.min() < -K):
            raise ValueError("parent map out of range")
        both = torch.from_numpy(np.stack([sel, ids])).to(self.dev.device)          # one upload for both index rows
        return self.dev.perturb(last["parents"], last["sigma"], self.seed, last["gen"], 0, len(ids),
                                parent_idx=both[0], row_ids=both[1], idx_in_range=True)

    def _select_elites(self, rank, k, alias_state=None):
        """Elite ids, their rows and (simple_evolution) the aliasing flags without a host round trip: one
        ses_elite_select launch on the rank vector and the device copy of the current parent map."""
        last = self._last
        cached = self._map_dev                            # whole-population map on the device, uploaded once
        if cached is None or (cached[0] is not last["idx_host"] and not np.array_equal(cached[0], last["idx_host"])):
            cached = (last["idx_host"], torch.from_numpy(np.ascontiguousarray(last["idx_host"], dtype=np.int32)).to(self.dev.device))
            self._map_dev = cached
        ids, sel, alias = self.dev.elite_select(rank, k, cached[1], alias_state)
        self._elite_ids_dev = ids
        if self.noise == "numpy":
            rows = self.dev.gather_rows(last["theta"], ids)
        else:
            # the elite rows are not "the next population": this launch must not write the loop's tail time stamp
            # (ses_set_stamp), or eval_t could be read before the population-writing launch has stamped it
            keep = getattr(self.dev, "_stamp_keepalive", None)
            if keep is not None:
                self.dev.set_stamp(None)
            rows = self.dev.perturb(last["parents"], last["sigma"], self.seed, last["gen"], 0, k,
                                    parent_idx=sel, row_ids=ids, idx_in_range=True)   # map checked at upload
            if keep is not None:
                self.dev.set_stamp(keep)
        return rows, alias

    @property
    def elite_ids(self):
        """Global ids of the last elite selection (host copy on demand; the loop itself never reads them back)."""
        return None if self._elite_ids_dev is None else self._elite_ids_dev.cpu().numpy()

    def _fitness_tensor(self, rewards):
        if (isinstance(rewards, torch.Tensor) and rewards.dtype == torch.float32 and rewards.device == self.dev.device
                and rewards.is_contiguous() and rewards.numel() == self._population_size()):
            return rewards.view(-1)
        if isinstance(rewards, torch.Tensor):
            fit = rewards.to(device=self.dev.device, dtype=torch.float32).contiguous()
        else:
            fit = torch.as_tensor(np.asarray(rewards, dtype=np.float32)).to(self.dev.device)
        if fit.numel() != self._population_size():
            raise ValueError(f"expected {self._population_size()} rewards, got {fit.numel()}")
        return fit

    def _model_from(self, vec):
        import copy
        return copy.deepcopy(self.network).load_flat(vec.detach().cpu().numpy())

    # ---- roll-back support (ESLoop.run: a multi-GPU exchange that timed out is replayed from the last boundary) -------
    def snapshot(self, population):
        """Everything the next generations depend on, as device clones + host scalars, taken while `population` (the
        group evaluate() has just returned) is the current one.  restore() rebuilds that population bit for bit: the
        noise is a pure function of (seed, generation key, row, column)."""
        snap = {"curr_sigma": self.curr_sigma, "pop_gen": population.gen, "pop_sigma": self._last["sigma"]}
        snap.update(self._snapshot_state())
        return snap

    def restore(self, snap):
        if self.noise != "philox":
            raise RuntimeError("restore() needs counter-based noise (noise='philox')")
        self.curr_sigma = snap["curr_sigma"]
        self.gen = snap["pop_gen"]                 # the population's rows are keyed with it, and it is bumped again
        self._restore_state(snap)
        return self._offsprings_at(snap["pop_sigma"])

    def _snapshot_state(self):
        snap = {key: getattr(self, attr).clone() for key, attr, _ in self._STATE}
        snap["t"] = self.t
        return snap

    def _restore_state(self, snap):
        self._set_state([snap[key].clone() for key, _, _ in self._STATE])
        self.t = snap["t"]
        self._spare = None

    def _offsprings_at(self, sigma):
        """this rank's rows of the population of (the state vectors, sigma, self.gen)"""
        raise NotImplementedError


class simple_genetic(_DeviceStrategy):
    _STATE = (("elite_models", "elite_models", "parents"),)
    _STRATEGY = "STRATEGY_SIMPLE_GENETIC"

    def __init__(self, init_sigma, sigma_decay, elite_num, offspring_num, noise="philox", seed=0):
        super().__init__(init_sigma, sigma_decay, offspring_num, noise, seed)
        self.elite_num = elite_num
        self.elite_models = None      # device float32[k, P], best first

    def _population_size(self):
        return self.elite_num * (self.offspring_num // self.elite_num)

    def _gen_offsprings(self, agent_ids, elite_models, elite_num, offspring_num, sigma):
        def build():
            per = offspring_num // elite_num
            idx = np.empty(elite_num * per, dtype=np.int32)
            for e in range(elite_num):
                idx[e * per] = -1 - e                 # the elite itself, verbatim
                idx[e * per + 1:(e + 1) * per] = e    # its children
            return idx
        return self._materialise(elite_models, self._const_map(("genetic", elite_num, offspring_num), build), sigma)

    def _offsprings_at(self, sigma):
        return self._gen_offsprings(self.agent_ids, self.elite_models, self.elite_num, self.offspring_num, sigma)

    def _gen_state_constants(self):
        return dict(elite_num=self.elite_num)

    def get_elite_model(self):
        return self._model_from(self.elite_models[0])

    def init_offspring(self, network, agent_ids):
        self._bind(network, agent_ids)
        self.elite_models = self.dev.zeros(self.elite_num, self.P)
        return self._offsprings_at(self.curr_sigma)

    def evaluate_async(self, rewards):
        """evaluate() without the read-back: best_reward comes as a PendingReward (result() waits for it)."""
        fit = self._fitness_tensor(rewards)
        rank, _ = self.dev.rank_center(fit, want_weights=False, best=self._ring.arm())
        best = self._ring.push()
        self.elite_models, _ = self._select_elites(rank, self.elite_num)
        pop = self._offsprings_at(self.curr_sigma)
        self.curr_sigma *= self.sigma_decay       # decays AFTER regeneration (offspring_strategies.py:117-124)
        return pop, best, self.curr_sigma

    def get_wandb_cfg(self):
        return dict(init_sigma=self.init_sigma, sigma_decay=self.sigma_decay, elite_num=self.elite_num,
                    offspring_num=self.offspring_num)


class simple_evolution(_DeviceStrategy):
    _STATE = (("mu", "mu_model", "parents"),)
    _STRATEGY = "STRATEGY_SIMPLE_EVOLUTION"

    def __init__(self, init_sigma, sigma_decay, elite_num, offspring_num, noise="philox", seed=0):
        super().__init__(init_sigma, sigma_decay, offspring_num, noise, seed)
        self.elite_num = elite_num
        self.mu_model = None          # device float32[P]
        self.elite0 = None            # device float32[P]  (elite_models[0])
        self._alias_state = None      # device int32[1]: population slots 0 and 1 are the same module object

    def _population_size(self):
        return self.offspring_num + 1

    def _parent_map(self, same):
        def build():
            idx = np.zeros(self.offspring_num + 1, dtype=np.int32)
            idx[0], idx[1] = -1, (-1 if same else -2)    # [mu, elite0, then N-1 children of mu]
            return idx
        return self._const_map(("evolution", self.offspring_num, same), build)

    def _gen_offsprings(self, agent_ids, elite_models, mu_model, sigma, offspring_num):
        # after evaluate() the elite IS the mean (the reference's in-place sum, offspring_strategies.py:234-248), and at
        # the start both are the zero network: one parent row then serves slots 0 and 1 -- no torch.stack (20 us of host
        # time and a copy kernel per generation, a tenth of a 96-offspring generation)
        same = elite_models is mu_model or elite_models.data_ptr() == mu_model.data_ptr()
        parents = mu_model.view(1, -1) if same else torch.stack([mu_model, elite_models]).contiguous()
        return self._materialise(parents, self._parent_map(same), sigma)

    def _offsprings_at(self, sigma):
        return self._gen_offsprings(self.agent_ids, self.elite0, self.mu_model, sigma, self.offspring_num)

    def _set_state(self, vectors):
        self.mu_model = self.elite0 = vectors[0]

    def _gen_state_constants(self):
        return dict(elite_num=self.elite_num, alias_state=self._alias_state)

    def _loop_parent_map(self):
        return self._parent_map(True)              # after any evaluate, and at the zero start, elite[0] IS mu

    def get_elite_model(self):
        return self._model_from(self.elite0)

    def init_offspring(self, network, agent_ids):
        self._bind(network, agent_ids)
        self.mu_model = self.dev.zeros(self.P)
        self.elite0 = self.dev.zeros(self.P)
        self._alias_state = torch.ones(1, dtype=torch.int32, device=self.dev.device)
        return self._offsprings_at(self.curr_sigma)

    def evaluate_async(self, rewards):
        """evaluate() without the read-back: best_reward comes as a PendingReward (result() waits for it)."""
        fit = self._fitness_tensor(rewards)
        rank, _ = self.dev.rank_center(fit, want_weights=False, best=self._ring.arm())
        best = self._ring.push()
        # the reference sums the elites IN PLACE into elite[0]; an elite that is the same object as elite[0]
        # (slots 0 and 1 while they alias) doubles the running sum instead of adding its own value: the flags and
        # the aliasing state are kept on the device by ses_elite_select (include/ses.h)
        rows, alias = self._select_elites(rank, self.elite_num, self._alias_state)
        self._set_state([self.dev.elite_mean(rows, alias)])      # elite[0] was overwritten with the mean (aliasing quirk)
        self.curr_sigma *= self.sigma_decay
        return self._offsprings_at(self.curr_sigma), best, self.curr_sigma

    def _snapshot_state(self):
        same = self.elite0 is self.mu_model or self.elite0.data_ptr() == self.mu_model.data_ptr()
        return dict(super()._snapshot_state(), elite0=None if same else self.elite0.clone(), alias=self._alias_state.clone())

    def _restore_state(self, snap):
        super()._restore_state(snap)
        if snap["elite0"] is not None:
            self.elite0 = snap["elite0"].clone()
        self._alias_state = snap["alias"].clone()

    def get_wandb_cfg(self):
        return dict(init_sigma=self.init_sigma, elite_num=self.elite_num, offspring_num=self.offspring_num)


class _AdamState:
    """Adam's moments and its update counter live in the optimizer object (self.optimizer, whose pi is mu_model); the state table
    of openai_es and pgpe reaches them under these names"""
    _m = property(lambda self: self.optimizer.m, lambda self, x: setattr(self.optimizer, "m", x))
    _v = property(lambda self: self.optimizer.v, lambda self, x: setattr(self.optimizer, "v", x))
    t = property(lambda self: self.optimizer.t, lambda self, t: setattr(self.optimizer, "t", t))

    def _set_state(self, vectors):
        super()._set_state(vectors)
        self.optimizer.pi = self.mu_model


class openai_es(_AdamState, _DeviceStrategy):
    _STATE = (("mu", "mu_model", "parents"), ("m", "_m", "adam_m"), ("v", "_v", "adam_v"))
    _STRATEGY = "STRATEGY_OPENAI_ES"

    def __init__(self, init_sigma, sigma_decay, learning_rate, offspring_num, noise="philox", seed=0, fused=True):
        super().__init__(init_sigma, sigma_decay, offspring_num, noise, seed)
        self.learning_rate = learning_rate
        self.mu_model = None
        self.optimizer = None
        self.fused = bool(fused)      # philox noise: the whole fitness loop through ses_openai_generation (four launches)
        self._sharded_key = self._sharded_ok = None      # _sharded_tail_comm: the layout and transports asked about, the answer

    def _population_size(self):
        return self.offspring_num

    def _gen_offsprings(self, agent_ids, mu_model, sigma, offspring_num):
        def build():
            idx = np.zeros(offspring_num, dtype=np.int32)
            idx[0] = -1                           # member 0 is the unperturbed mu (epsilon = 0)
            return idx
        return self._materialise(mu_model.view(1, -1), self._const_map(("openai", offspring_num), build), sigma)

    def _offsprings_at(self, sigma):
        return self._gen_offsprings(self.agent_ids, self.mu_model, sigma, self.offspring_num)

    def get_elite_model(self):
        return self._model_from(self.mu_model)

    def init_offspring(self, network, agent_ids):
        self._bind(network, agent_ids)
        self.mu_model = self.dev.zeros(self.P)
        self.optimizer = Adam(self.mu_model, self.learning_rate)
        return self._offsprings_at(self.curr_sigma)

    def evaluate_async(self, rewards):
        """evaluate() without the read-back: best_reward comes as a PendingReward (result() waits for it)."""
        if self.noise == "philox" and self.fused:
            return super().evaluate_async(rewards)
        fit = self._fitness_tensor(rewards)
        _, weights = self.dev.rank_center(fit, best=self._ring.arm())
        best = self._ring.push()
        a = self.optimizer.next_step_scale()
        opt = self.optimizer
        if self.noise == "philox":
            self.dev.es_update_philox(weights, self.seed, self._last["gen"], self.learning_rate, self.curr_sigma, a,
                                      self.mu_model, opt.m, opt.v, skip_row0=True)
        else:
            self.dev.es_update_stored(weights, self._last["eps_store"], self.learning_rate, self.curr_sigma, a,
                                      self.mu_model, opt.m, opt.v)
        self.curr_sigma *= self.sigma_decay
        return self._offsprings_at(self.curr_sigma), best, self.curr_sigma

    def _generation(self, fit, state_in, state_out, shard, best):
        """The same generation through ses_openai_generation: rank shaping, gradient, Adam and the next population
        in four launches; (mu, m, v) ping-pong between two buffer triples.  Bit-identical to the step-by-step path
        (tests/test_gpu_host_mirror.py::test_openai_fused_generation_equals_stepwise)."""
        a = self.optimizer.next_step_scale()
        sigma = self.curr_sigma
        self.curr_sigma *= self.sigma_decay
        comm = self._sharded_tail_comm(self.offspring_num, shard)
        return self.dev.openai_generation(fit, self.seed, self._last["gen"], self.learning_rate, sigma, a, state_in,
                                          state_out, self.curr_sigma, self.gen, shard.first, shard.n_local,
                                          best=best, comm=comm, per_rank=shard.per_rank, world=shard.world)

    def _sharded_tail_comm(self, n, shard):
        """The transport handle for ses_openai_generation_sharded, or None for the replicated tail: the shard form needs
        shards aligned to the gradient's 1024-row chunks and a library transport for the chunk partials (asked once per
        layout and transport state; the tuning knob "openai_sharded_tail" = 0 forces the replicated form, for A/B runs)."""
        owner = getattr(self.dev, "_comm_owner", None)
        if shard.world == 1 or owner is None:
            return None
        key = (n, shard.per_rank, shard.world, owner.comm_route())
        if self._sharded_key != key:
            self._sharded_key = key
            self._sharded_ok = self.dev.openai_sharded_ok(owner, n, shard.per_rank, shard.world)
        return owner if self._sharded_ok else None

    def get_wandb_cfg(self):
        return dict(init_sigma=self.init_sigma, sigma_decay=self.sigma_decay, learning_rate=self.learning_rate,
                    offspring_num=self.offspring_num)


class _DistributionStrategy(_DeviceStrategy):
    """What pgpe, ars, sep_cma_es and lm_ma_es share: a search distribution (mu first, then the class's other state vectors) and a
    population of offspring_num rows drawn from it with no unperturbed row, hence no parent map.  A subclass declares its state and
    gives the perturbation and the generation call."""

    _C_LOOP_ONE_GPU = True

    def __init__(self, init_sigma, sigma_decay, offspring_num, noise, seed):
        if noise != "philox":
            raise ValueError(f"{type(self).__name__} has no counterpart in the reference whose numpy stream it could mirror: "
                             "noise must be 'philox'")
        super().__init__(init_sigma, sigma_decay, offspring_num, noise, seed)
        self.mu_model = None

    # ---- constructor checks -------------------------------------------------------------------
    def _set_offspring_num(self, offspring_num, refusal, even=False):
        if int(offspring_num) != offspring_num or offspring_num < 4 or (even and offspring_num % 2):
            raise ValueError(f"{refusal}, got {offspring_num}")
        self.offspring_num = int(offspring_num)

    def _set_elite_num(self, elite_num):
        if elite_num is None:
            elite_num = self.offspring_num // 2
        if int(elite_num) != elite_num or not 1 <= elite_num <= self.offspring_num:
            raise ValueError(f"{type(self).__name__}: elite_num must lie in [1, offspring_num = {self.offspring_num}], got {elite_num}")
        self.elite_num = int(elite_num)

    @staticmethod
    def _limits(name, pair, what="value", finite=True):
        lo, hi = (float(x) for x in pair)
        if not (0.0 < lo <= 1.0 <= hi and (math.isfinite(hi) or not finite)):
            raise ValueError(f"{name} must bracket the initial {what} 1.0 with a positive lower limit")
        return lo, hi

    # ---- populations ----------------------------------------------------------------------------
    def _population_size(self):
        return self.offspring_num

    def _perturb(self, sigma, first_row, n_rows):
        raise NotImplementedError

    def _gen_offsprings(self, sigma):
        shard = self._shard(self.offspring_num)
        theta = self._perturb(sigma, shard.first, shard.n_local) if shard.n_local else self.dev.empty(0, self.P)
        return self._population(theta, shard, sigma, None)

    _offsprings_at = _gen_offsprings

    def get_elite_model(self):
        return self._model_from(self.mu_model)


class pgpe(_AdamState, _DistributionStrategy):
    """PGPE with symmetric sampling (Sehnke et al. 2010) on the rank shaping and Adam of openai_es (Salimans et al. 2017), with
    a step size per parameter; no counterpart in the reference.

    The population is offspring_num / 2 mirrored pairs mu +- (curr_sigma * scale) * z, no unperturbed row.  evaluate() moves mu
    along the pairs' weight differences (Adam, learning_rate) and scale[p] along the pairs' weight sums, by at most
    sigma_max_change per generation and inside scale_limits (include/ses.h: ses_pgpe_generation has the arithmetic).  curr_sigma
    stays the plain float the loop reports and decays like openai_es's; sigma_decay = 1 is textbook PGPE."""

    _STATE = (("mu", "mu_model", "parents"), ("m", "_m", "adam_m"), ("v", "_v", "adam_v"), ("scale", "_scale", "scale"))
    _STRATEGY = "STRATEGY_PGPE"

    def __init__(self, init_sigma, sigma_decay, learning_rate, offspring_num, sigma_learning_rate=0.2, sigma_max_change=0.2,
                 scale_limits=(0.01, 100.0), noise="philox", seed=0):
        super().__init__(init_sigma, sigma_decay, offspring_num, noise, seed)
        self._set_offspring_num(offspring_num, "pgpe samples in mirrored pairs: offspring_num must be even and >= 4", even=True)
        self.scale_limits = self._limits("scale_limits", scale_limits, what="scale", finite=False)
        if not 0.0 <= sigma_max_change < 1.0:
            raise ValueError("sigma_max_change must lie in [0, 1)")
        self.learning_rate = learning_rate
        self.sigma_learning_rate = float(sigma_learning_rate)
        self.sigma_max_change = float(sigma_max_change)
        self.optimizer = None
        self._scale = None

    @property
    def scale(self):
        """float32[P] on the device: the per-parameter factor of curr_sigma (all ones at the start)."""
        return self._scale

    def _gen_state_constants(self):
        return dict(sigma_learning_rate=self.sigma_learning_rate, sigma_max_change=self.sigma_max_change,
                    scale_lo=self.scale_limits[0], scale_hi=self.scale_limits[1])

    def _perturb(self, sigma, first_row, n_rows):
        return self.dev.perturb_mirrored(self.mu_model, self._scale, sigma, self.seed, self.gen, first_row, n_rows)

    def init_offspring(self, network, agent_ids):
        self._bind(network, agent_ids)
        self.mu_model = self.dev.zeros(self.P)
        self._scale = torch.ones(self.P, dtype=torch.float32, device=self.dev.device)
        self.optimizer = Adam(self.mu_model, self.learning_rate)
        self._spare = None
        return self._offsprings_at(self.curr_sigma)

    def _generation(self, fit, state_in, state_out, shard, best):
        a = self.optimizer.next_step_scale()
        sigma = self.curr_sigma
        self.curr_sigma *= self.sigma_decay
        return self.dev.pgpe_generation(fit, self.seed, self._last["gen"], sigma, a, self.sigma_learning_rate, self.sigma_max_change,
                                        self.scale_limits, state_in, state_out, self.curr_sigma, self.gen, shard.first,
                                        shard.n_local, best=best)

    def get_wandb_cfg(self):
        return dict(init_sigma=self.init_sigma, sigma_decay=self.sigma_decay, learning_rate=self.learning_rate,
                    offspring_num=self.offspring_num, sigma_learning_rate=self.sigma_learning_rate,
                    sigma_max_change=self.sigma_max_change, scale_limits=list(self.scale_limits))


class ars(_DistributionStrategy):
    """Augmented Random Search (Mania, Guy & Recht 2018), the V1-t form: mirrored directions, the best elite_num of them by
    max(return+, return-), raw return differences, the step divided by the standard deviation of the returns kept, a plain step
    (no Adam, no rank shaping); no counterpart in the reference.

    The population is offspring_num / 2 mirrored pairs mu +- curr_sigma * z, no unperturbed row.  evaluate() moves mu by
    learning_rate / (elite_num * sigma_R) * sum_k (f+_k - f-_k) z_k over the elite_num best pairs (include/ses.h:
    ses_ars_generation has the arithmetic); with every kept return equal (sigma_R = 0) mu stays.  curr_sigma is the plain float
    the loop reports and decays like openai_es's; sigma_decay = 1 is textbook ARS.  The observation normaliser of ARS V2 is the
    network's: network.obs_normalizer (networks/neural_network.py; conf/reacher_ars_v2.yaml), which works with every strategy."""

    _STATE = (("mu", "mu_model", "parents"),)
    _STRATEGY = "STRATEGY_ARS"

    def __init__(self, init_sigma, sigma_decay, learning_rate, offspring_num, elite_num=None, noise="philox", seed=0):
        super().__init__(init_sigma, sigma_decay, offspring_num, noise, seed)
        self._set_offspring_num(offspring_num, "ars samples in mirrored pairs: offspring_num must be even and >= 4", even=True)
        pairs = self.offspring_num // 2
        if elite_num is None:
            elite_num = max(1, self.offspring_num // 4)
        if isinstance(elite_num, bool) or int(elite_num) != elite_num or not 1 <= elite_num <= pairs:
            raise ValueError(f"ars: elite_num (the directions used) must be an integer in [1, offspring_num / 2 = {pairs}], got {elite_num}")
        self.elite_num = int(elite_num)
        self.learning_rate = learning_rate
        self._ones = None

    def _gen_state_constants(self):
        return dict(ars_b=self.elite_num)

    def _perturb(self, sigma, first_row, n_rows):
        # ses_perturb_mirrored with scale = 1 is this strategy's population bit for bit
        return self.dev.perturb_mirrored(self.mu_model, self._ones, sigma, self.seed, self.gen, first_row, n_rows)

    def init_offspring(self, network, agent_ids):
        self._bind(network, agent_ids)
        self.mu_model = self.dev.zeros(self.P)
        self._ones = torch.ones(self.P, dtype=torch.float32, device=self.dev.device)
        self._spare = None
        return self._offsprings_at(self.curr_sigma)

    def _generation(self, fit, state_in, state_out, shard, best):
        sigma = self.curr_sigma
        self.curr_sigma *= self.sigma_decay
        return self.dev.ars_generation(fit, self.elite_num, self.seed, self._last["gen"], sigma, self.learning_rate, state_in,
                                       state_out, self.curr_sigma, self.gen, shard.first, shard.n_local, best=best)

    def get_wandb_cfg(self):
        return dict(init_sigma=self.init_sigma, sigma_decay=self.sigma_decay, learning_rate=self.learning_rate,
                    offspring_num=self.offspring_num, elite_num=self.elite_num)


def sep_cma_constants(n, P, mu):
    """The constants of sep_cma_es from (population n, parameters P, selected rows mu), in double (include/ses.h:
    ses_sepcma_params), and the normalised weights w_k ~ ln(mu + 0.5) - ln(k + 1), k < mu, as the float32 table the kernel reads."""
    w = math.log(mu + 0.5) - np.log(np.arange(1, mu + 1, dtype=np.float64))
    w = w / w.sum()
    mueff = 1.0 / float((w * w).sum())
    c_sigma = (mueff + 2.0) / (P + mueff + 5.0)
    d_sigma = 1.0 + 2.0 * max(0.0, math.sqrt((mueff - 1.0) / (P + 1.0)) - 1.0) + c_sigma
    c_c = (4.0 + mueff / P) / (P + 4.0 + 2.0 * mueff / P)
    c_1 = min(1.0, (P + 2.0) / 3.0 * 2.0 / ((P + 1.3) ** 2 + mueff))
    c_mu = min(1.0 - c_1, (P + 2.0) / 3.0 * 2.0 * (mueff - 2.0 + 1.0 / mueff) / ((P + 2.0) ** 2 + mueff))
    chi = math.sqrt(P) * (1.0 - 1.0 / (4.0 * P) + 1.0 / (21.0 * P * P))
    return dict(mu=int(mu), mueff=mueff, c_sigma=c_sigma, d_sigma=d_sigma, c_c=c_c, c_1=c_1, c_mu=c_mu, chi=chi), w.astype(np.float32)


class sep_cma_es(_DistributionStrategy):
    """sep-CMA-ES (Ros & Hansen 2008): CMA-ES with a diagonal covariance and cumulative step-size adaptation; no counterpart in
    the reference.

    The population is offspring_num rows mu + (curr_sigma * step * sqrt(C)) * z, no unperturbed row.  evaluate() moves mu along
    the weighted mean of the elite_num best rows' normals, adapts the variances C[p] from the evolution path p_c and the weighted
    squares, and the scalar step from the length of the path p_sigma -- all on the device, the step included (include/ses.h:
    ses_sepcma_generation has the arithmetic).  curr_sigma stays the plain float the loop reports and decays like openai_es's;
    sigma_decay = 1 is textbook CMA-ES."""

    _STATE = (("mu", "mu_model", "parents"), ("C", "_C", "cma_C"), ("p_sigma", "_ps", "cma_ps"), ("p_c", "_pc", "cma_pc"),
              ("step", "_step", "cma_step"))
    _STRATEGY = "STRATEGY_SEP_CMA_ES"

    def __init__(self, init_sigma, sigma_decay, offspring_num, elite_num=None, scale_limits=(0.01, 100.0), step_limits=(1e-6, 1e6),
                 noise="philox", seed=0):
        super().__init__(init_sigma, sigma_decay, offspring_num, noise, seed)
        self._set_offspring_num(offspring_num, "sep_cma_es: offspring_num must be an integer >= 4")
        self._set_elite_num(elite_num)
        self.scale_limits = self._limits("scale_limits", scale_limits)
        self.step_limits = self._limits("step_limits", step_limits)
        self.t = 0                     # updates done
        self.constants = None
        self._params = None
        self._weights = None
        self._C = self._ps = self._pc = self._step = None

    @property
    def variance(self):
        """float32[P] on the device: C, the per-parameter variances (all ones at the start)."""
        return self._C

    @property
    def step(self):
        """float32[1] on the device: the adapted factor of curr_sigma (1.0 at the start)."""
        return self._step

    def _gen_state_constants(self):
        return dict(cma_weights=self._weights, cma=self._params)

    def _perturb(self, sigma, first_row, n_rows):
        return self.dev.perturb_sepcma(self.mu_model, self._C, self._step, sigma, self.seed, self.gen, first_row, n_rows)

    def init_offspring(self, network, agent_ids):
        from ses import _lib
        self._bind(network, agent_ids)
        self.constants, w = sep_cma_constants(self.offspring_num, self.P, self.elite_num)
        c = self.constants
        self._params = _lib.SesSepcmaParams(c["mu"], 0, c["mueff"], c["c_sigma"], c["d_sigma"], c["c_c"], c["c_1"], c["c_mu"], c["chi"],
                                            self.scale_limits[0], self.scale_limits[1], self.step_limits[0], self.step_limits[1])
        self._weights = torch.from_numpy(w).to(self.dev.device)
        self.mu_model = self.dev.zeros(self.P)
        self._C = torch.ones(self.P, dtype=torch.float32, device=self.dev.device)
        self._ps, self._pc = self.dev.zeros(self.P), self.dev.zeros(self.P)
        self._step = torch.ones(1, dtype=torch.float32, device=self.dev.device)
        self.t = 0
        self._spare = None
        return self._offsprings_at(self.curr_sigma)

    def hsig_scale(self, t):
        """1 / sqrt(1 - (1 - c_sigma)^(2 t)) of update t (from 1): what ses_run_generations forms per generation"""
        return 1.0 / math.sqrt(1.0 - (1.0 - self.constants["c_sigma"]) ** (2.0 * float(t)))

    def _generation(self, fit, state_in, state_out, shard, best):
        t, sigma, next_sigma = self.t + 1, self.curr_sigma, self.curr_sigma * self.sigma_decay
        theta = self.dev.sepcma_generation(fit, self.seed, self._last["gen"], sigma, self.hsig_scale(t), self._params,
                                           self._weights, state_in, state_out, next_sigma, self.gen, shard.first,
                                           shard.n_local, best=best)
        self.t, self.curr_sigma = t, next_sigma        # the host scalars move only once the generation is enqueued
        return theta

    def get_wandb_cfg(self):
        return dict(init_sigma=self.init_sigma, sigma_decay=self.sigma_decay, offspring_num=self.offspring_num,
                    elite_num=self.elite_num, scale_limits=list(self.scale_limits), step_limits=list(self.step_limits))


def lm_ma_constants(n, P, mu, m=None):
    """The constants of lm_ma_es from (population n, parameters P, selected rows mu, direction vectors m), in double (include/ses.h:
    ses_lmma_params): mu, mueff, c_sigma, d_sigma, chi and the float32 weight table are sep_cma_es's; m defaults to
    min(32, 4 + floor(3 ln P)); c_d[j] = 1 / (1.5^j P) and c_c[j] = min(1, n / (4^j P)) for j < m."""
    c, w = sep_cma_constants(n, P, mu)
    m = min(32, 4 + int(math.floor(3.0 * math.log(P)))) if m is None else int(m)
    c_d = [1.0 / (1.5 ** j * P) for j in range(m)]
    c_c = [min(1.0, n / (4.0 ** j * P)) for j in range(m)]
    return dict(mu=c["mu"], m=m, mueff=c["mueff"], c_sigma=c["c_sigma"], d_sigma=c["d_sigma"], chi=c["chi"], c_d=c_d, c_c=c_c), w


def lm_ma_params(c, step_limits):
    """the _lib.SesLmmaParams of lm_ma_constants' dict: the doubles as they are, the four tables cast to float32 once"""
    from ses import _lib
    p = _lib.SesLmmaParams()
    p.mu, p.m = c["mu"], c["m"]
    p.mueff, p.c_sigma, p.d_sigma, p.chi = c["mueff"], c["c_sigma"], c["d_sigma"], c["chi"]
    p.step_lo, p.step_hi = step_limits
    for j in range(c["m"]):
        p.cd[j], p.ad[j] = c["c_d"][j], 1.0 - c["c_d"][j]
        p.ac[j], p.bc[j] = 1.0 - c["c_c"][j], math.sqrt(c["mueff"] * c["c_c"][j] * (2.0 - c["c_c"][j]))
    return p


class lm_ma_es(_DistributionStrategy):
    """LM-MA-ES (Loshchilov, Glasmachers & Beyer 2019): matrix adaptation ES whose transformation matrix is kept as `memory`
    direction vectors, with cumulative step-size adaptation; no counterpart in the reference.

    The population is offspring_num rows mu + (curr_sigma * step) * v, no unperturbed row; v is the row's normal vector passed
    through one rank-one transform (1 - c_d[j]) I + c_d[j] M_j M_j^T per direction vector learnt so far (min(t, memory) of them
    after t updates).  evaluate() moves mu along the transformed weighted mean of the elite_num best rows' normals, pulls every
    M_j towards that mean at its own rate c_c[j], and adapts the scalar step from the length of the path p_sigma -- all on the
    device (include/ses.h: ses_lmma_generation has the arithmetic).  memory = 0 is isotropic ES with cumulative step-size
    adaptation.  curr_sigma stays the plain float the loop reports and decays like openai_es's; sigma_decay = 1 is the paper's."""

    _STATE = (("mu", "mu_model", "parents"), ("p_sigma", "_ps", "lm_ps"), ("M", "_M", "lm_M"), ("step", "_step", "lm_step"))
    _STRATEGY = "STRATEGY_LM_MA_ES"

    def __init__(self, init_sigma, sigma_decay, offspring_num, elite_num=None, memory=None, step_limits=(1e-6, 1e6), noise="philox",
                 seed=0):
        super().__init__(init_sigma, sigma_decay, offspring_num, noise, seed)
        self._set_offspring_num(offspring_num, "lm_ma_es: offspring_num must be an integer >= 4")
        self._set_elite_num(elite_num)
        if memory is not None and (int(memory) != memory or not 0 <= memory <= 32):
            raise ValueError(f"lm_ma_es: memory must be an integer in [0, 32], got {memory}")
        self.memory = None if memory is None else int(memory)      # None: the default for P, fixed in init_offspring
        self.step_limits = self._limits("step_limits", step_limits)
        self.t = 0                     # updates done
        self.constants = None
        self._params = None
        self._weights = None
        self._ps = self._M = self._step = None

    @property
    def directions(self):
        """float32[memory, P] on the device: the direction vectors M_j (zeros at the start)."""
        return self._M

    @property
    def step(self):
        """float32[1] on the device: the adapted factor of curr_sigma (1.0 at the start)."""
        return self._step

    def m_active(self, t):
        """the direction vectors a population drawn after t updates uses"""
        return min(int(t), self.memory)

    def _gen_state_constants(self):
        return dict(lm_weights=self._weights, lm=self._params)

    def _perturb(self, sigma, first_row, n_rows):
        return self.dev.perturb_lmma(self.mu_model, self._M, self._step, self._params, self.m_active(self.t), sigma, self.seed,
                                     self.gen, first_row, n_rows)

    def init_offspring(self, network, agent_ids):
        self._bind(network, agent_ids)
        self.constants, w = lm_ma_constants(self.offspring_num, self.P, self.elite_num, self.memory)
        self.memory = self.constants["m"]
        self._params = lm_ma_params(self.constants, self.step_limits)
        self._weights = torch.from_numpy(w).to(self.dev.device)
        self.mu_model = self.dev.zeros(self.P)
        self._ps = self.dev.zeros(self.P)
        self._M = self.dev.zeros(self.memory, self.P)
        self._step = torch.ones(1, dtype=torch.float32, device=self.dev.device)
        self.t = 0
        self._spare = None
        return self._offsprings_at(self.curr_sigma)

    def _generation(self, fit, state_in, state_out, shard, best):
        t, sigma, next_sigma = self.t + 1, self.curr_sigma, self.curr_sigma * self.sigma_decay
        theta = self.dev.lmma_generation(fit, self.seed, self._last["gen"], sigma, self._params, self._weights,
                                         self.m_active(self.t), self.m_active(t), state_in, state_out, next_sigma, self.gen,
                                         shard.first, shard.n_local, best=best)
        self.t, self.curr_sigma = t, next_sigma        # the host scalars move only once the generation is enqueued
        return theta

    def get_wandb_cfg(self):
        return dict(init_sigma=self.init_sigma, sigma_decay=self.sigma_decay, offspring_num=self.offspring_num,
                    elite_num=self.elite_num, memory=self.memory, step_limits=list(self.step_limits))


def ma_es_constants(n, P, mu):
    """The constants of ma_es from (population n, parameters P, selected rows mu), in double (include/ses.h: ses_maes_params): mu,
    mueff, c_sigma, d_sigma, chi and the float32 weight table are sep_cma_es's; c_1 and c_mu are the full-matrix rates (without
    sep_cma_es's (P + 2) / 3 factor)."""
    c, w = sep_cma_constants(n, P, mu)
    mueff = c["mueff"]
    c_1 = 2.0 / ((P + 1.3) ** 2 + mueff)
    c_mu = min(1.0 - c_1, 2.0 * (mueff - 2.0 + 1.0 / mueff) / ((P + 2.0) ** 2 + mueff))
    return dict(mu=c["mu"], mueff=mueff, c_sigma=c["c_sigma"], d_sigma=c["d_sigma"], chi=c["chi"], c_1=c_1, c_mu=c_mu), w


def ma_es_params(c, step_limits):
    """the _lib.SesMaesParams of ma_es_constants' dict: the doubles as they are, the three factors of the update cast to float32 once"""
    from ses import _lib
    p = _lib.SesMaesParams()
    p.mu = c["mu"]
    p.mueff, p.c_sigma, p.d_sigma, p.chi, p.c_1, p.c_mu = c["mueff"], c["c_sigma"], c["d_sigma"], c["chi"], c["c_1"], c["c_mu"]
    p.a_m, p.c1h, p.cmuh = 1.0 - c["c_1"] / 2.0 - c["c_mu"] / 2.0, c["c_1"] / 2.0, c["c_mu"] / 2.0
    p.step_lo, p.step_hi = step_limits
    return p


class ma_es(_DistributionStrategy):
    """MA-ES (Beyer & Sendhoff 2017): matrix adaptation ES with the full P x P transformation matrix M and cumulative step-size
    adaptation; no counterpart in the reference.  For policies of up to MAX_P = 1024 parameters (M is 4 MB there); lm_ma_es is the
    strategy for larger ones.

    The population is offspring_num rows mu + (curr_sigma * step) * M z, no unperturbed row: one GEMM D = Z M^T.  evaluate() moves
    mu along the weighted mean of the elite_num best rows' D, multiplies M by (a I + c_1 / 2 p p^T + c_mu / 2 sum w z z^T) -- one
    more GEMM over the selected rows, since M z is the D the population was drawn with -- and adapts the scalar step from the length
    of the path p_sigma, all on the device (include/ses.h: ses_maes_generation has the arithmetic).  curr_sigma stays the plain float
    the loop reports and decays like openai_es's; sigma_decay = 1 is the paper's."""

    MAX_P = 1024                       # SES_MAES_MAX_P
    # D: this rank's rows of the current population's transformed normals; on one GPU that is all of them and the update reads
    # them, a sharded run's replicated tail recomputes the rows it never drew
    _STATE = (("mu", "mu_model", "parents"), ("p_sigma", "_ps", "ma_ps"), ("M", "_M", "ma_M"), ("step", "_step", "ma_step"),
              ("D", "_D", "ma_D"))
    _STRATEGY = "STRATEGY_MA_ES"

    def __init__(self, init_sigma, sigma_decay, offspring_num, elite_num=None, step_limits=(1e-6, 1e6), noise="philox", seed=0):
        super().__init__(init_sigma, sigma_decay, offspring_num, noise, seed)
        self._set_offspring_num(offspring_num, "ma_es: offspring_num must be an integer >= 4")
        self._set_elite_num(elite_num)
        self.step_limits = self._limits("step_limits", step_limits)
        self.t = 0                     # updates done
        self.constants = None
        self._params = None
        self._weights = None
        self._ps = self._M = self._step = self._D = None

    @property
    def matrix(self):
        """float32[P, P] on the device: the transformation matrix M (the identity at the start)."""
        return self._M

    @property
    def step(self):
        """float32[1] on the device: the adapted factor of curr_sigma (1.0 at the start)."""
        return self._step

    @classmethod
    def check_parameters(cls, P):
        if P > cls.MAX_P:
            raise ValueError(f"ma_es keeps a P x P matrix and serves policies of up to {cls.MAX_P} parameters, this one has {P}: "
                             "lm_ma_es is the strategy for larger policies")

    def _gen_state_constants(self):
        return dict(ma_weights=self._weights, ma=self._params)

    def _perturb(self, sigma, first_row, n_rows):
        return self.dev.perturb_maes(self.mu_model, self._M, self._step, sigma, self.seed, self.gen, first_row, n_rows,
                                     d_out=self._D)[0]

    def init_offspring(self, network, agent_ids):
        self._bind(network, agent_ids)
        self.check_parameters(self.P)
        self.constants, w = ma_es_constants(self.offspring_num, self.P, self.elite_num)
        self._params = ma_es_params(self.constants, self.step_limits)
        self._weights = torch.from_numpy(w).to(self.dev.device)
        self.mu_model = self.dev.zeros(self.P)
        self._ps = self.dev.zeros(self.P)
        self._M = torch.eye(self.P, dtype=torch.float32, device=self.dev.device)
        self._step = torch.ones(1, dtype=torch.float32, device=self.dev.device)
        self._D = self.dev.empty(self._shard(self.offspring_num).n_local, self.P)
        self.t = 0
        self._spare = None
        return self._offsprings_at(self.curr_sigma)

    def _generation(self, fit, state_in, state_out, shard, best):
        t, sigma, next_sigma = self.t + 1, self.curr_sigma, self.curr_sigma * self.sigma_decay
        d_in = state_in[4] if shard.world == 1 else None
        theta = self.dev.maes_generation(fit, self.seed, self._last["gen"], sigma, self._params, self._weights, state_in[:4],
                                         state_out[:4], d_in, next_sigma, self.gen, shard.first, shard.n_local,
                                         d_next_out=state_out[4], best=best)
        self.t, self.curr_sigma = t, next_sigma        # the host scalars move only once the generation is enqueued
        return theta

    def get_wandb_cfg(self):
        return dict(init_sigma=self.init_sigma, sigma_decay=self.sigma_decay, offspring_num=self.offspring_num,
                    elite_num=self.elite_num, step_limits=list(self.step_limits))
