"""HipES: shape/dtype-checked torch-tensor front end of the C ABI (include/ses.h).

PyTorch-ROCm tensors are only the parameter/fitness containers; every compute step is a
hand-written gfx950 kernel inside libses_hip.so, enqueued on torch's current HIP stream.
All checks happen on the host BEFORE a kernel is launched: a wrong shape raises here, it never
reaches the GPU.
"""
import contextlib
import ctypes
import os
import sys

import numpy as np
import torch

from . import _lib
from ._lib import HIDDEN, MODE_EPISODIC, SesConfig, SesError, check
from .envs import ENV_IDS, REGISTRY      # (ENV_IDS: name -> env id, None for a handle without an env)

# names that share an env id: the head selects the variant (gym's two landers -- one world step, two action spaces)
LANDER_DISCRETE = {name: e.discrete for name, e in REGISTRY.items()
                   if any(o.env_id == e.env_id and o.discrete != e.discrete for o in REGISTRY.values())}
_ACTION_DTYPE = {_lib.ACTION_I32_N: torch.int32, _lib.ACTION_I32_N_AGENTS: torch.int32,
                 _lib.ACTION_F32_N_A: torch.float32, _lib.ACTION_F32_N_AGENTS_A: torch.float32}


def param_count(num_state, num_action, gru):
    return _lib.load().ses_param_count(int(num_state), int(num_action), int(bool(gru)))


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@contextlib.contextmanager
def _stdout_to_stderr():
    """fd-level redirect of stdout to stderr around a native call that prints (RCCL's banner): programs that emit
    machine-readable lines on stdout (bench.py, run_es.py --log pipelines) stay clean."""
    sys.stdout.flush()
    saved = os.dup(1)
    try:
        os.dup2(2, 1)
        yield
    finally:
        sys.stdout.flush()
        os.dup2(saved, 1)
        os.close(saved)


def exclusive_stream(device=None):
    """A torch stream with a hardware queue of its own (ses_stream_create_exclusive): for HipES handles that share a device and
    exchange over the peer-store transport from ONE process -- their kernels wait for each other, so two of them must never sit
    behind one another on one queue.  The stream lives as long as the process (rigs create a handful)."""
    if not torch.cuda.is_available():
        raise SesError("no HIP device visible to torch")
    device = torch.cuda.current_device() if device is None else int(device)
    raw = ctypes.c_void_p()
    check(_lib.load().ses_stream_create_exclusive(device, ctypes.byref(raw)), "ses_stream_create_exclusive")
    return torch.cuda.ExternalStream(raw.value, device=torch.device("cuda", device))


def destroy_stream(stream):
    """Give back a stream of exclusive_stream() (ses_stream_destroy) once every handle built on it is closed.  A rig that
    ends with such streams alive is fine by itself, but under rocprofv3 the HIP runtime's exit-time teardown of live
    CU-masked streams runs after the profiler has finalised and the process ends in SIGSEGV (profiles/README.md, round 6)."""
    stream.synchronize()
    check(_lib.load().ses_stream_destroy(ctypes.c_void_p(stream.cuda_stream)), "ses_stream_destroy")


class BatchEliteLayout:
    """Where the trials of a simple_evolution / simple_genetic batch sit (ses_elite_generation_batch), built once per batch from
    (strategy, offspring_num, the trials' elite_num): the host arrays row0, n, elite_num, parent0 (int32[R]) and the totals the
    library validates its launches against.  A population has offspring_num + 1 rows under simple_evolution and
    elite_num * (offspring_num // elite_num) under simple_genetic; a trial keeps one parent row (its mu) or elite_num (its elites)."""

    def __init__(self, strategy, offspring_num, elite_nums):
        if strategy not in (_lib.STRATEGY_SIMPLE_EVOLUTION, _lib.STRATEGY_SIMPLE_GENETIC):
            raise SesError(f"BatchEliteLayout: strategy {strategy!r}; it serves simple_evolution and simple_genetic")
        self.strategy = int(strategy)
        self.evolution = strategy == _lib.STRATEGY_SIMPLE_EVOLUTION
        self.offspring_num = N = int(offspring_num)
        ks = [int(k) for k in elite_nums]
        if not ks:
            raise SesError("BatchEliteLayout: there must be at least one trial")
        ns = []
        for r, k in enumerate(ks):
            if k < 1:
                raise SesError(f"BatchEliteLayout: trial {r} has elite_num = {k}; there must be at least 1")
            n = N + 1 if self.evolution else k * (N // k)
            if k > n:
                raise SesError(f"BatchEliteLayout: trial {r} has elite_num = {k} above its {n} rows (offspring_num = {N})")
            if not 2 <= n <= _lib.BATCH_ELITE_MAX_N:
                raise SesError(f"BatchEliteLayout: trial {r} has {n} rows; a batched trial takes 2 .. {_lib.BATCH_ELITE_MAX_N}")
            ns.append(n)
        self.R = len(ks)
        self.n = np.asarray(ns, dtype=np.int32)
        self.elite_num = np.asarray(ks, dtype=np.int32)
        self.row0 = (np.cumsum(self.n) - self.n).astype(np.int32)
        per_trial = np.ones(self.R, dtype=np.int32) if self.evolution else self.elite_num
        self.parent0 = (np.cumsum(per_trial) - per_trial).astype(np.int32)
        self.rows_total = int(self.n.sum())
        self.parents_total = int(per_trial.sum())
        self.n_max = int(self.n.max())
        self.k_max = int(self.elite_num.max())
        if self.rows_total > _lib.BATCH_MAX_ROWS:
            raise SesError(f"BatchEliteLayout: {self.rows_total} rows in all exceed {_lib.BATCH_MAX_ROWS}")

    def parent_map(self, r):
        """int32[n_r]: trial r's parent map relative to its first parent row, in ses_perturb's convention (-1 - e: parent e verbatim)"""
        return elite_parent_map(self.strategy, int(self.n[r]), int(self.elite_num[r]))


def elite_parent_map(strategy, n, elite_num):
    """The closed-form parent map of a population of n rows (include/ses.h, ses_elite_generation_batch): simple_evolution's
    [mu, mu, children of mu], simple_genetic's blocks of [elite e, its children]."""
    i = np.arange(n, dtype=np.int32)
    if strategy == _lib.STRATEGY_SIMPLE_EVOLUTION:
        return np.where(i < 2, -1, 0).astype(np.int32)
    per = n // elite_num
    e = i // per
    return np.where(i % per == 0, -1 - e, e).astype(np.int32)


class HipES:
    """One handle = one (env, network shape, device, stream).  Mirrors the constructor arguments of
    the reference's builder.build_env / build_network (builder.py:10-24)."""

    def __init__(self, env_name="CartPole-v1", num_state=4, num_action=2, discrete_action=True, gru=False,
                 pomdp=False, max_step=500, eval_ep_num=5, device=None, lanes_per_env=0, n_agents=1,
                 physics64=False, stream=None):
        # the two landers share an env id; the head selects the variant, so a name that contradicts it is refused here
        if env_name in LANDER_DISCRETE and bool(discrete_action) != LANDER_DISCRETE[env_name]:
            other = next(k for k in LANDER_DISCRETE if k != env_name)
            raise SesError(f"{env_name} takes discrete_action={LANDER_DISCRETE[env_name]} "
                           f"(discrete_action={bool(discrete_action)} is {other})")
        lib = _lib.load()
        if not torch.cuda.is_available():
            raise SesError("no HIP device visible to torch: the simple-es hot path needs an MI355X "
                           "(there is no CPU fallback)")
        if env_name not in ENV_IDS:
            raise SesError(f"env {env_name!r} has no device kernel (available: {sorted(k for k in ENV_IDS if k)})")
        device = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", device)
        self.S, self.A = int(num_state), int(num_action)
        self.discrete, self.gru, self.pomdp = bool(discrete_action), bool(gru), bool(pomdp)
        self.max_step, self.E = int(max_step), int(eval_ep_num)
        self.P = param_count(self.S, self.A, self.gru)
        self.env_id = ENV_IDS[env_name]
        self.n_agents = int(n_agents)
        # What the library's env table says about this config's env (ses_env_info; it refuses a config the env does not run): the
        # width of one initial-state row and its reset distribution, the step-wise action.  A handle without an env has none; the
        # rows init_states_uniform draws on one stay CartPole's.
        if env_name is None:
            self.env_info, rows = None, _lib.env_info(REGISTRY["CartPole-v1"].env_id, 4, 2, True)
        else:
            self.env_info = rows = _lib.env_info(self.env_id, self.S, self.A, self.discrete, self.gru, self.pomdp, self.E,
                                                 self.n_agents, physics64)
        self.init_dim, self.init_range = rows.init_width, (rows.init_lo, rows.init_hi)
        cfg = SesConfig(self.env_id, self.S, self.A, int(self.discrete), int(self.gru), int(self.pomdp),
                        self.max_step, self.E, int(device), int(lanes_per_env), self.n_agents, int(bool(physics64)))
        self._lib = lib
        self._cfg = cfg
        self._h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            self.stream = torch.cuda.current_stream(self.device) if stream is None else stream   # the handle's launch stream
            check(lib.ses_create(ctypes.byref(cfg), ctypes.c_void_p(self.stream.cuda_stream), ctypes.byref(self._h)),
                  "ses_create")
        # test hook: SES_TUNING="gru_ep_parallel_max=0,gru_mfma_min_e=1" forces a kernel path for every handle of the
        # process (the library reads no environment itself; tests/test_gpu_gru.py reruns the parity suites this way)
        for item in filter(None, os.environ.get("SES_TUNING", "").split(",")):
            name, _, value = item.partition("=")
            self.set_tuning(name.strip(), int(value))

    def set_tuning(self, name, value):
        """ses_set_tuning: choose among the result-identical rollout kernels (include/ses.h lists the knobs)."""
        check(self._lib.ses_set_tuning(self._h, name.encode(), int(value)), "ses_set_tuning")

    def rollout_plan(self, n_rows, mode=_lib.MODE_EPISODIC, **knobs):
        """ses_rollout_plan for this handle's config: the launch form a rollout of n_rows offspring takes with the knobs at their
        DEFAULTS except those given (what set_tuning changed on the handle is passed again here)."""
        return _lib.rollout_plan(self._cfg, n_rows, mode, **knobs)

    def launch_counts(self):
        """ses_launch_counts: (pair-kernel rollouts, those that formed their own rows, k_es_apply_perturb launches) so far."""
        out = [ctypes.c_int64(0) for _ in range(3)]
        check(self._lib.ses_launch_counts(self._h, *[ctypes.byref(o) for o in out]), "ses_launch_counts")
        return tuple(int(o.value) for o in out)

    def set_stamp(self, dst):
        """ses_set_stamp: dst = pinned host (or device) int64[1] tensor that receives the GPU real-time counter at the end
        of this handle's next rollouts / perturbation launches; None switches the stamping off."""
        if dst is not None and not (isinstance(dst, torch.Tensor) and dst.dtype == torch.int64 and dst.numel() >= 1 and
                                    (dst.is_pinned() if dst.device.type == "cpu" else dst.device == self.device)):
            raise SesError("set_stamp: expected a pinned host or device int64 tensor")
        self._stamp_keepalive = dst
        check(self._lib.ses_set_stamp(self._h, _ptr(dst)), "ses_set_stamp")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.ses_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- argument validation ------------------------------------------------------------------
    def _chk(self, t, name, dtype, shape, optional=False):
        if t is None:
            if optional:
                return None
            raise SesError(f"{name}: tensor required")
        if not isinstance(t, torch.Tensor):
            raise SesError(f"{name}: expected a torch tensor, got {type(t).__name__}")
        if t.device != self.device:
            raise SesError(f"{name}: on {t.device}, handle is on {self.device}")
        if t.dtype != dtype:
            raise SesError(f"{name}: dtype {t.dtype}, expected {dtype}")
        if not t.is_contiguous():
            raise SesError(f"{name}: must be contiguous")
        if tuple(t.shape) != tuple(shape):
            raise SesError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
        return t

    def _chk_best(self, best):
        """float32[1] that receives max(fitness): a tensor on the handle's device, or PINNED host memory -- the kernel
        then stores the value straight into host-visible memory (no device-to-host copy queued between the kernels)."""
        if best is None:
            return None
        if isinstance(best, torch.Tensor) and best.device.type == "cpu":
            if not (best.is_pinned() and best.dtype == torch.float32 and best.numel() == 1 and best.is_contiguous()):
                raise SesError("best: a host tensor must be pinned float32[1]")
            return best
        return self._chk(best, "best", torch.float32, (1,))

    def _check_parent_idx(self, parent_idx, K):
        """-K <= parent_idx < K, or raise.  The check reads the tensor back (a device sync), so its result is cached --
        on the tensor OBJECT (held here, so its address cannot be recycled for another tensor) and its version."""
        last = getattr(self, "_idx_checked", None)
        if last is not None and last[0] is parent_idx and last[1] == parent_idx._version and last[2] == K:
            return
        lo, hi = int(parent_idx.min()), int(parent_idx.max())
        if hi >= K or lo < -K:
            raise SesError(f"parent_idx outside [-{K}, {K})")
        self._idx_checked = (parent_idx, parent_idx._version, K)

    def empty(self, *shape, dtype=torch.float32):
        return torch.empty(*shape, dtype=dtype, device=self.device)

    def zeros(self, *shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype, device=self.device)

    def alloc_env_soa(self, n, skew_bytes=4096):
        """SoA env-state arrays (x, xd, th, thd, action i32, ret, status i32) carved out of ONE allocation
        with a 4 KiB skew between consecutive arrays.  Seven separately allocated power-of-two-sized arrays
        start on the same HBM channel/bank phase and their 13 concurrent streams collide; the skew spreads
        them (measured on MI355X at 2^24 envs: 5.4 -> 5.97 TB/s for the env-step kernel)."""
        stride = (n * 4 + skew_bytes + 15) // 16 * 16
        pool = torch.zeros(stride * 7 // 4, dtype=torch.float32, device=self.device)
        views = [pool[k * stride // 4: k * stride // 4 + n] for k in range(7)]
        x, xd, th, thd, action, ret, status = views
        return x, xd, th, thd, action.view(torch.int32), ret, status.view(torch.int32)

    def sync(self):
        check(self._lib.ses_sync(self._h), "ses_sync")

    # -- multi-GPU: RCCL communicator owned by the handle (include/ses.h, ses_comm_*) -------------
    @staticmethod
    def comm_unique_id():
        """128 opaque bytes from ncclGetUniqueId; rank 0 creates them, every rank passes them to comm_init."""
        buf = ctypes.create_string_buffer(_lib.COMM_ID_BYTES)
        with _stdout_to_stderr():
            check(_lib.load().ses_comm_unique_id(buf), "ses_comm_unique_id")
        return buf.raw

    def comm_init(self, rank, world, unique_id):
        if len(unique_id) != _lib.COMM_ID_BYTES:
            raise SesError(f"comm_init: unique id must be {_lib.COMM_ID_BYTES} bytes")
        buf = ctypes.create_string_buffer(bytes(unique_id), _lib.COMM_ID_BYTES)
        with _stdout_to_stderr():          # RCCL prints a version banner on stdout when it initialises
            check(self._lib.ses_comm_init(self._h, int(rank), int(world), buf), "ses_comm_init")
        self._route = None

    def comm_info(self):
        """(rank, world, rccl_version_code); world == 0 means the handle has no communicator."""
        r, w, v = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        check(self._lib.ses_comm_info(self._h, ctypes.byref(r), ctypes.byref(w), ctypes.byref(v)), "ses_comm_info")
        return r.value, w.value, v.value

    def comm_destroy(self):
        check(self._lib.ses_comm_destroy(self._h), "ses_comm_destroy")
        self._route = None

    def comm_p2p_export(self, rank, world, max_per_rank):
        """ses_comm_p2p_export: allocate this rank's mailbox of the peer-store transport; returns the 64 handle bytes the
        peers need (gather them over the control plane and pass all of them, in rank order, to comm_p2p_attach)."""
        buf = ctypes.create_string_buffer(_lib.COMM_P2P_HANDLE_BYTES)
        check(self._lib.ses_comm_p2p_export(self._h, int(rank), int(world), int(max_per_rank), buf), "ses_comm_p2p_export")
        return buf.raw

    def comm_p2p_attach(self, handles):
        blob = b"".join(bytes(h) for h in handles)
        check(self._lib.ses_comm_p2p_attach(self._h, ctypes.create_string_buffer(blob, len(blob))), "ses_comm_p2p_attach")
        self._route = None

    def comm_p2p_attach_local(self, peers):
        """ses_comm_p2p_attach_local: `peers` = the HipES handles of all ranks of this process, in rank order (each has
        exported its mailbox and has a stream of its own)."""
        arr = (ctypes.c_void_p * len(peers))(*[p._h.value for p in peers])
        check(self._lib.ses_comm_p2p_attach_local(self._h, arr), "ses_comm_p2p_attach_local")
        self._route = None

    def comm_p2p_info(self):
        """(world, max_per_rank, exchanges); world == 0 means the peer-store transport is not attached."""
        w, m, x = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        check(self._lib.ses_comm_p2p_info(self._h, ctypes.byref(w), ctypes.byref(m), ctypes.byref(x)), "ses_comm_p2p_info")
        return w.value, m.value, x.value

    def comm_p2p_counts(self):
        """(exchanges with sequence words, granule exchanges) issued over the attached peer-store transport so far."""
        f, g = ctypes.c_int32(), ctypes.c_int32()
        check(self._lib.ses_comm_p2p_counts(self._h, ctypes.byref(f), ctypes.byref(g)), "ses_comm_p2p_counts")
        return f.value, g.value

    def comm_p2p_status(self):
        """Bit mask of the ranks some peer-store exchange of this handle gave up waiting for (0 = all good).  Reads a
        host-visible word: no stream operation, no synchronisation."""
        m = ctypes.c_uint32()
        check(self._lib.ses_comm_p2p_status(self._h, ctypes.byref(m)), "ses_comm_p2p_status")
        return m.value

    def comm_p2p_reset_status(self):
        """ses_comm_p2p_reset_status: clear the time-out mask (the ranks have agreed to keep using the transport)."""
        check(self._lib.ses_comm_p2p_reset_status(self._h), "ses_comm_p2p_reset_status")

    def comm_p2p_detach(self):
        check(self._lib.ses_comm_p2p_detach(self._h), "ses_comm_p2p_detach")
        self._route = None

    def comm_route(self):
        """(p2p world, p2p floats per rank, rccl world) -- what ses_allgather_fitness has to work with.  Cached: the three
        ctypes calls cost ~2 us per generation otherwise; attach / detach / comm_init / comm_destroy drop the cache."""
        r = getattr(self, "_route", None)
        if r is None:
            w, cap, _ = self.comm_p2p_info()
            r = self._route = (w, cap, self.comm_info()[1])
        return r

    def allgather_fitness(self, local, out=None):
        """local float32[n_per_rank] on every rank -> float32[world * n_per_rank], rank-major, identical everywhere.
        Peer stores when that transport is attached and the shard fits its mailbox, RCCL otherwise."""
        world, cap, rccl_world = self.comm_route()
        if world < 1 or local.shape[0] > cap:
            world = rccl_world                              # (with "comm_force_rccl" both transports span the same ranks)
        if world < 1:
            raise SesError("allgather_fitness: the handle has no communicator (comm_init or comm_p2p_attach first)")
        n = local.shape[0]
        self._chk(local, "local", torch.float32, (n,))
        out = self.empty(world * n) if out is None else self._chk(out, "all", torch.float32, (world * n,))
        check(self._lib.ses_allgather_fitness(self._h, _ptr(local), int(n), _ptr(out)), "ses_allgather_fitness")
        return out

    # -- K1 -----------------------------------------------------------------------------------
    def perturb(self, parents, sigma, seed, gen, first_row, n_rows, parent_idx=None, row_ids=None, out=None,
                idx_in_range=False):
        """idx_in_range: the caller built parent_idx on the host and checked -K <= idx < K there (skips the device
        read-back below)."""
        parents = parents.view(-1, self.P) if parents.dim() == 1 else parents
        K = parents.shape[0]
        self._chk(parents, "parents", torch.float32, (K, self.P))
        self._chk(parent_idx, "parent_idx", torch.int32, (n_rows,), optional=True)
        self._chk(row_ids, "row_ids", torch.int32, (n_rows,), optional=True)
        if parent_idx is not None and not idx_in_range:
            self._check_parent_idx(parent_idx, K)
        theta = self.empty(n_rows, self.P) if out is None else self._chk(out, "theta", torch.float32, (n_rows, self.P))
        check(self._lib.ses_perturb(self._h, _ptr(parents), _ptr(parent_idx), _ptr(row_ids), float(sigma), int(seed),
                                    int(gen), int(first_row), int(n_rows), _ptr(theta)), "ses_perturb")
        return theta

    def noise(self, seed, gen, first_row, n_rows):
        eps = self.empty(n_rows, self.P)
        check(self._lib.ses_noise(self._h, int(seed), int(gen), int(first_row), int(n_rows), _ptr(eps)), "ses_noise")
        return eps

    def perturb_host_noise(self, parents, eps64, sigma, parent_idx=None, want_eps_store=False):
        parents = parents.view(-1, self.P) if parents.dim() == 1 else parents
        K = parents.shape[0]
        n_rows = eps64.shape[0]
        self._chk(parents, "parents", torch.float32, (K, self.P))
        self._chk(eps64, "eps64", torch.float64, (n_rows, self.P))
        self._chk(parent_idx, "parent_idx", torch.int32, (n_rows,), optional=True)
        if parent_idx is not None:
            self._check_parent_idx(parent_idx, K)
        theta = self.empty(n_rows, self.P)
        store = self.empty(n_rows, self.P) if want_eps_store else None
        check(self._lib.ses_perturb_host_noise(self._h, _ptr(parents), _ptr(parent_idx), _ptr(eps64), float(sigma),
                                               int(n_rows), _ptr(theta), _ptr(store)), "ses_perturb_host_noise")
        return (theta, store) if want_eps_store else theta

    def init_states_uniform(self, seed, gen, first_row, n_rows, shared=False, lo=None, hi=None, out=None):
        lo = self.init_range[0] if lo is None else lo
        hi = self.init_range[1] if hi is None else hi
        out = (self.empty(n_rows, self.E, self.init_dim) if out is None else
               self._chk(out, "out", torch.float32, (n_rows, self.E, self.init_dim)))
        check(self._lib.ses_init_states_uniform(self._h, int(seed), int(gen), int(first_row), int(n_rows),
                                                int(bool(shared)), int(self.init_dim), float(lo), float(hi), _ptr(out)),
              "ses_init_states_uniform")
        return out

    def init_states_uniform_gens(self, seed, gen0, gens, first_row, n_rows, shared=False, out=None):
        """The resets of `gens` consecutive generations in one launch: float32[gens, n_rows, E, init_dim]."""
        lo, hi = self.init_range
        out = (self.empty(gens, n_rows, self.E, self.init_dim) if out is None else
               self._chk(out, "out", torch.float32, (gens, n_rows, self.E, self.init_dim)))
        check(self._lib.ses_init_states_uniform_gens(self._h, int(seed), int(gen0), int(gens), int(first_row), int(n_rows),
                                                     int(bool(shared)), int(self.init_dim), float(lo), float(hi), _ptr(out)),
              "ses_init_states_uniform_gens")
        return out

    # -- K2 / K3 ------------------------------------------------------------------------------
    def policy_forward(self, theta, obs, hidden=None):
        n = obs.shape[0]
        self._chk(theta, "theta", torch.float32, (n, self.P))
        self._chk(obs, "obs", torch.float32, (n, self.S))
        if self.gru:
            self._chk(hidden, "hidden", torch.float32, (n, HIDDEN))
        logits = self.empty(n, self.A)
        act = self.empty(n, self.A)
        action = self.empty(n, dtype=torch.int32)
        check(self._lib.ses_policy_forward(self._h, _ptr(theta), _ptr(obs), _ptr(hidden if self.gru else None), int(n),
                                           _ptr(logits), _ptr(act), _ptr(action)), "ses_policy_forward")
        return action, logits, act

    # -- the running observation normaliser (ses_obs_norm_*; float64 envs, MLP policies) -----------------
    def obs_norm_new(self):
        """Fresh normaliser state: (stats float64[S, 3] = 0, affine float32[2, S] = shift 0, scale 1)."""
        stats = self.zeros(self.S, 3, dtype=torch.float64)
        affine = self.zeros(2, self.S)
        affine[1].fill_(1.0)
        return stats, affine

    def obs_norm_bind(self, stats, affine, update=True):
        """ses_obs_norm_bind: every rollout of this handle normalises with `affine` from now on and, update on, accumulates the
        raw observations' statistics and merges them into (stats, affine).  The handle keeps the tensors alive."""
        self._chk(stats, "stats", torch.float64, (self.S, 3))
        self._chk(affine, "affine", torch.float32, (2, self.S))
        check(self._lib.ses_obs_norm_bind(self._h, _ptr(stats), _ptr(affine), int(bool(update))), "ses_obs_norm_bind")
        self._obs_norm_keepalive = (stats, affine)

    def obs_norm_unbind(self):
        check(self._lib.ses_obs_norm_bind(self._h, None, None, 0), "ses_obs_norm_bind")
        self._obs_norm_keepalive = None

    def obs_norm_merge(self, partials, stats, affine):
        """ses_obs_norm_merge: the reduction and merge alone on partials float64[2 S + 1, n_env] (step counts, sums, sums of
        squares); stats and affine are updated in place."""
        if not isinstance(partials, torch.Tensor) or partials.dim() != 2:
            raise SesError("partials: expected a float64[2 S + 1, n_env] tensor")
        n_env = partials.shape[1]
        if n_env < 1:
            raise SesError("partials: there must be at least one env")
        self._chk(partials, "partials", torch.float64, (2 * self.S + 1, n_env))
        self._chk(stats, "stats", torch.float64, (self.S, 3))
        self._chk(affine, "affine", torch.float32, (2, self.S))
        check(self._lib.ses_obs_norm_merge(self._h, _ptr(partials), int(n_env), _ptr(stats), _ptr(affine)), "ses_obs_norm_merge")

    def env_step(self, x, xd, th, thd, action, ret, status, mode=MODE_EPISODIC):
        n = x.shape[0]
        for name, t in (("x", x), ("xd", xd), ("th", th), ("thd", thd), ("ret", ret)):
            self._chk(t, name, torch.float32, (n,))
        self._chk(action, "action", torch.int32, (n,))
        self._chk(status, "status", torch.int32, (n,))   # bit pattern of the uint32 status word
        check(self._lib.ses_env_step(self._h, int(n), int(mode), _ptr(x), _ptr(xd), _ptr(th), _ptr(thd), _ptr(action),
                                     _ptr(ret), _ptr(status)), "ses_env_step")

    # -- k generations per call (ses_run_generations) ---------------------------------------------------
    def run_generations(self, state, k, best, stamps=None):
        """Enqueue k whole generations described by `state` (a _lib.SesGenState the caller keeps alive together with the
        tensors it points to).  best: pinned host (or device) float32[>= k]; stamps: pinned int64[>= k, 2] or None."""
        if not (isinstance(best, torch.Tensor) and best.dtype == torch.float32 and best.numel() >= k and best.is_contiguous()
                and (best.is_pinned() if best.device.type == "cpu" else best.device == self.device)):
            raise SesError("run_generations: best must be a pinned host or device float32 tensor of at least k elements")
        if stamps is not None and not (isinstance(stamps, torch.Tensor) and stamps.dtype == torch.int64 and stamps.numel() >= 2 * k
                                       and stamps.is_contiguous()
                                       and (stamps.is_pinned() if stamps.device.type == "cpu" else stamps.device == self.device)):
            raise SesError("run_generations: stamps must be a pinned host or device int64 tensor of at least 2 k elements")
        check(self._lib.ses_run_generations(self._h, ctypes.byref(state), int(k), _ptr(best), _ptr(stamps)), "ses_run_generations")

    # -- step-wise envs (ses_env_reset / ses_env_step_generic) --------------------------------------
    def env_state_bytes(self):
        b = self._lib.ses_env_state_bytes(self._h)
        if b <= 0:
            check(b, "ses_env_state_bytes")
        return b

    def env_obs_width(self):
        w = self._lib.ses_env_obs_width(self._h)
        if w <= 0:
            check(w, "ses_env_obs_width")
        return w

    def _env(self):
        if self.env_info is None:
            raise SesError("handle has no env")
        return self.env_info

    def action_shape(self, n):
        """shape of env_step_generic's action for n envs, by the env's action layout (ses_env_info)"""
        e = self._env()
        return {_lib.ACTION_I32_N: (n,), _lib.ACTION_I32_N_AGENTS: (n, e.agents), _lib.ACTION_F32_N_A: (n, e.num_action),
                _lib.ACTION_F32_N_AGENTS_A: (n, e.agents, e.num_action)}[e.action_layout]

    def env_reset(self, init):
        """init float32[n, init_dim] -> (state blob uint8[n, state_bytes], obs float32[n, obs_width])."""
        n = init.shape[0]
        self._chk(init, "init", torch.float32, (n, self.init_dim))
        state = torch.zeros(n, self.env_state_bytes(), dtype=torch.uint8, device=self.device)
        obs = self.empty(n, self.env_obs_width())
        check(self._lib.ses_env_reset(self._h, _ptr(init), int(n), _ptr(state), _ptr(obs)), "ses_env_reset")
        return state, obs

    def env_step_generic(self, state, action):
        """One transition of n envs: (obs float32[n, obs_width], reward float32[n], done int32[n]); the state blob is
        updated in place.  action: int32[n] (CartPole, Acrobot, MountainCar; LunarLander-v2: 0 .. 3, anything else is the no-op),
        int32[n, n_agents] (simple_spread; pursuit: int32[n, 8], a move 0 .. 4 each, anything else stays), float32[n, 5, 2] (waterworld: every pursuer's action already multiplied by 0.001),
        float32[n, A] (the continuous Box2D envs; Pendulum, MountainCarContinuous and the inverted-pendulum family float32[n, 1], Reacher float32[n, 2], the hopper float32[n, 3] = (thigh, leg, foot), Walker2D float32[n, 6] = the right leg's three, then the left leg's: any float, the env clips it -- their reward is the
        env's float64 reward rounded to float32)."""
        n = state.shape[0]
        self._chk(state, "state", torch.uint8, (n, self.env_state_bytes()))
        self._chk(action, "action", _ACTION_DTYPE[self._env().action_layout], self.action_shape(n))
        obs = self.empty(n, self.env_obs_width())
        reward = self.empty(n)
        done = self.empty(n, dtype=torch.int32)
        check(self._lib.ses_env_step_generic(self._h, _ptr(state), _ptr(action), int(n), _ptr(obs), _ptr(reward), _ptr(done)),
              "ses_env_step_generic")
        return obs, reward, done

    def env_step_shape(self):
        """ses_env_step_shape: (threads per workgroup, LDS bytes reserved per workgroup, waves per CU by the occupancy
        calculator, the device's LDS bytes per CU)."""
        b, l, w, c = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        check(self._lib.ses_env_step_shape(self._h, ctypes.byref(b), ctypes.byref(l), ctypes.byref(w), ctypes.byref(c)),
              "ses_env_step_shape")
        return b.value, l.value, w.value, c.value

    # -- rendering (ses_render_*) ----------------------------------------------
    def _render_check(self, rc, what):
        """an env without a scene is NotImplementedError (what the wrappers' render() raises), with the library's message"""
        if rc == _lib.SES_ERR_UNSUPPORTED:
            raise NotImplementedError(self._lib.ses_last_error().decode("utf-8", "replace"))
        check(rc, what)

    def render_size(self):
        """ses_render_size: (width, height) of the env's nominal canvas; NotImplementedError for an env without a scene."""
        w, h = ctypes.c_int32(), ctypes.c_int32()
        self._render_check(self._lib.ses_render_size(self._h, ctypes.byref(w), ctypes.byref(h)), "ses_render_size")
        return w.value, h.value

    def render_scene(self, state):
        """state blobs uint8[n, state_bytes] -> (prims int32[n, 256, 8], counts int32[n]): one launch, no synchronisation."""
        self.render_size()
        n = state.shape[0]
        self._chk(state, "state", torch.uint8, (n, self.env_state_bytes()))
        prims = self.empty(n, _lib.RENDER_MAX_PRIMS, 8, dtype=torch.int32)      # (slots from counts[i] on are not written)
        counts = self.empty(n, dtype=torch.int32)
        self._render_check(self._lib.ses_render_scene(self._h, _ptr(state), int(n), _ptr(prims), _ptr(counts)), "ses_render_scene")
        return prims, counts

    def render_frames(self, prims, counts, width, height):
        """prims int32[n, cap, 8], counts int32[n] -> palette-indexed frames uint8[n, height, width]: one launch for all n
        frames, no synchronisation; works on any handle (the rasteriser knows no env)."""
        if not isinstance(prims, torch.Tensor) or prims.dim() != 3:
            raise SesError("prims: expected an int32 tensor [n, cap, 8]")
        n, cap = int(prims.shape[0]), int(prims.shape[1])
        self._chk(prims, "prims", torch.int32, (n, cap, 8))
        self._chk(counts, "counts", torch.int32, (n,))
        width, height = int(width), int(height)
        if not (1 <= width <= 1024 and 1 <= height <= 1024 and 1 <= cap <= _lib.RENDER_MAX_PRIMS and n >= 1):
            raise SesError(f"render_frames: {n} frames of {width} x {height} from lists of {cap}: needs n >= 1, sides in 1..1024 "
                           f"and 1..{_lib.RENDER_MAX_PRIMS} primitives a list")
        frames = self.empty(n, height, width, dtype=torch.uint8)
        check(self._lib.ses_render_frames(self._h, _ptr(prims), _ptr(counts), n, cap, int(width), int(height), _ptr(frames)),
              "ses_render_frames")
        return frames

    def render(self, state):
        """state blobs -> uint8[n, H, W] palette indices at the env's nominal size (ses.render.to_rgb makes RGB of them): the scene
        launch and the raster launch, no synchronisation."""
        width, height = self.render_size()
        prims, counts = self.render_scene(state)
        return self.render_frames(prims, counts, width, height)

    def stream_probe(self, x, xd, th, thd, action, ret, status):
        """ses_stream_probe: the env-step kernel's 13 streams with no arithmetic (values unchanged) -- bench.py's ceiling."""
        n = x.shape[0]
        for name, t in (("x", x), ("xd", xd), ("th", th), ("thd", thd), ("ret", ret)):
            self._chk(t, name, torch.float32, (n,))
        self._chk(action, "action", torch.int32, (n,))
        self._chk(status, "status", torch.int32, (n,))
        check(self._lib.ses_stream_probe(self._h, int(n), _ptr(x), _ptr(xd), _ptr(th), _ptr(thd), _ptr(action), _ptr(ret),
                                         _ptr(status)), "ses_stream_probe")

    # -- fused rollout ------------------------------------------------------------------------
    def rollout(self, theta, init, mode=MODE_EPISODIC, want_episodes=False, fitness=None):
        n_rows = theta.shape[0]
        self._chk(theta, "theta", torch.float32, (n_rows, self.P))
        if init.dim() == 2:
            self._chk(init, "init", torch.float32, (self.E, self.init_dim))
            per = 0
        else:
            self._chk(init, "init", torch.float32, (n_rows, self.E, self.init_dim))
            per = 1
        fitness = self.empty(n_rows) if fitness is None else self._chk(fitness, "fitness", torch.float32, (n_rows,))
        ep_ret = self.empty(n_rows, self.E, dtype=torch.float64) if want_episodes else None
        ep_steps = self.empty(n_rows, self.E, dtype=torch.int32) if (want_episodes and self._env().has_ep_steps) else None
        check(self._lib.ses_rollout(self._h, _ptr(theta), _ptr(init), per, int(n_rows), int(mode), _ptr(fitness),
                                    _ptr(ep_ret), _ptr(ep_steps)), "ses_rollout")
        return (fitness, ep_ret, ep_steps) if want_episodes else fitness

    # -- K4 / K5 / K6 -------------------------------------------------------------------------
    def rank_center(self, fitness, want_weights=True, best=None):
        """rank int32[n], weights float64[n] (None when want_weights is False).  best: optional float32[1] device
        tensor that receives max(fitness) in the same launch."""
        n = fitness.shape[0]
        self._chk(fitness, "fitness", torch.float32, (n,))
        self._chk_best(best)
        rank = self.empty(n, dtype=torch.int32)
        weights = self.empty(n, dtype=torch.float64) if want_weights else None
        check(self._lib.ses_rank_center(self._h, _ptr(fitness), int(n), _ptr(rank), _ptr(weights), _ptr(best)),
              "ses_rank_center")
        return rank, weights

    def es_update_philox(self, weights, seed, gen, lr, sigma, adam_a, mu, m, v, skip_row0=True, want_grad=False):
        n = weights.shape[0]
        self._chk(weights, "weights", torch.float64, (n,))
        for name, t in (("mu", mu), ("m", m), ("v", v)):
            self._chk(t, name, torch.float32, (self.P,))
        grad = self.empty(self.P) if want_grad else None
        check(self._lib.ses_es_update_philox(self._h, _ptr(weights), int(n), int(bool(skip_row0)), int(seed), int(gen),
                                             float(lr), float(sigma), float(adam_a), _ptr(mu), _ptr(m), _ptr(v),
                                             _ptr(grad)), "ses_es_update_philox")
        return grad

    def openai_sharded_ok(self, comm, n, per_rank, world):
        """ses_openai_sharded_ok: can the openai_es tail of this layout run in its shard form over `comm`'s transport?"""
        rc = self._lib.ses_openai_sharded_ok(self._h, comm._h, int(n), int(per_rank), int(world))
        if rc < 0:
            check(rc, "ses_openai_sharded_ok")
        return rc == 1

    def openai_generation(self, fitness, seed, gen, lr, sigma, adam_a, state_in, state_out, next_sigma, next_gen,
                          first_row, n_rows, theta_next=None, best=None, comm=None, per_rank=0, world=1):
        """ses_openai_generation: rank shaping + ES gradient + Adam + the next population in four launches (five above 8192 rows).
        state_in / state_out: (mu, m, v) triples of distinct float32[P] tensors.  Returns theta_next[n_rows, P].
        comm (a HipES that owns a transport of `world` ranks) selects ses_openai_generation_sharded: this rank ranks and
        accumulates its own rows only, the chunk partials are all-gathered over comm (openai_sharded_ok says when)."""
        n = fitness.shape[0]
        self._chk(fitness, "fitness", torch.float32, (n,))
        for name, t in zip(("mu_in", "m_in", "v_in", "mu_out", "m_out", "v_out"), tuple(state_in) + tuple(state_out)):
            self._chk(t, name, torch.float32, (self.P,))
        if any(a.data_ptr() == b.data_ptr() for a, b in zip(state_in, state_out)):
            raise SesError("openai_generation: state_in and state_out must be distinct buffers")
        self._chk_best(best)
        if not (0 <= first_row and first_row + n_rows <= n):
            raise SesError(f"openai_generation: rows [{first_row}, +{n_rows}) outside the population of {n}")
        theta = (self.empty(n_rows, self.P) if theta_next is None else
                 self._chk(theta_next, "theta_next", torch.float32, (n_rows, self.P)))
        if comm is not None:
            check(self._lib.ses_openai_generation_sharded(
                self._h, comm._h, _ptr(fitness), int(n), int(seed), int(gen), float(lr), float(sigma), float(adam_a),
                *[_ptr(t) for t in state_in], *[_ptr(t) for t in state_out], float(next_sigma), int(next_gen), int(first_row),
                int(n_rows), int(per_rank), int(world), _ptr(theta), _ptr(best)), "ses_openai_generation_sharded")
            return theta
        check(self._lib.ses_openai_generation(self._h, _ptr(fitness), int(n), int(seed), int(gen), float(lr), float(sigma),
                                              float(adam_a), *[_ptr(t) for t in state_in], *[_ptr(t) for t in state_out],
                                              float(next_sigma), int(next_gen), int(first_row), int(n_rows),
                                              _ptr(theta) if n_rows else None, _ptr(best)), "ses_openai_generation")
        return theta

    def openai_generation_batch(self, fitness, n, trials, state_in, state_out, theta_next=None, best=None):
        """ses_openai_generation_batch: the openai_es tail of R trials of n rows each in three launches (four above 1024
        parameters), whatever R.  fitness: float32[R n], trial r's rows at [r n, (r + 1) n); trials: uint8[R, 40] on the device, the
        ses_batch_trial records (_lib.SesBatchTrial) the caller uploaded; state_in / state_out: (mu, m, v) triples of distinct
        float32[R, P] tensors; best: optional float32[R], on the device or pinned.  Returns theta_next[R n, P].  Every trial gets
        what openai_generation gives for its slice alone, bit for bit."""
        who = "openai_generation_batch"
        n = int(n)
        if not isinstance(trials, torch.Tensor) or trials.dim() != 2:
            raise SesError(f"{who}: trials must be a uint8[R, {ctypes.sizeof(_lib.SesBatchTrial)}] tensor")
        R = trials.shape[0]
        if R < 1:
            raise SesError(f"{who}: there must be at least one trial")
        if n < 2:
            raise SesError(f"{who}: {n} rows per trial; there must be at least 2")
        if n > _lib.BATCH_MAX_N:
            raise SesError(f"{who}: {n} rows per trial; the batch tail serves up to {_lib.BATCH_MAX_N}")
        if R * n > _lib.BATCH_MAX_ROWS:
            raise SesError(f"{who}: {R} trials x {n} rows exceed {_lib.BATCH_MAX_ROWS} rows in all")
        try:
            self._chk(trials, "trials", torch.uint8, (R, ctypes.sizeof(_lib.SesBatchTrial)))
            self._chk(fitness, "fitness", torch.float32, (R * n,))
            for name, t in zip(("mu_in", "m_in", "v_in", "mu_out", "m_out", "v_out"), tuple(state_in) + tuple(state_out)):
                self._chk(t, name, torch.float32, (R, self.P))
            if best is not None:
                if isinstance(best, torch.Tensor) and best.device.type == "cpu":
                    if not (best.is_pinned() and best.dtype == torch.float32 and tuple(best.shape) == (R,) and best.is_contiguous()):
                        raise SesError(f"best: a host tensor must be pinned float32[{R}]")
                else:
                    self._chk(best, "best", torch.float32, (R,))
            theta = (self.empty(R * n, self.P) if theta_next is None else
                     self._chk(theta_next, "theta_next", torch.float32, (R * n, self.P)))
        except SesError as e:
            raise SesError(f"{who}: {e}") from None
        if any(a.data_ptr() == b.data_ptr() for a, b in zip(state_in, state_out)):
            raise SesError(f"{who}: state_in and state_out must be distinct buffers")
        check(self._lib.ses_openai_generation_batch(self._h, _ptr(fitness), R, n, _ptr(trials), *[_ptr(t) for t in state_in],
                                                    *[_ptr(t) for t in state_out], _ptr(theta), _ptr(best)),
              "ses_openai_generation_batch")
        return theta

    def elite_generation_batch(self, fitness, layout, trials, parents_in, parents_out, alias_state=None, theta_next=None, best=None,
                               want_ids=False):
        """ses_elite_generation_batch: the simple_evolution / simple_genetic tail of the R ragged trials of `layout` (a
        BatchEliteLayout) in three launches, whatever R.  fitness: float32[rows_total]; trials: uint8[R, 48] on the device, the
        ses_batch_elite_trial records (_lib.SesBatchEliteTrial) the caller uploaded, in agreement with the layout; parents_in /
        parents_out: distinct float32[parents_total, P]; alias_state: int32[R], updated in place (evolution only); best: optional
        float32[R], on the device or pinned.  Returns theta_next[rows_total, P], and with want_ids also the elite ids
        (int32[parents_total] for genetic, int32[R, k_max] for evolution).  Every trial gets what the solo calls give for its
        slice alone, bit for bit."""
        who = "elite_generation_batch"
        if not isinstance(layout, BatchEliteLayout):
            raise SesError(f"{who}: layout must be a BatchEliteLayout")
        R, size = layout.R, ctypes.sizeof(_lib.SesBatchEliteTrial)
        if not isinstance(trials, torch.Tensor) or trials.dim() != 2:
            raise SesError(f"{who}: trials must be a uint8[R, {size}] tensor")
        try:
            self._chk(trials, "trials", torch.uint8, (R, size))
            self._chk(fitness, "fitness", torch.float32, (layout.rows_total,))
            self._chk(parents_in, "parents_in", torch.float32, (layout.parents_total, self.P))
            self._chk(parents_out, "parents_out", torch.float32, (layout.parents_total, self.P))
            if layout.evolution:
                self._chk(alias_state, "alias_state", torch.int32, (R,))
            elif alias_state is not None:
                raise SesError("alias_state is simple_evolution's; simple_genetic takes none")
            if best is not None:
                if isinstance(best, torch.Tensor) and best.device.type == "cpu":
                    if not (best.is_pinned() and best.dtype == torch.float32 and tuple(best.shape) == (R,) and best.is_contiguous()):
                        raise SesError(f"best: a host tensor must be pinned float32[{R}]")
                else:
                    self._chk(best, "best", torch.float32, (R,))
            theta = (self.empty(layout.rows_total, self.P) if theta_next is None else
                     self._chk(theta_next, "theta_next", torch.float32, (layout.rows_total, self.P)))
        except SesError as e:
            raise SesError(f"{who}: {e}") from None
        if parents_in.data_ptr() == parents_out.data_ptr():
            raise SesError(f"{who}: parents_in and parents_out must be distinct buffers")
        ids = None
        if want_ids:
            ids = (self.empty(R, layout.k_max, dtype=torch.int32) if layout.evolution else
                   self.empty(layout.parents_total, dtype=torch.int32))
        check(self._lib.ses_elite_generation_batch(self._h, layout.strategy, _ptr(fitness), R, _ptr(trials), layout.n_max, layout.k_max,
                                                   layout.rows_total, layout.parents_total, _ptr(parents_in), _ptr(parents_out),
                                                   _ptr(alias_state), _ptr(theta), _ptr(best), _ptr(ids)),
              "ses_elite_generation_batch")
        return (theta, ids) if want_ids else theta

    # -- what the wrappers of the distribution strategies share (pgpe, sep_cma_es, lm_ma_es) ------------
    def _chk_vectors(self, names, tensors, shapes):
        """float32 tensors against a (names, shapes) table; a shape of None is the caller's to check"""
        for name, t, shape in zip(names, tensors, shapes):
            if shape is not None:
                self._chk(t, name, torch.float32, shape)

    def _chk_state(self, who, names, shapes, state_in, state_out):
        """state_in / state_out: one tensor per name, of the table's shapes, no buffer on both sides (an empty tensor -- lm_ma_es
        with memory = 0 -- has no buffer to share)"""
        if len(state_in) != len(names) or len(state_out) != len(names):
            raise SesError(f"{who}: state_in / state_out are ({', '.join(names)})")
        for side, state in (("in", state_in), ("out", state_out)):
            self._chk_vectors([f"{name}_{side}" for name in names], state, shapes)
        if any(a.data_ptr() == b.data_ptr() and a.numel() for a, b in zip(state_in, state_out)):
            raise SesError(f"{who}: state_in and state_out must be distinct buffers")

    def _next_rows(self, who, n, first_row, n_rows, theta_next, best):
        """a generation's shard [first_row, first_row + n_rows) of the next population of n rows: theta_next[n_rows, P], allocated
        unless given"""
        self._chk_best(best)
        if not (0 <= first_row and 0 <= n_rows and first_row + n_rows <= n):
            raise SesError(f"{who}: rows [{first_row}, +{n_rows}) outside the population of {n}")
        return (self.empty(n_rows, self.P) if theta_next is None else
                self._chk(theta_next, "theta_next", torch.float32, (n_rows, self.P)))

    def _perturb_rows(self, who, first_row, n_rows, out):
        """a perturbation's rows [first_row, first_row + n_rows): theta[n_rows, P], allocated unless given"""
        if not (first_row >= 0 and n_rows >= 1):
            raise SesError(f"{who}: bad row range [{first_row}, +{n_rows})")
        return self.empty(n_rows, self.P) if out is None else self._chk(out, "theta", torch.float32, (n_rows, self.P))

    # -- pgpe (ses_perturb_mirrored / ses_pgpe_generation) ------------------------------------------
    def perturb_mirrored(self, mu, scale, sigma, seed, gen, first_row, n_rows, out=None):
        """Rows [first_row, first_row + n_rows) of the mirrored population mu +- (sigma * scale) * z: pair j = rows
        (2 j, 2 j + 1), z = the noise of row j.  Returns theta[n_rows, P]."""
        self._chk_vectors(("mu", "scale"), (mu, scale), ((self.P,),) * 2)
        theta = self._perturb_rows("perturb_mirrored", first_row, n_rows, out)
        check(self._lib.ses_perturb_mirrored(self._h, _ptr(mu), _ptr(scale), float(sigma), int(seed), int(gen), int(first_row),
                                             int(n_rows), _ptr(theta)), "ses_perturb_mirrored")
        return theta

    def pgpe_generation(self, fitness, seed, gen, sigma, adam_a, sigma_learning_rate, sigma_max_change, scale_limits, state_in,
                        state_out, next_sigma, next_gen, first_row, n_rows, theta_next=None, best=None, want_sums=False):
        """ses_pgpe_generation: rank shaping, pair gradient, Adam on mu + the clipped step of scale, and the next mirrored
        population.  state_in / state_out: (mu, m, v, scale) quadruples of distinct float32[P] tensors.  Returns theta_next
        [n_rows, P], or (theta_next, Gmu, Gs) with want_sums."""
        n = fitness.shape[0]
        self._chk(fitness, "fitness", torch.float32, (n,))
        if n < 4 or n % 2:
            raise SesError(f"pgpe_generation: the population must be even and >= 4, got {n}")
        self._chk_state("pgpe_generation", ("mu", "m", "v", "scale"), ((self.P,),) * 4, state_in, state_out)
        lo, hi = (float(x) for x in scale_limits)
        if not (0.0 < lo <= hi and 0.0 <= sigma_max_change < 1.0):
            raise SesError("pgpe_generation: need 0 < scale_lo <= scale_hi and 0 <= sigma_max_change < 1")
        theta = self._next_rows("pgpe_generation", n, first_row, n_rows, theta_next, best)
        gmu = self.empty(self.P) if want_sums else None
        gs = self.empty(self.P) if want_sums else None
        check(self._lib.ses_pgpe_generation(self._h, _ptr(fitness), int(n), int(seed), int(gen), float(sigma), float(adam_a),
                                            float(sigma_learning_rate), float(sigma_max_change), lo, hi,
                                            *[_ptr(t) for t in state_in], *[_ptr(t) for t in state_out], float(next_sigma),
                                            int(next_gen), int(first_row), int(n_rows), _ptr(theta) if n_rows else None,
                                            _ptr(best), _ptr(gmu), _ptr(gs)), "ses_pgpe_generation")
        return (theta, gmu, gs) if want_sums else theta

    # -- ars (ses_perturb_mirrored with scale = 1 / ses_ars_generation) -----------------------------
    def ars_generation(self, fitness, b, seed, gen, sigma, learning_rate, state_in, state_out, next_sigma, next_gen, first_row,
                       n_rows, theta_next=None, best=None, want_sums=False):
        """ses_ars_generation: pair scores, their rank, the gradient over the b best mirrored directions, the step divided by the
        standard deviation of the returns kept, and the next mirrored population.  state_in / state_out: (mu,) 1-tuples of
        distinct float32[P] tensors.  Returns theta_next[n_rows, P], or (theta_next, G, sigma_R) with want_sums (sigma_R:
        float64[1] on the device)."""
        n = fitness.shape[0]
        self._chk(fitness, "fitness", torch.float32, (n,))
        if n < 4 or n % 2:
            raise SesError(f"ars_generation: the population must be even and >= 4, got {n}")
        if int(b) != b or not 1 <= b <= n // 2:
            raise SesError(f"ars_generation: b must lie in [1, {n // 2}], got {b}")
        self._chk_state("ars_generation", ("mu",), ((self.P,),), state_in, state_out)
        theta = self._next_rows("ars_generation", n, first_row, n_rows, theta_next, best)
        g = self.empty(self.P) if want_sums else None
        sigma_r = self.empty(1, dtype=torch.float64) if want_sums else None
        check(self._lib.ses_ars_generation(self._h, _ptr(fitness), int(n), int(b), int(seed), int(gen), float(sigma),
                                           float(learning_rate), _ptr(state_in[0]), _ptr(state_out[0]), float(next_sigma),
                                           int(next_gen), int(first_row), int(n_rows), _ptr(theta) if n_rows else None,
                                           _ptr(best), _ptr(g), _ptr(sigma_r)), "ses_ars_generation")
        return (theta, g, sigma_r) if want_sums else theta

    def ars_generation_batch(self, fitness, n, bs, trials, state_in, state_out, theta_next=None, best=None, want_sums=False):
        """ses_ars_generation_batch: the ars tail of R trials of n rows each in four launches, whatever R (five where ars_generation
        takes five).  fitness: float32[R n], trial r's rows at [r n, (r + 1) n); bs: the trials' b_r (host integers, 1 .. n / 2);
        trials: uint8[R, 40] on the device, the ses_batch_ars_trial records (_lib.SesBatchArsTrial) the caller uploaded; state_in /
        state_out: (mu,) 1-tuples of distinct float32[R, P] tensors; best: optional float32[R], on the device or pinned.  Returns
        theta_next[R n, P], or (theta_next, G[R, P], sigma_R float64[R]) with want_sums.  Every trial gets what ars_generation gives
        for its slice alone, bit for bit."""
        who = "ars_generation_batch"
        n = int(n)
        tsize = ctypes.sizeof(_lib.SesBatchArsTrial)
        if not isinstance(trials, torch.Tensor) or trials.dim() != 2:
            raise SesError(f"{who}: trials must be a uint8[R, {tsize}] tensor")
        R = trials.shape[0]
        if R < 1:
            raise SesError(f"{who}: there must be at least one trial")
        if n < _lib.BATCH_ARS_MIN_N or n % 2:
            raise SesError(f"{who}: {n} rows per trial; the population must be even and >= {_lib.BATCH_ARS_MIN_N}")
        if n > _lib.BATCH_ARS_MAX_N:
            raise SesError(f"{who}: {n} rows per trial; the batch tail serves up to {_lib.BATCH_ARS_MAX_N}")
        if R * n > _lib.BATCH_MAX_ROWS:
            raise SesError(f"{who}: {R} trials x {n} rows exceed {_lib.BATCH_MAX_ROWS} rows in all")
        bs = [int(b) for b in bs]
        if len(bs) != R:
            raise SesError(f"{who}: {len(bs)} values of b for {R} trials")
        for r, b in enumerate(bs):
            if not 1 <= b <= n // 2:
                raise SesError(f"{who}: trial {r} has b = {b} outside [1, {n // 2}]")
        try:
            self._chk(trials, "trials", torch.uint8, (R, tsize))
            self._chk(fitness, "fitness", torch.float32, (R * n,))
            if best is not None:
                if isinstance(best, torch.Tensor) and best.device.type == "cpu":
                    if not (best.is_pinned() and best.dtype == torch.float32 and tuple(best.shape) == (R,) and best.is_contiguous()):
                        raise SesError(f"best: a host tensor must be pinned float32[{R}]")
                else:
                    self._chk(best, "best", torch.float32, (R,))
            theta = (self.empty(R * n, self.P) if theta_next is None else
                     self._chk(theta_next, "theta_next", torch.float32, (R * n, self.P)))
            self._chk_state(who, ("mu",), ((R, self.P),), state_in, state_out)
        except SesError as e:
            raise SesError(str(e) if str(e).startswith(who) else f"{who}: {e}") from None
        g = self.empty(R, self.P) if want_sums else None
        sigma_r = self.empty(R, dtype=torch.float64) if want_sums else None
        check(self._lib.ses_ars_generation_batch(self._h, _ptr(fitness), R, n, (ctypes.c_int32 * R)(*bs), _ptr(trials),
                                                 _ptr(state_in[0]), _ptr(state_out[0]), _ptr(theta), _ptr(best), _ptr(g),
                                                 _ptr(sigma_r)), "ses_ars_generation_batch")
        return (theta, g, sigma_r) if want_sums else theta

    # -- sep_cma_es (ses_perturb_sepcma / ses_sepcma_generation) ------------------------------------
    def perturb_sepcma(self, mu, C, step, sigma, seed, gen, first_row, n_rows, out=None):
        """Rows [first_row, first_row + n_rows) of the population mu + ((sigma * step) * sqrt(C)) * z, z = the noise of the row.
        step: float32[1] on the device.  Returns theta[n_rows, P]."""
        self._chk_vectors(("mu", "C", "step"), (mu, C, step), ((self.P,), (self.P,), (1,)))
        theta = self._perturb_rows("perturb_sepcma", first_row, n_rows, out)
        check(self._lib.ses_perturb_sepcma(self._h, _ptr(mu), _ptr(C), _ptr(step), float(sigma), int(seed), int(gen), int(first_row),
                                           int(n_rows), _ptr(theta)), "ses_perturb_sepcma")
        return theta

    def sepcma_generation(self, fitness, seed, gen, sigma, hsig_scale, params, weights, state_in, state_out, next_sigma, next_gen,
                          first_row, n_rows, theta_next=None, best=None, want_sums=False):
        """ses_sepcma_generation: rank, weighted sums over the params.mu best rows, the update of (mu, C, p_sigma, p_c, step) and
        the next population.  params: a _lib.SesSepcmaParams; weights: float32[params.mu] on the device; state_in / state_out:
        (mu, C, p_sigma, p_c, step) quintuples of distinct tensors (float32[P]; step float32[1]).  Returns theta_next[n_rows, P],
        or (theta_next, Sz, Szz, norm2) with want_sums (norm2: float64[1])."""
        n = fitness.shape[0]
        self._chk(fitness, "fitness", torch.float32, (n,))
        if n < 4:
            raise SesError(f"sepcma_generation: the population must have at least 4 rows, got {n}")
        if not isinstance(params, _lib.SesSepcmaParams):
            raise SesError("sepcma_generation: params must be a SesSepcmaParams")
        if not 1 <= params.mu <= n:
            raise SesError(f"sepcma_generation: mu = {params.mu} outside [1, {n}]")
        self._chk(weights, "weights", torch.float32, (params.mu,))
        self._chk_state("sepcma_generation", ("mu", "C", "p_sigma", "p_c", "step"), ((self.P,),) * 4 + ((1,),), state_in, state_out)
        if not (0.0 < params.scale_lo <= params.scale_hi and 0.0 < params.step_lo <= params.step_hi):
            raise SesError("sepcma_generation: need 0 < scale_lo <= scale_hi and 0 < step_lo <= step_hi")
        theta = self._next_rows("sepcma_generation", n, first_row, n_rows, theta_next, best)
        sz = self.empty(self.P) if want_sums else None
        szz = self.empty(self.P) if want_sums else None
        norm2 = self.empty(1, dtype=torch.float64) if want_sums else None
        check(self._lib.ses_sepcma_generation(self._h, _ptr(fitness), int(n), int(seed), int(gen), float(sigma), float(hsig_scale),
                                              ctypes.byref(params), _ptr(weights), *[_ptr(t) for t in state_in],
                                              *[_ptr(t) for t in state_out], float(next_sigma), int(next_gen), int(first_row),
                                              int(n_rows), _ptr(theta) if n_rows else None, _ptr(best), _ptr(sz), _ptr(szz),
                                              _ptr(norm2)), "ses_sepcma_generation")
        return (theta, sz, szz, norm2) if want_sums else theta

    def sepcma_generation_batch(self, fitness, n, mus, trials, consts, weights, state_in, state_out, theta_next=None, best=None):
        """ses_sepcma_generation_batch: the sep_cma_es tail of R trials of n rows each in four launches, whatever R.  fitness:
        float32[R n], trial r's rows at [r n, (r + 1) n); mus: the trials' mu_r (host integers, 1 .. n); trials: uint8[R, 40] on the
        device, the ses_batch_sepcma_trial records (_lib.SesBatchSepcmaTrial) the caller uploaded; consts: uint8[R, 80], the
        ses_batch_sepcma_consts blocks (_lib.SesBatchSepcmaConsts); weights: float32[R, n], row r = trial r's mu_r weights, then
        zeros; state_in / state_out: (mu, C, p_sigma, p_c, step) quintuples of distinct tensors (float32[R, P]; step float32[R]);
        best: optional float32[R], on the device or pinned.  Returns theta_next[R n, P].  Every trial gets what sepcma_generation
        gives for its slice alone, bit for bit."""
        who = "sepcma_generation_batch"
        n = int(n)
        tsize, csize = ctypes.sizeof(_lib.SesBatchSepcmaTrial), ctypes.sizeof(_lib.SesBatchSepcmaConsts)
        if not isinstance(trials, torch.Tensor) or trials.dim() != 2:
            raise SesError(f"{who}: trials must be a uint8[R, {tsize}] tensor")
        R = trials.shape[0]
        if R < 1:
            raise SesError(f"{who}: there must be at least one trial")
        if n < _lib.BATCH_SEPCMA_MIN_N:
            raise SesError(f"{who}: {n} rows per trial; there must be at least {_lib.BATCH_SEPCMA_MIN_N}")
        if n > _lib.BATCH_SEPCMA_MAX_N:
            raise SesError(f"{who}: {n} rows per trial; the batch tail serves up to {_lib.BATCH_SEPCMA_MAX_N}")
        if R * n > _lib.BATCH_MAX_ROWS:
            raise SesError(f"{who}: {R} trials x {n} rows exceed {_lib.BATCH_MAX_ROWS} rows in all")
        mus = [int(m) for m in mus]
        if len(mus) != R:
            raise SesError(f"{who}: {len(mus)} values of mu for {R} trials")
        for r, m in enumerate(mus):
            if not 1 <= m <= n:
                raise SesError(f"{who}: trial {r} has mu = {m} outside [1, {n}]")
        try:
            self._chk(trials, "trials", torch.uint8, (R, tsize))
            self._chk(consts, "consts", torch.uint8, (R, csize))
            self._chk(weights, "weights", torch.float32, (R, n))
            self._chk(fitness, "fitness", torch.float32, (R * n,))
            if best is not None:
                if isinstance(best, torch.Tensor) and best.device.type == "cpu":
                    if not (best.is_pinned() and best.dtype == torch.float32 and tuple(best.shape) == (R,) and best.is_contiguous()):
                        raise SesError(f"best: a host tensor must be pinned float32[{R}]")
                else:
                    self._chk(best, "best", torch.float32, (R,))
            theta = (self.empty(R * n, self.P) if theta_next is None else
                     self._chk(theta_next, "theta_next", torch.float32, (R * n, self.P)))
            self._chk_state(who, ("mu", "C", "p_sigma", "p_c", "step"), ((R, self.P),) * 4 + ((R,),), state_in, state_out)
        except SesError as e:
            raise SesError(str(e) if str(e).startswith(who) else f"{who}: {e}") from None
        check(self._lib.ses_sepcma_generation_batch(self._h, _ptr(fitness), R, n, (ctypes.c_int32 * R)(*mus), _ptr(trials), _ptr(consts),
                                                    _ptr(weights), *[_ptr(t) for t in state_in], *[_ptr(t) for t in state_out],
                                                    _ptr(theta), _ptr(best)), "ses_sepcma_generation_batch")
        return theta

    # -- lm_ma_es (ses_perturb_lmma / ses_lmma_generation) ------------------------------------------
    def _chk_lmma(self, who, params, M, m_active, name="M"):
        if not isinstance(params, _lib.SesLmmaParams):
            raise SesError(f"{who}: params must be a SesLmmaParams")
        if self.P > _lib.LMMA_MAX_P:
            raise SesError(f"{who}: {self.P} parameters; the lm_ma_es kernels hold at most {_lib.LMMA_MAX_P}")
        if not 0 <= params.m <= _lib.LMMA_MAX_MEMORY:
            raise SesError(f"{who}: memory = {params.m} outside [0, {_lib.LMMA_MAX_MEMORY}]")
        if not 0 <= m_active <= params.m:
            raise SesError(f"{who}: m_active = {m_active} outside [0, memory = {params.m}]")
        self._chk(M, name, torch.float32, (params.m, self.P))

    def perturb_lmma(self, mu, M, step, params, m_active, sigma, seed, gen, first_row, n_rows, out=None, want_dots=False):
        """Rows [first_row, first_row + n_rows) of the population mu + (sigma * step) * v, v = the row's noise passed through the
        first m_active rank-one transforms of M (float32[params.m, P]).  step: float32[1] on the device.  Returns theta[n_rows, P],
        or (theta, dots[n_rows, m_active]) with want_dots."""
        self._chk_vectors(("mu", "step"), (mu, step), ((self.P,), (1,)))
        self._chk_lmma("perturb_lmma", params, M, m_active)
        theta = self._perturb_rows("perturb_lmma", first_row, n_rows, out)
        dots = self.empty(n_rows, m_active) if want_dots else None
        check(self._lib.ses_perturb_lmma(self._h, _ptr(mu), _ptr(M) if params.m else None, _ptr(step), ctypes.byref(params),
                                         int(m_active), float(sigma), int(seed), int(gen), int(first_row), int(n_rows), _ptr(theta),
                                         _ptr(dots) if want_dots and m_active else None), "ses_perturb_lmma")
        return (theta, dots) if want_dots else theta

    def lmma_generation(self, fitness, seed, gen, sigma, params, weights, m_active, m_active_next, state_in, state_out, next_sigma,
                        next_gen, first_row, n_rows, theta_next=None, best=None, want_sums=False):
        """ses_lmma_generation: rank, the weighted sum Sz over the params.mu best rows, the update of (mu, p_sigma, M, step) and the
        next population.  params: a _lib.SesLmmaParams; weights: float32[params.mu] on the device; state_in / state_out:
        (mu, p_sigma, M, step) quadruples of distinct tensors (float32[P], float32[P], float32[params.m, P], float32[1]).  Returns
        theta_next[n_rows, P], or (theta_next, Sz, u_last, sdots[m_active], norm2 (float64[1]), dots_next[n_rows, m_active_next])
        with want_sums."""
        n = fitness.shape[0]
        self._chk(fitness, "fitness", torch.float32, (n,))
        if n < 4:
            raise SesError(f"lmma_generation: the population must have at least 4 rows, got {n}")
        # (M's shape depends on params: _chk_lmma checks it)
        self._chk_state("lmma_generation", ("mu", "p_sigma", "M", "step"), ((self.P,), (self.P,), None, (1,)), state_in, state_out)
        self._chk_lmma("lmma_generation", params, state_in[2], m_active, "M_in")
        self._chk_lmma("lmma_generation", params, state_out[2], m_active_next, "M_out")
        if not 1 <= params.mu <= n:
            raise SesError(f"lmma_generation: mu = {params.mu} outside [1, {n}]")
        self._chk(weights, "weights", torch.float32, (params.mu,))
        if not 0.0 < params.step_lo <= params.step_hi:
            raise SesError("lmma_generation: need 0 < step_lo <= step_hi")
        theta = self._next_rows("lmma_generation", n, first_row, n_rows, theta_next, best)
        sz = self.empty(self.P) if want_sums else None
        sd = self.empty(self.P) if want_sums else None
        sdots = self.empty(m_active) if want_sums else None
        norm2 = self.empty(1, dtype=torch.float64) if want_sums else None
        dots = self.empty(n_rows, m_active_next) if want_sums else None

        def opt(t):
            return _ptr(t) if t is not None and t.numel() else None
        M_in, M_out = (opt(state_in[2]), opt(state_out[2]))
        check(self._lib.ses_lmma_generation(self._h, _ptr(fitness), int(n), int(seed), int(gen), float(sigma), ctypes.byref(params),
                                            _ptr(weights), int(m_active), int(m_active_next), _ptr(state_in[0]), _ptr(state_in[1]),
                                            M_in, _ptr(state_in[3]), _ptr(state_out[0]), _ptr(state_out[1]), M_out,
                                            _ptr(state_out[3]), float(next_sigma), int(next_gen), int(first_row), int(n_rows),
                                            _ptr(theta) if n_rows else None, _ptr(best), _ptr(sz), _ptr(sd), opt(sdots), _ptr(norm2),
                                            opt(dots)), "ses_lmma_generation")
        return (theta, sz, sd, sdots, norm2, dots) if want_sums else theta

    # -- ma_es (ses_perturb_maes / ses_maes_generation) ----------------------------------------------
    def _chk_maes(self, who):
        if self.P > _lib.MAES_MAX_P:
            raise SesError(f"{who}: {self.P} parameters; the ma_es kernels hold at most {_lib.MAES_MAX_P} "
                           "(lm_ma_es serves larger policies)")

    def perturb_maes(self, mu, M, step, sigma, seed, gen, first_row, n_rows, out=None, d_out=None, want_d=False):
        """Rows [first_row, first_row + n_rows) of the population mu + (sigma * step) * D, D = Z M^T with M float32[P, P].  step:
        float32[1] on the device.  d_out: optional float32[n_rows, P] that receives D (want_d allocates it).  Returns
        theta[n_rows, P], or (theta, D) with d_out / want_d."""
        self._chk_maes("perturb_maes")
        self._chk_vectors(("mu", "M", "step"), (mu, M, step), ((self.P,), (self.P, self.P), (1,)))
        theta = self._perturb_rows("perturb_maes", first_row, n_rows, out)
        if d_out is None and want_d:
            d_out = self.empty(n_rows, self.P)
        if d_out is not None:
            self._chk(d_out, "d_out", torch.float32, (n_rows, self.P))
        check(self._lib.ses_perturb_maes(self._h, _ptr(mu), _ptr(M), _ptr(step), float(sigma), int(seed), int(gen), int(first_row),
                                         int(n_rows), _ptr(theta), _ptr(d_out)), "ses_perturb_maes")
        return theta if d_out is None else (theta, d_out)

    def maes_generation(self, fitness, seed, gen, sigma, params, weights, state_in, state_out, d_in, next_sigma, next_gen, first_row,
                        n_rows, theta_next=None, d_next_out=None, best=None, want_sums=False):
        """ses_maes_generation: rank, the weighted sum Sz over the params.mu best rows, the update of (mu, p_sigma, M, step) and the
        next population.  params: a _lib.SesMaesParams; weights: float32[params.mu] on the device; state_in / state_out:
        (mu, p_sigma, M, step) quadruples of distinct tensors (float32[P], float32[P], float32[P, P], float32[1]); d_in: float32[n, P],
        the D of the evaluated population, or None (the call recomputes it); d_next_out: optional float32[n_rows, P] <- the D of the
        next population's rows.  Returns theta_next[n_rows, P], or (theta_next, Sz, Sd, qv, G[P, P], norm2 (float64[1])) with
        want_sums."""
        n = fitness.shape[0]
        self._chk_maes("maes_generation")
        self._chk(fitness, "fitness", torch.float32, (n,))
        if n < 4:
            raise SesError(f"maes_generation: the population must have at least 4 rows, got {n}")
        if not isinstance(params, _lib.SesMaesParams):
            raise SesError("maes_generation: params must be a SesMaesParams")
        self._chk_state("maes_generation", ("mu", "p_sigma", "M", "step"), ((self.P,), (self.P,), (self.P, self.P), (1,)), state_in,
                        state_out)
        if not 1 <= params.mu <= n:
            raise SesError(f"maes_generation: mu = {params.mu} outside [1, {n}]")
        self._chk(weights, "weights", torch.float32, (params.mu,))
        if not 0.0 < params.step_lo <= params.step_hi:
            raise SesError("maes_generation: need 0 < step_lo <= step_hi")
        if d_in is not None:
            self._chk(d_in, "d_in", torch.float32, (n, self.P))
        theta = self._next_rows("maes_generation", n, first_row, n_rows, theta_next, best)
        if d_next_out is not None:
            self._chk(d_next_out, "d_next_out", torch.float32, (n_rows, self.P))
            if d_in is not None and d_in.data_ptr() == d_next_out.data_ptr() and d_in.numel():
                raise SesError("maes_generation: d_in and d_next_out must be distinct buffers")
        sz, sd, qv = (self.empty(self.P) if want_sums else None for _ in range(3))
        g = self.empty(self.P, self.P) if want_sums else None
        norm2 = self.empty(1, dtype=torch.float64) if want_sums else None

        def opt(t):
            return _ptr(t) if t is not None and t.numel() else None
        check(self._lib.ses_maes_generation(self._h, _ptr(fitness), int(n), int(seed), int(gen), float(sigma), ctypes.byref(params),
                                            _ptr(weights), _ptr(state_in[0]), _ptr(state_in[1]), _ptr(state_in[2]), _ptr(state_in[3]),
                                            opt(d_in), _ptr(state_out[0]), _ptr(state_out[1]), _ptr(state_out[2]), _ptr(state_out[3]),
                                            float(next_sigma), int(next_gen), int(first_row), int(n_rows),
                                            _ptr(theta) if n_rows else None, opt(d_next_out), _ptr(best), _ptr(sz), _ptr(sd), _ptr(qv),
                                            _ptr(g), _ptr(norm2)), "ses_maes_generation")
        return (theta, sz, sd, qv, g, norm2) if want_sums else theta

    def es_update_stored(self, weights, eps_store, lr, sigma, adam_a, mu, m, v, want_grad=False):
        n = weights.shape[0]
        self._chk(weights, "weights", torch.float64, (n,))
        self._chk(eps_store, "eps_store", torch.float32, (n, self.P))
        for name, t in (("mu", mu), ("m", m), ("v", v)):
            self._chk(t, name, torch.float32, (self.P,))
        grad = self.empty(self.P) if want_grad else None
        check(self._lib.ses_es_update_stored(self._h, _ptr(weights), int(n), _ptr(eps_store), float(lr), float(sigma),
                                             float(adam_a), _ptr(mu), _ptr(m), _ptr(v), _ptr(grad)),
              "ses_es_update_stored")
        return grad

    def elite_ids(self, rank, k):
        n = rank.shape[0]
        self._chk(rank, "rank", torch.int32, (n,))
        if not 1 <= k <= n:
            raise SesError(f"elite_ids: need 1 <= k <= n, got k={k} n={n}")
        ids = self.empty(k, dtype=torch.int32)
        check(self._lib.ses_elite_ids(self._h, _ptr(rank), int(n), int(k), _ptr(ids)), "ses_elite_ids")
        return ids

    def elite_select(self, rank, k, parent_map, alias_state=None):
        """One launch: (elite_ids[k], elite_parent_idx[k], alias_first[k] or None), all on the device.
        alias_state: int32[1] device tensor updated in place (simple_evolution), or None (simple_genetic)."""
        n = rank.shape[0]
        self._chk(rank, "rank", torch.int32, (n,))
        self._chk(parent_map, "parent_map", torch.int32, (n,))
        self._chk(alias_state, "alias_state", torch.int32, (1,), optional=True)
        if not 1 <= k <= min(n, 1024):
            raise SesError(f"elite_select: need 1 <= k <= min(n, 1024), got k={k} n={n}")
        out = self.empty(3, k, dtype=torch.int32)
        alias = out[2] if alias_state is not None else None
        check(self._lib.ses_elite_select(self._h, _ptr(rank), int(n), int(k), _ptr(parent_map), _ptr(alias_state),
                                         _ptr(out[0]), _ptr(out[1]), _ptr(alias)), "ses_elite_select")
        return out[0], out[1], alias

    def elite_mean(self, rows, alias_first=None):
        k = rows.shape[0]
        self._chk(rows, "rows", torch.float32, (k, self.P))
        self._chk(alias_first, "alias_first", torch.int32, (k,), optional=True)
        mean = self.empty(self.P)
        check(self._lib.ses_elite_mean(self._h, _ptr(rows), _ptr(alias_first), int(k), _ptr(mean)), "ses_elite_mean")
        return mean

    def gather_rows(self, src, ids):
        n_src = src.shape[0]
        k = ids.shape[0]
        self._chk(src, "src", torch.float32, (n_src, self.P))
        self._chk(ids, "ids", torch.int32, (k,))
        lo, hi = int(ids.min()), int(ids.max())
        if lo < 0 or hi >= n_src:
            raise SesError(f"gather_rows: ids outside [0, {n_src})")
        dst = self.empty(k, self.P)
        check(self._lib.ses_gather_rows(self._h, _ptr(src), _ptr(ids), int(k), _ptr(dst)), "ses_gather_rows")
        return dst
