"""Several ranks sharing the one GPU of the test box (gloo rendezvous; RCCL refuses duplicate devices): the sharded
generation loop must give every rank the identical fitness vector and parent, bit-equal to a single-rank run.
This is the population-sharding path that bench.py --gpus N / run_es.py use on a multi-GPU node, and the fitness
all-gather is the library's own peer-store transport (ses_comm_p2p_*: mailboxes mapped across processes with hipIpc --
same mechanism across GPUs over xGMI); with SES_COMM_P2P=0 the torch.distributed fallback carries it."""
import os
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "simple-es_amd")

WORKER = textwrap.dedent("""
    import contextlib, io, os, sys
    import numpy as np, torch, yaml
    sys.path[:0] = [%r, %r]
    out_dir, world = sys.argv[1], int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo")
    import builder
    os.chdir(out_dir)
    for name, n in (("openai_es", 203), ("simple_evolution", 96), ("simple_genetic", 120)):
        cfg = {"env": {"name": "CartPole-v1", "max_step": 200, "pomdp": False, "seed": 3},
               "network": {"name": "gym_model", "num_state": 4, "num_action": 2, "discrete_action": True, "gru": False},
               "strategy": {"name": name, "init_sigma": 0.5, "sigma_decay": 0.99, "learning_rate": 0.05,
                            "elite_num": 8, "offspring_num": n, "seed": 5}}
        loop = builder.build_loop(cfg, 4, 1, 3, False, 10 ** 9)
        fits = []
        orig = loop.rollout
        loop.rollout = lambda pop, _o=orig: (fits.append(_o(pop).cpu().numpy().copy()) or torch.from_numpy(fits[-1]).cuda())
        with contextlib.redirect_stdout(io.StringIO()):
            loop.run()
        rank = int(os.environ.get("RANK", "0"))
        from ses.parallel import comm_transport
        open(os.path.join(out_dir, f"{name}_w{world}_r{rank}.transport"), "w").write(comm_transport(loop.dev))
        elite = loop.offspring_strategy.get_elite_model().flat()
        np.savez(os.path.join(out_dir, f"{name}_w{world}_r{rank}.npz"), fits=np.stack(fits), elite=elite,
                 best=np.array([b for b, _ in loop.history]))
    if world > 1:
        dist.destroy_process_group()
""")


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


# (the GPU boxes admit at most 6 processes on a card; the test runner and the launcher hold one each, so 4 ranks is the
#  largest world this rig can form -- 5 ranks were killed by the box's process guard.  The 8-rank layout -- shard
#  boundaries, ragged tail -- is covered on the CPU in tests/test_host_logic.py)
@pytest.mark.parametrize("world,p2p", [(2, True), (4, True), (2, False)],
                         ids=["2_ranks_peer_stores", "4_ranks_peer_stores", "2_ranks_torch_fallback"])
def test_ranks_equal_one_rank_bitwise(tmp_path, world, p2p):
    script = tmp_path / "w.py"
    script.write_text(WORKER % (ROOT, SRC))
    one = subprocess.run([sys.executable, str(script), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stdout + one.stderr
    env = {**os.environ, "SES_COMM_P2P": "1" if p2p else "0"}
    many = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
                           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), str(script), str(tmp_path)],
                          capture_output=True, text=True, timeout=900, env=env)
    assert many.returncode == 0, many.stdout + many.stderr
    for name in ("openai_es", "simple_evolution", "simple_genetic"):
        ref = np.load(tmp_path / f"{name}_w1_r0.npz")
        for r in range(world):
            got = np.load(tmp_path / f"{name}_w{world}_r{r}.npz")
            assert np.array_equal(got["fits"].view(np.uint32), ref["fits"].view(np.uint32)), (name, r, "fitness")
            assert np.array_equal(got["elite"].view(np.uint32), ref["elite"].view(np.uint32)), (name, r, "elite")
            assert np.array_equal(got["best"], ref["best"])
            transport = open(tmp_path / f"{name}_w{world}_r{r}.transport").read()
            assert transport == ("p2p-store" if p2p else "torch"), (name, r, transport, many.stderr[-2000:])
        assert ref["fits"].shape[0] == 4 and ref["fits"].std() > 0


C4_WORKER = textwrap.dedent("""
    import os, sys
    import numpy as np, torch
    sys.path[:0] = [%r, %r]
    out_dir = sys.argv[1]
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    import builder
    from ses.parallel import comm_transport
    os.chdir(out_dir)
    # BASELINE configs[3] per rank: 8192 offspring on every rank, the replicated fitness loop over all world * 8192 rows
    n = 8192 * world
    cfg = {"env": {"name": "CartPole-v1", "max_step": 30, "pomdp": False, "seed": 1, "shared_init": True},
           "network": {"name": "gym_model", "num_state": 4, "num_action": 2, "discrete_action": True, "gru": False},
           "strategy": {"name": "openai_es", "init_sigma": 0.3, "sigma_decay": 0.99, "learning_rate": 0.05,
                        "offspring_num": n, "seed": 9}}
    loop = builder.build_loop(cfg, 3, 1, 2, False, 10 ** 9)
    pop = loop.offspring_strategy.init_offspring(loop.network, loop.env.get_agent_ids())
    assert pop.theta.shape[0] == 8192 and pop.shard.first == rank * 8192
    fits = []
    for g in range(3):
        fit = loop.rollout(pop)
        assert fit.shape[0] == n
        fits.append(fit.cpu().numpy().copy())
        pop, best, sigma = loop.offspring_strategy.evaluate(fit)
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, f"c4_r{rank}.npz"), fits=np.stack(fits), mu=loop.offspring_strategy.mu_model.cpu().numpy(),
             transport=np.array(comm_transport(loop.dev, 8192)))
    dist.destroy_process_group()
""")


def test_c4_shape_four_ranks_of_8192_rows_over_peer_stores(tmp_path):
    """The C4 layout on the rig: every rank owns 8192 rows (32 KB shards, two 4096-float slices each), the fitness loop
    runs replicated over all 32 768 rows (sort + search rank path), peer stores carry the exchange; all ranks end
    with the same fitness vectors and the same parent, bit for bit."""
    world = 4
    script = tmp_path / "c4.py"
    script.write_text(C4_WORKER % (ROOT, SRC))
    run = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
                          "--master-addr", "127.0.0.1", "--master-port", str(free_port()), str(script), str(tmp_path)],
                         capture_output=True, text=True, timeout=900, env={**os.environ, "SES_COMM_P2P": "1"})
    assert run.returncode == 0, run.stdout + run.stderr
    ref = np.load(tmp_path / "c4_r0.npz")
    assert str(ref["transport"]) == "p2p-store"
    assert ref["fits"].shape == (3, 8192 * world) and np.isfinite(ref["fits"]).all() and ref["fits"].std() > 0
    for r in range(1, world):
        got = np.load(tmp_path / f"c4_r{r}.npz")
        assert str(got["transport"]) == "p2p-store"
        assert np.array_equal(got["fits"].view(np.uint32), ref["fits"].view(np.uint32)), r
        assert np.array_equal(got["mu"].view(np.uint32), ref["mu"].view(np.uint32)), r


FREEZE_WORKER = textwrap.dedent("""
    import contextlib, io, os, sys, time
    import numpy as np, torch
    sys.path[:0] = [%r, %r]
    out_dir, world = sys.argv[1], int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo")
    rank = int(os.environ.get("RANK", "0"))
    import builder
    from learning_strategies.evolution.loop import ESLoop
    from ses.parallel import comm_transport
    ESLoop.comm_check_period = 4
    batched = len(sys.argv) > 2 and sys.argv[2] == "batched"
    from learning_strategies.evolution import loop as loop_module
    os.chdir(out_dir)
    for name, n in (("openai_es", 203), ("simple_evolution", 96), ("simple_genetic", 120)):
        cfg = {"env": {"name": "CartPole-v1", "max_step": 100, "pomdp": False, "seed": 3},
               "network": {"name": "gym_model", "num_state": 4, "num_action": 2, "discrete_action": True, "gru": False},
               "strategy": {"name": name, "init_sigma": 0.5, "sigma_decay": 0.99, "learning_rate": 0.05,
                            "elite_num": 8, "offspring_num": n, "seed": 5}}
        loop = builder.build_loop(cfg, 12, 1, 3, False, 8)
        before = comm_transport(loop.dev) if world > 1 else "none"
        calls = [0]
        orig = loop.generation
        def generation(pop, _o=orig):
            calls[0] += 1
            if world > 1 and rank == 1 and calls[0] == 6 and name == "openai_es":
                torch.cuda.synchronize()
                time.sleep(1.5)                      # this rank freezes for five time-outs of its peer
            return _o(pop)
        orig_run = loop_module._GenerationBatch.run
        chunks = [0]
        def run_chunk(self, k, _o=orig_run):
            # the device-side loop (ses_run_generations): the stall sits between two chunks, on the CLASS -- a hook on the loop
            # object would put run() back on the per-generation path
            chunks[0] += 1
            if world > 1 and rank == 1 and chunks[0] == 2 and name == "openai_es":
                torch.cuda.synchronize()
                time.sleep(1.5)
            return _o(self, k)
        orig_gen = ESLoop.generation
        def counted(self, pop, _o=orig_gen):       # on the class: the per-generation calls of the replay are counted, run() stays eligible
            calls[0] += 1
            return _o(self, pop)
        if batched:
            loop_module._GenerationBatch.run = run_chunk
            ESLoop.generation = counted
        else:
            loop.generation = generation
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                loop.run()
        finally:
            loop_module._GenerationBatch.run = orig_run
            ESLoop.generation = orig_gen
        if batched:
            calls[0] += loop.batched_generations
        after = comm_transport(loop.dev) if world > 1 else "none"
        elite = loop.offspring_strategy.get_elite_model().flat()
        saved = sorted(os.listdir(os.path.join(loop.save_dir, "saved_models"))) if loop.save_dir else []
        np.savez(os.path.join(out_dir, f"fz_{name}_w{world}_r{rank}.npz"), elite=elite, best=np.array([b for b, _ in loop.history]),
                 sigma=np.array([s for _, s in loop.history]), transports=np.array([before, after]), calls=calls[0],
                 saved=np.array(saved))
    if world > 1:
        dist.destroy_process_group()
""")


@pytest.mark.parametrize("mode", ["stepwise", "batched"])
def test_a_frozen_rank_costs_a_rollback_not_the_run(tmp_path, mode):
    """(batched: the same through the device-side loop -- the stall between two ses_run_generations chunks, the time-out inside the
    kernels that poll the granules, the rollback out of a batched segment, the deferred checkpoints.)
    One rank stalls for 1.5 s while its peer's exchanges give up after 0.3 s (SES_COMM_P2P_TIMEOUT_MS): the run is not
    killed and nothing diverges silently -- at the next boundary the ranks agree that an exchange failed, drop the
    peer-store transport (torch.distributed carries the all-gather from there on this rig), roll back to the last
    boundary and replay.  History, sigma trace and final parent equal the undisturbed one-rank run bit for bit, and
    the strategies that ran afterwards (no transport left) are equal too."""
    script = tmp_path / "fz.py"
    script.write_text(FREEZE_WORKER % (ROOT, SRC))
    one = subprocess.run([sys.executable, str(script), str(tmp_path), mode], capture_output=True, text=True, timeout=600)
    assert one.returncode == 0, one.stdout + one.stderr
    env = {**os.environ, "SES_COMM_P2P": "1", "SES_COMM_P2P_TIMEOUT_MS": "300"}
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(free_port()), str(script), str(tmp_path), mode],
                         capture_output=True, text=True, timeout=900, env=env)
    assert two.returncode == 0, two.stdout + two.stderr
    assert "timed out" in two.stderr
    for name in ("openai_es", "simple_evolution", "simple_genetic"):
        ref = np.load(tmp_path / f"fz_{name}_w1_r0.npz")
        for r in range(2):
            got = np.load(tmp_path / f"fz_{name}_w2_r{r}.npz")
            assert np.array_equal(got["elite"].view(np.uint32), ref["elite"].view(np.uint32)), (name, r)
            assert np.array_equal(got["best"], ref["best"]) and np.array_equal(got["sigma"], ref["sigma"]), (name, r)
            if name == "openai_es":
                assert list(got["transports"]) == ["p2p-store", "torch"], got["transports"]
                assert int(got["calls"]) > 12                     # generations were replayed
            else:
                assert list(got["transports"]) == ["torch", "torch"]
        assert list(np.load(tmp_path / f"fz_{name}_w2_r0.npz")["saved"]) == ["ep_8.pt"]


# ---- round 4: the shard form of the openai_es tail and the device-side generation loop on several ranks -----------------

SHARDED_WORKER = textwrap.dedent("""
    import contextlib, io, os, sys
    import numpy as np, torch
    sys.path[:0] = [%r, %r]
    out_dir, world = sys.argv[1], int(os.environ.get("WORLD_SIZE", "1"))
    sizes = [int(x) for x in sys.argv[2].split(",")]
    batched = sys.argv[3] == "batched"
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo")
    rank = int(os.environ.get("RANK", "0"))
    import builder
    os.chdir(out_dir)
    for n in sizes:
        cfg = {"env": {"name": "CartPole-v1", "max_step": 25, "pomdp": False, "seed": 3},
               "network": {"name": "gym_model", "num_state": 4, "num_action": 2, "discrete_action": True, "gru": False},
               "strategy": {"name": "openai_es", "init_sigma": 0.5, "sigma_decay": 0.99, "learning_rate": 0.05,
                            "offspring_num": n, "seed": 5}}
        loop = builder.build_loop(cfg, 5, 1, 2, False, 10 ** 9)
        owner0 = getattr(loop.dev, "_comm_owner", None)
        counts0 = owner0.comm_p2p_counts() if owner0 is not None else (0, 0)
        fits = []
        if not batched:                      # observing the rollouts keeps run() on the per-generation path
            orig = loop.rollout
            loop.rollout = lambda pop, _o=orig: (fits.append(_o(pop).cpu().numpy().copy()) or torch.from_numpy(fits[-1]).cuda())
        with contextlib.redirect_stdout(io.StringIO()):
            pop = loop.run()
        strat = loop.offspring_strategy
        sharded = False
        if world > 1:
            owner = getattr(strat.dev, "_comm_owner", None)
            sharded = owner is not None and strat.dev.openai_sharded_ok(owner, n, pop.shard.per_rank, world)
        np.savez(os.path.join(out_dir, f"sh_{n}_w{world}_r{rank}.npz"), fits=np.stack(fits) if fits else np.zeros(0),
                 elite=strat.get_elite_model().flat(), best=np.array([b for b, _ in loop.history]),
                 m=strat.optimizer.m.cpu().numpy(), v=strat.optimizer.v.cpu().numpy(), theta=pop.theta.cpu().numpy(),
                 first=pop.shard.first, sharded=sharded, batched_generations=loop.batched_generations,
                 exchanges=np.array(owner0.comm_p2p_counts() if owner0 is not None else (0, 0)) - np.array(counts0))
    if world > 1:
        dist.destroy_process_group()
""")


def _run_ranks(script, tmp_path, world, extra, env=None, timeout=900):
    cmd = ([sys.executable, str(script), str(tmp_path)] if world == 1 else
           [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
            "--master-addr", "127.0.0.1", "--master-port", str(free_port()), str(script), str(tmp_path)]) + list(extra)
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env={**os.environ, "SES_COMM_P2P": "1", **(env or {})})
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    return run


@pytest.mark.parametrize("world,sizes,mode,tuning",
                         [(2, "2048,10239", "stepwise", ""), (4, "4096,12285", "stepwise", ""), (2, "2048,10239", "batched", ""),
                          (4, "12285", "batched", ""), (2, "10239", "batched", "fused_fitness_exchange=0"),
                          (2, "10239", "batched", "openai_granule_exchange=0")],
                         ids=["2_ranks", "4_ranks", "2_ranks_device_loop", "4_ranks_device_loop", "2_ranks_device_loop_fitness_allgather",
                              "2_ranks_device_loop_partials_allgather"])
def test_sharded_openai_tail_equals_one_rank_bitwise(tmp_path, world, sizes, mode, tuning):
    """Shards aligned to the gradient's 1024-row chunks: every rank ranks and accumulates its own rows only, the chunk
    partials (and the best-reward candidates) are all-gathered through the mailboxes, the ordered update finishes --
    fitness vectors, best rewards, parent, Adam moments and the next population's rows equal the one-rank run bit for bit.
    2048 rows: counting rank; 10 239 / 12 285: one sort + search launch, last shard ragged (5119 of 5120, 3069 of 3072
    rows).  `device_loop`: the same through ESLoop.run()'s ses_run_generations path -- with BOTH exchanges of a generation fused
    into the kernels around them (the episode-mean kernel stores the fitness granules, the rank kernel -- counting, or sort +
    search -- polls them; the gradient kernel stores the partials, the update polls them); the last two cases switch one of
    the two back to an all-gather launch of its own."""
    script = tmp_path / "sh.py"
    script.write_text(SHARDED_WORKER % (ROOT, SRC))
    _run_ranks(script, tmp_path, 1, [sizes, mode])
    # (openai_sharded_min_rows=0: the product keeps populations below 8192 rows in total replicated -- measured faster, round 6 --
    #  and this test is about the shard form, at 2048 and 4096 rows too)
    _run_ranks(script, tmp_path, world, [sizes, mode], env={"SES_TUNING": ",".join(filter(None, ["openai_sharded_min_rows=0", tuning]))})
    for n in (int(x) for x in sizes.split(",")):
        ref = np.load(tmp_path / f"sh_{n}_w1_r0.npz")
        assert len(ref["best"]) == 5 and np.isfinite(ref["best"]).all()
        for r in range(world):
            got = np.load(tmp_path / f"sh_{n}_w{world}_r{r}.npz")
            assert bool(got["sharded"]), (n, r, "the shard form was not available")
            for key in ("fits", "elite", "m", "v"):
                assert np.array_equal(got[key].view(np.uint32), ref[key].view(np.uint32)), (n, r, key)
            assert np.array_equal(got["best"], ref["best"]), (n, r)
            lo = int(got["first"])
            assert np.array_equal(got["theta"].view(np.uint32), ref["theta"][lo:lo + got["theta"].shape[0]].view(np.uint32)), (n, r)
            assert int(got["batched_generations"]) == (5 if mode == "batched" else 0)
            # what carried the two exchanges of the 5 generations: (launches of ses_allgather_fitness, granule exchanges)
            want = {("stepwise", ""): (5, 5), ("batched", "fused_fitness_exchange=0"): (5, 5), ("batched", "openai_granule_exchange=0"): (5, 5),
                    ("batched", ""): (0, 10)}[(mode, tuning)]
            assert tuple(int(v) for v in got["exchanges"]) == want, (n, r, mode, tuning, got["exchanges"])
        assert int(ref["batched_generations"]) == (5 if mode == "batched" else 0)


BATCHED_WORKER = textwrap.dedent("""
    import contextlib, io, os, sys, time
    import numpy as np, torch
    sys.path[:0] = [%r, %r]
    out_dir, world = sys.argv[1], int(os.environ.get("WORLD_SIZE", "1"))
    freeze = len(sys.argv) > 2 and sys.argv[2] == "freeze"
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo")
    rank = int(os.environ.get("RANK", "0"))
    import builder
    from learning_strategies.evolution import loop as loop_mod
    from ses.parallel import comm_transport
    loop_mod.ESLoop.comm_check_period = 4
    os.chdir(out_dir)
    for name, n in (("openai_es", 203), ("simple_evolution", 96), ("simple_genetic", 120)):
        cfg = {"env": {"name": "CartPole-v1", "max_step": 100, "pomdp": False, "seed": 3},
               "network": {"name": "gym_model", "num_state": 4, "num_action": 2, "discrete_action": True, "gru": False},
               "strategy": {"name": name, "init_sigma": 0.5, "sigma_decay": 0.99, "learning_rate": 0.05,
                            "elite_num": 8, "offspring_num": n, "seed": 5}}
        loop = builder.build_loop(cfg, 12, 1, 3, False, 8)
        before = comm_transport(loop.dev) if world > 1 else "none"
        calls = [0]
        orig = loop_mod._GenerationBatch.run
        def run(self, k, _o=orig):
            calls[0] += 1
            if freeze and world > 1 and rank == 1 and calls[0] == 2 and name == "openai_es":
                torch.cuda.synchronize()
                time.sleep(1.5)                      # this rank freezes for five time-outs of its peer
            return _o(self, k)
        loop_mod._GenerationBatch.run = run
        with contextlib.redirect_stdout(io.StringIO()):
            loop.run()
        loop_mod._GenerationBatch.run = orig
        after = comm_transport(loop.dev) if world > 1 else "none"
        elite = loop.offspring_strategy.get_elite_model().flat()
        saved = sorted(os.listdir(os.path.join(loop.save_dir, "saved_models"))) if loop.save_dir else []
        rows = [l for l in open(os.path.join(loop.save_dir, "metrics.jsonl"))] if loop.save_dir else []
        np.savez(os.path.join(out_dir, f"bt_{name}_w{world}_r{rank}.npz"), elite=elite, best=np.array([b for b, _ in loop.history]),
                 sigma=np.array([s for _, s in loop.history]), transports=np.array([before, after]), calls=calls[0],
                 saved=np.array(saved), batched_generations=loop.batched_generations,
                 rollbacks=sum('"rollback_to"' in l for l in rows))
    if world > 1:
        dist.destroy_process_group()
""")


@pytest.mark.parametrize("world", [2, 4])
def test_device_side_loop_on_several_ranks_equals_one_rank(tmp_path, world):
    """ESLoop.run() with no observer: on several ranks, too, the generations go to the device through ses_run_generations
    (rollout of the own rows, fitness all-gather by peer stores INSIDE the C loop, the strategy's tail, the own rows of the
    next population), all three strategies, shards of 203 / 97 / 120 rows that no chunk boundary divides (the replicated
    tail) -- history, sigma trace, parent and the one checkpoint equal the one-rank run."""
    script = tmp_path / "bt.py"
    script.write_text(BATCHED_WORKER % (ROOT, SRC))
    _run_ranks(script, tmp_path, 1, [])
    _run_ranks(script, tmp_path, world, [])
    for name in ("openai_es", "simple_evolution", "simple_genetic"):
        ref = np.load(tmp_path / f"bt_{name}_w1_r0.npz")
        assert int(ref["batched_generations"]) == 12
        for r in range(world):
            got = np.load(tmp_path / f"bt_{name}_w{world}_r{r}.npz")
            assert list(got["transports"]) == ["p2p-store", "p2p-store"], got["transports"]
            assert int(got["batched_generations"]) == 12, (name, r)
            assert np.array_equal(got["elite"].view(np.uint32), ref["elite"].view(np.uint32)), (name, r)
            assert np.array_equal(got["best"], ref["best"]) and np.array_equal(got["sigma"], ref["sigma"]), (name, r)
        assert list(np.load(tmp_path / f"bt_{name}_w{world}_r0.npz")["saved"]) == ["ep_8.pt"]


def test_a_frozen_rank_in_the_device_side_loop_costs_a_rollback(tmp_path):
    """The same freeze as above, but inside the ses_run_generations path: rank 1 sleeps 1.5 s before it enqueues its second
    chunk of generations, rank 0's exchanges give up after 0.3 s (then after 2 ms each: the peer is known to be late),
    both meet at the boundary, drop the transport, roll back and replay on the per-generation path over torch.distributed
    (this rig has no RCCL between processes of one GPU).  Results equal the undisturbed one-rank run; metrics.jsonl says
    which rows were superseded."""
    script = tmp_path / "bt.py"
    script.write_text(BATCHED_WORKER % (ROOT, SRC))
    _run_ranks(script, tmp_path, 1, [])
    two = _run_ranks(script, tmp_path, 2, ["freeze"], env={"SES_COMM_P2P_TIMEOUT_MS": "300"})
    assert "timed out" in two.stderr
    for name in ("openai_es", "simple_evolution", "simple_genetic"):
        ref = np.load(tmp_path / f"bt_{name}_w1_r0.npz")
        for r in range(2):
            got = np.load(tmp_path / f"bt_{name}_w2_r{r}.npz")
            assert np.array_equal(got["elite"].view(np.uint32), ref["elite"].view(np.uint32)), (name, r)
            assert np.array_equal(got["best"], ref["best"]) and np.array_equal(got["sigma"], ref["sigma"]), (name, r)
            if name == "openai_es":
                assert list(got["transports"]) == ["p2p-store", "torch"], got["transports"]
                assert 0 < int(got["batched_generations"]) <= 12
            else:
                assert list(got["transports"]) == ["torch", "torch"] and int(got["batched_generations"]) == 0
        r0 = np.load(tmp_path / f"bt_{name}_w2_r0.npz")
        assert list(r0["saved"]) == ["ep_8.pt"]
        assert int(r0["rollbacks"]) == (1 if name == "openai_es" else 0)


UNGUARDED_WORKER = textwrap.dedent("""
    import os, sys, time
    import numpy as np, torch
    sys.path[:0] = [%r, %r]
    out_dir = sys.argv[1]
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    from ses import HipES
    from ses._lib import SesError
    from ses.parallel import Shard, attach_comm, comm_failed, comm_transport
    dev = HipES("CartPole-v1", 4, 2, True, False)
    assert attach_comm(dev) and comm_transport(dev, 512) == "p2p-store"
    shard = Shard(1024)
    local = torch.full((512,), float(rank + 1), device=dev.device)
    outcome = "none"
    if rank == 1:
        torch.cuda.synchronize(); time.sleep(1.2)         # far beyond rank 0's time-out
        got = shard.allgather_fitness(local, dev=dev); torch.cuda.synchronize()
        outcome = "late rank: " + ("ok" if bool((got[:512] == 1).all()) else "bad")
    else:
        got = shard.allgather_fitness(local, dev=dev); torch.cuda.synchronize()
        nan_shard = bool(torch.isnan(got[512:]).all()) and bool((got[:512] == 1).all())
        try:
            shard.allgather_fitness(local, dev=dev)
            outcome = "second exchange went through"
        except SesError as exc:
            outcome = f"nan_shard={nan_shard} failed={comm_failed(dev)} raised: {exc}"
    open(os.path.join(out_dir, f"ug_r{rank}.txt"), "w").write(outcome)
    dist.barrier()
    dist.destroy_process_group()
""")


def test_an_unguarded_caller_fails_loudly_after_a_timed_out_exchange(tmp_path):
    """attach_comm leaves "comm_p2p_keep_going" off: whoever all-gathers without ESLoop's roll-back (RolloutWorker, bench
    legs, noise='numpy' strategies, user code) consumes ONE NaN-marked shard and the next exchange raises SES_ERR_COMM --
    a stalled peer cannot feed NaN fitness into ranking, updates and checkpoints indefinitely."""
    script = tmp_path / "ug.py"
    script.write_text(UNGUARDED_WORKER % (ROOT, SRC))
    _run_ranks(script, tmp_path, 2, [], env={"SES_COMM_P2P_TIMEOUT_MS": "200"})
    r0 = open(tmp_path / "ug_r0.txt").read()
    assert r0.startswith("nan_shard=True failed=True raised:") and "timed out" in r0 and "code -5" in r0, r0
    assert open(tmp_path / "ug_r1.txt").read() == "late rank: ok"


def test_run_es_command_line_on_two_ranks(tmp_path):
    """`python -m torch.distributed.run ... run_es.py --cfg-path conf/cartpole_openai.yaml` -- the reference's command line
    (run_es.py:15-62) with the population sharded over two ranks (here: sharing the GPU, gloo control plane): same printed
    best rewards and the same checkpoints as the one-rank command, only rank 0 prints and writes."""
    import re
    import shutil
    outs = {}
    for world in (1, 2):
        work = tmp_path / f"w{world}"
        shutil.copytree(SRC, work, ignore=shutil.ignore_patterns("logs", "__pycache__", "_obj"))
        args = ["run_es.py", "--cfg-path", "conf/cartpole_openai.yaml", "--generation-num", "12", "--offspring-num", "2048",
                "--save-model-period", "5", "--seed", "3"]
        cmd = ([sys.executable] + args if world == 1 else
               [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                "--master-port", str(free_port())] + args)
        run = subprocess.run(cmd, cwd=work, capture_output=True, text=True, timeout=900,
                             env={**os.environ, "SES_DIST_BACKEND": "gloo", "SES_COMM_P2P": "1"})
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-3000:]
        lines = [l for l in run.stdout.splitlines() if l.startswith("episode:")]
        assert len(lines) == 12, run.stdout[-2000:]                    # rank 0 only
        outs[world] = [re.match(r"episode: (\d+), Best reward: ([-0-9.]+), sigma: ([0-9.]+)", l).groups() for l in lines]
        saved = sorted(p.name for p in work.glob("logs/*/*/saved_models/*.pt"))
        assert saved == ["ep_10.pt", "ep_5.pt"], saved
    assert outs[1] == outs[2]


def _bench_line(world, extra_env, tmp_path, flags=()):
    import json
    env = {**os.environ, "SES_BENCH_BACKEND": "gloo", "SES_BENCH_SKIP": "c3 loop e1", **extra_env}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(world), "--steps", "5", "--warmup", "2",
                          "--blocks", "2", "--min-timed-seconds", "0", "--preroll", "10", "--no-roofline", "--full", *flags],
                         capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines                                     # stdout carries ONE line, the JSON
    return json.loads(lines[0])


def test_bench_multi_gpu_line_certifies_itself(tmp_path):
    """bench.py --gpus 2 on the rig (ranks share the GPU, gloo control plane): every job of the N > 1 line carries a shard_check --
    one generation's all-gathered fitness against rank 0's own rollout of the whole population, parent + Adam moments after four
    generations of the timed call against rank 0's single-rank replay -- and it says bit_equal on a population whose returns
    are not all the same value; the strong job is the metric as written (4096 offspring in total)."""
    line = _bench_line(2, {}, tmp_path)
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["config"]["offspring_total"] == 4096
    for key, total in (("strong_4096_total", 4096), ("weak_4096_per_gpu", 8192), ("c4_65536_total", 65536)):
        chk = line[key]["shard_check"]
        assert chk["offspring_total"] == total and chk["ranks"] == 2, (key, chk)
        assert chk["bit_equal"] is True and chk["fitness_bit_equal"] is True and chk["state_bit_equal"] is True, (key, chk)
        assert chk["fitness_distinct_values"] >= 8 and chk["state_nonzero"] is True, (key, chk)
        assert chk["timed_path"].startswith("device-side loop"), (key, chk)
        assert line[key + "_rccl"] == "absent"                        # no RCCL communicator spans ranks that share a device
    assert set(line["legs_wall_s"]) >= {"headline", "headline_shard_check", "weak_4096_per_gpu", "c4_65536_total"}
    assert line["gpu_event_seconds"] > 0 and line["wall_seconds"] >= line["gpu_event_seconds"] * 0.5


def test_bench_shard_check_catches_a_wrong_shard(tmp_path):
    """The certification is only worth something if it can fail: SES_BENCH_FAULT=shard makes rank 1 perturb ONE fitness value of
    its shard (bench.py, test hook) before the exchange of the checked generation -- every rank must then report
    fitness_bit_equal false."""
    line = _bench_line(2, {"SES_BENCH_FAULT": "shard", "SES_BENCH_SKIP": "c3 loop e1 weak_4096_per_gpu c4_65536_total"}, tmp_path)
    chk = line["strong_4096_total"]["shard_check"]
    assert chk["fitness_bit_equal"] is False and chk["bit_equal"] is False, chk
    assert chk["state_bit_equal"] is True, chk                        # the fault touched the checked exchange only


def test_bench_survives_a_hanging_rccl_leg(tmp_path):
    """The RCCL-forced twins run last and behind a watchdog: a leg that never returns (SES_BENCH_FAULT=rccl_hang stands in for an
    ncclAllGather whose peer never arrives) costs the run its RCCL legs, not its line -- every rank exits with code 0 after
    SES_BENCH_RCCL_BUDGET_S, rank 0 having written the line with everything measured before.  (The same watchdog holds the whole
    multi-GPU run to SES_BENCH_TOTAL_BUDGET_S: a second case lets that one run out before the headline is measured -- exit code 4,
    no line.)"""
    line = _bench_line(2, {"SES_BENCH_FAULT": "rccl_hang", "SES_BENCH_RCCL_BUDGET_S": "8",
                           "SES_BENCH_SKIP": "c3 loop e1 weak_4096_per_gpu c4_65536_total small_shards"}, tmp_path)
    assert "budget of the RCCL legs (8 s" in line["watchdog"] and "fault_injected_hang" in line["watchdog"], line.get("watchdog")
    assert line["strong_4096_total"]["shard_check"]["bit_equal"] is True
    assert line["strong_4096_total_rccl"] == "absent" and line["value"] > 0 and "legs_wall_s" in line


def test_bench_plain_line_times_exactly_steps_and_dumps_the_same_outputs(tmp_path):
    """A plain `bench.py --steps K --warmup W` times exactly K generations (one block) and runs none of the --full legs; with
    --dump-outputs two runs with the same arguments write the same arrays, float32, within 64 MB, and the dumped parent is
    the one the timed population's row 0 carries (openai_es: member 0 is mu)."""
    import json
    lines = []
    for k in range(2):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                              "--dump-outputs", str(tmp_path / f"out{k}")],
                             capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
        rows = [ln for ln in out.stdout.splitlines() if ln.strip()]
        assert len(rows) == 1, rows
        lines.append(json.loads(rows[0]))
    line = lines[0]
    assert line["steps"] == 20 and line["blocks"] == 1 and line["ms_per_step"] > 0
    assert abs(line["timed_seconds"] - 20 * line["ms_per_step"] * 1e-3) < 1e-9 + 1e-6 * line["timed_seconds"]
    assert {"metric", "value", "unit", "higher_is_better", "dtype"} <= set(line)
    for key in ("cpu_baseline", "roofline", "rollout_kernel", "c4_65536_total", "e1", "loop_ms_per_generation", "rollout_us"):
        assert key not in line and key not in line["strong_4096_total"], key
    names = sorted(os.listdir(tmp_path / "out0"))
    assert names == sorted(os.listdir(tmp_path / "out1")) and {"theta.npy", "mu.npy", "adam_m.npy", "adam_v.npy"} <= set(names)
    total = 0
    for name in names:
        a, b = np.load(tmp_path / "out0" / name), np.load(tmp_path / "out1" / name)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 << 20
    theta, mu = np.load(tmp_path / "out0" / "theta.npy"), np.load(tmp_path / "out0" / "mu.npy")
    assert theta.shape == (4096, mu.size) and np.array_equal(theta[0], mu) and np.abs(mu).sum() > 0


def test_bench_whose_budget_runs_out_before_the_headline_says_so(tmp_path):
    env = {**os.environ, "SES_BENCH_BACKEND": "gloo", "SES_BENCH_TOTAL_BUDGET_S": "0.5"}
    # (the headline's timed blocks cover 6 s: far beyond the budget)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2", "--no-roofline",
                          "--min-timed-seconds", "6"],
                         capture_output=True, text=True, timeout=600, env=env, cwd=str(tmp_path))
    assert out.returncode != 0 and not out.stdout.strip(), (out.returncode, out.stdout[-500:])
    assert "the headline had not been measured: no line" in out.stderr, out.stderr[-2000:]
