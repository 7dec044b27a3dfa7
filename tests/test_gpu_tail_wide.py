"""The wide form of the openai_es gradient kernel (tuning knob "es_tail_wide", csrc/ses_strategy.hip) against the form before it,
the step-wise entry points and the host oracle.  Everything is compared bit for bit: the wide form moves no IEEE operation.

Gradient, Adam and the next population (ses_openai_generation on a given fitness vector, two consecutive calls on one handle so
that the second count starts from the rank vector the first call's last launch cleared):
  * knob 1 == knob 0: mu, m, v, the next population and best;
  * == ses_rank_center + ses_es_update_philox (the stored-weights gradient) on the same inputs;
  * the step-wise rank == snp.stable_rank, its weights within snp.WEIGHT_ATOL of snp.centered_ranks;
  * the step-wise gradient lies within snp.es_grad_f64's rigorous bound of the float64 gradient, best == max(fitness), the next
    population == the C oracle's perturbation of the new mu.
Sizes: 2 (n - 1 = 1), 255, 1024 (exactly one chunk), 1025 (a second chunk of one row: its slices j >= 1 are empty), 2500 (a ragged
third chunk whose slice j = 1 is partly filled), 4096; each also with "es_final_max_chunks" = 8, the <true> instance.

The gradient behind the rank count that forms the episode means (ses_run_generations, k = 1 twice): E in {1, 2, 5, 8} x n in
{2, 257, 4096} x returns without ties (Pendulum's float returns) / with about half the rows tied / with every row equal, so
that the index decides every compare.  Knob 1, knob 0 and "fused_episode_mean" = 0 must each equal the oracle of
test_gpu_run_generations_oracle.check_generation -- fitness[] == the sequential float64 episode mean, and mu, m, v, the next
population and best == ses_openai_generation on that fitness by a second handle that runs the narrow gradient -- and end in the
same bits.  rank[] itself lives in the handle's scratch and is cleared by the generation's last launch; it is asserted through
what it alone decides: the second handle's rank is compared with snp.stable_rank, and any other rank gives another mu.

The shard and granule instances of the narrow form: two ranks on one GPU (test_gpu_multirank's worker) with the knob at 0 against
one rank at the default, over granules and over the all-gather launch; the existing multi-rank tests run the wide instances.
"""
import math

import numpy as np
import pytest

import test_gpu_multirank as mr
import test_gpu_run_generations_oracle as rgo
from oracle import c_oracle as co
from oracle import strategies_np as snp

pytestmark = pytest.mark.gpu

KNOB = "es_tail_wide"
LR, SIGMA, DECAY, SEED, GEN0, ADAM_T0 = 0.05, 0.1, 0.99, 11, 5, 3
GRAD_SIZES = (2, 255, 1024, 1025, 2500, 4096)

dev, host, assert_bit_equal = rgo.dev, rgo.host, rgo.assert_bit_equal


def adam_a(t):
    return LR * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.99 ** t)             # optimizers.py:43-47


def plain_handle():
    from ses import HipES
    return HipES(None, 4, 2, True, False)                                    # P = 226


def grad_inputs(n):
    rng = np.random.RandomState(n)
    fits = [rng.randint(0, max(2, n // 2), size=n).astype(np.float32) for _ in range(2)]     # about half the rows tie
    P = 226
    return fits, ((rng.randn(P) * 0.3).astype(np.float32), (rng.randn(P) * 1e-3).astype(np.float32),
                  (rng.rand(P) * 1e-5).astype(np.float32))


def fused_trace(n, wide, final):
    """two consecutive ses_openai_generation calls: [(mu, m, v, theta_next, best)] per generation, on the host"""
    fits, state = grad_inputs(n)
    es = plain_handle()
    try:
        es.set_tuning(KNOB, wide)
        es.set_tuning("es_final_max_chunks", final)
        cur = tuple(dev(x) for x in state)
        sigma, trace = SIGMA, []
        for g, fit in enumerate(fits):
            out = tuple(es.empty(es.P) for _ in range(3))
            best = es.zeros(1)
            theta = es.openai_generation(dev(fit), SEED, GEN0 + g, LR, sigma, adam_a(ADAM_T0 + 1 + g), cur, out,
                                         np.float32(sigma * DECAY), GEN0 + g + 1, 0, n, best=best)
            es.sync()
            trace.append(tuple(host(x).copy() for x in out) + (host(theta).copy(), host(best).copy()))
            cur, sigma = out, sigma * DECAY
        return trace
    finally:
        es.close()


_STEPWISE = {}


def stepwise_trace(n):
    """the same two generations through ses_rank_center + ses_es_update_philox, checked against the host oracle on the way;
    computed once per size and left unchanged"""
    if n in _STEPWISE:
        return _STEPWISE[n]
    fits, state = grad_inputs(n)
    es = plain_handle()
    try:
        mu, m, v = (dev(x) for x in state)
        sigma, trace = SIGMA, []
        for g, fit in enumerate(fits):
            rank, w = es.rank_center(dev(fit))
            es.sync()
            want_rank = snp.stable_rank(fit)
            assert_bit_equal(host(rank), want_rank, f"n = {n}: ses_rank_center rank vs the stable rank")
            assert np.abs(host(w) - snp.centered_ranks(fit, stable=True)).max() <= snp.WEIGHT_ATOL
            grad = es.es_update_philox(w, SEED, GEN0 + g, LR, sigma, adam_a(ADAM_T0 + 1 + g), mu, m, v, want_grad=True)
            es.sync()
            g64, _, tol = snp.es_grad_f64(fit, SEED, GEN0 + g, es.P, LR, sigma)
            err = np.abs(host(grad).astype(np.float64) - g64)
            assert (err <= tol).all(), f"n = {n}: gradient outside the float64 bound, worst {np.max(err / tol):.3g} x tol"
            sigma = sigma * DECAY
            mu_h = host(mu).copy()
            theta = co.perturb(mu_h[None], None, np.float32(sigma), SEED, GEN0 + g + 1, 0, n)
            theta[0] = mu_h
            trace.append((mu_h, host(m).copy(), host(v).copy(), theta, np.array([fit.max()], np.float32)))
        _STEPWISE[n] = trace
        return trace
    finally:
        es.close()


def assert_same_trace(got, want, what):
    for g, (a, b) in enumerate(zip(got, want)):
        for name, x, y in zip(("mu", "m", "v", "theta_next", "best"), a, b):
            assert_bit_equal(x, y, f"{what}, generation {g}: {name}")


@pytest.mark.parametrize("final", [0, 8], ids=["update-launch", "update-in-gradient"])
@pytest.mark.parametrize("n", GRAD_SIZES)
def test_wide_gradient_equals_the_narrow_one_the_stepwise_path_and_the_oracle(n, final):
    want = stepwise_trace(n)
    narrow = fused_trace(n, 0, final)
    wide = fused_trace(n, 1, final)
    assert_same_trace(narrow, want, f"n = {n}: {KNOB} = 0 vs step-wise")
    assert_same_trace(wide, want, f"n = {n}: {KNOB} = 1 vs step-wise")
    assert_same_trace(wide, narrow, f"n = {n}: {KNOB} = 1 vs 0")


# ---- the tail of ses_run_generations on every tie pattern -----------------------------------------------------------------------------
# no-ties: Pendulum-v1 (P = 161), whose reward is a continuous function of the state and of the torque at every step, so that two
# different policies never share a return (CartPole counts steps and the lander's engines stay off below a threshold: both tie),
# every row on resets of its own, so that the returns spread over ~100 units whatever the generation's draw: at a float32 spacing
# of 8e-6 that is n^2 / 2 x 8e-6 / 100, about one pair of 4096 rows rounded to the same float32 (resets shared by all rows can
# land where the 16-step return hardly depends on the policy: a spread of 1.5 units and ~90 rounded pairs).
# half-tied: Pendulum on shared resets, but the rows from n / 2 on of the first population are copies of the parent, like row 0:
# one tie of half the rows, decided by the index, beside distinct values (the second generation's population is the kernel's own
# draw again).
# all-equal: CartPole (P = 226) with sigma = 1e-12, so that every row of both generations is float32(mu + 1e-12 z) = mu.
NETS = dict(rgo.NETS, pendulum=("Pendulum-v1", 3, 1, False, False, {}))
TIES = {"no-ties": dict(net="pendulum", sigma=0.1, shared=False),
        "half-tied": dict(net="pendulum", sigma=0.1, shared=True),
        "all-equal": dict(net="cartpole", sigma=1e-12, shared=True)}
RANK_CASES = [rgo.case(f"{ties}-n{n}-E{E}", rgo.OPENAI, n=n, E=E, T=16, ties=ties, **kw)
              for ties, kw in TIES.items() for n in (2, 257, 4096) for E in (1, 2, 5, 8)]
CONFIGS = (("wide", {KNOB: 1}), ("narrow", {KNOB: 0}), ("unfused", {"fused_episode_mean": 0}))


def handle(net, T, E):
    from ses import HipES
    env, S, A, disc, gru, extra = NETS[net]
    return HipES(env, S, A, disc, gru, max_step=T, eval_ep_num=E, **extra)


@pytest.mark.parametrize("c", RANK_CASES, ids=[c["id"] for c in RANK_CASES])
def test_generations_on_every_tie_pattern_equal_the_oracle_at_both_knob_values(c):
    ref = handle(c["net"], c["T"], c["E"])
    finals, fits = {}, []
    try:
        ref.set_tuning(KNOB, 0)                                  # the oracle's tail: the narrow gradient
        for label, knobs in CONFIGS:
            es = handle(c["net"], c["T"], c["E"])
            try:
                for name, value in knobs.items():
                    es.set_tuning(name, value)
                cc = dict(c, fused=1)
                start = rgo.initial(es, cc, np.random.RandomState(c["n"] + c["E"]))
                if c["ties"] == "half-tied":
                    start[1][c["n"] // 2:] = start[0]
                b = rgo.Batch(es, cc, *start)
                infos = [rgo.check_generation(b, ref, f"{c['id']} {label}") for _ in range(2)]
                finals[label] = b.state()
                if label == "wide":
                    fits = [i["fit"] for i in infos]
            finally:
                es.close()
        for fit in fits:                                         # the oracle's own rank: the stable rule
            rank, _ = ref.rank_center(dev(fit), want_weights=False)
            ref.sync()
            assert_bit_equal(host(rank), snp.stable_rank(fit), f"{c['id']}: rank of the oracle's tail")
    finally:
        ref.close()
    for label, _ in CONFIGS[1:]:
        for name in ("theta", "parents", "fitness", "m", "v"):
            assert_bit_equal(finals["wide"][name], finals[label][name], f"{c['id']}: {name}, wide vs {label}")
    n = c["n"]
    for g, fit in enumerate(fits):
        values, counts = np.unique(fit, return_counts=True)
        share = counts.max() / n
        print(f"{c['id']} generation {g}: {len(values)} distinct fitness values, largest tie {share:.3f} of the rows")
        if c["ties"] == "all-equal":
            assert len(values) == 1, (c["id"], g, len(values))
        elif c["ties"] == "no-ties":
            assert len(values) >= 0.99 * n, (c["id"], g, len(values))
        elif n > 2 and g == 0:
            assert 0.45 <= share <= 0.55 and len(values) >= 0.45 * n, (c["id"], share, len(values))


# ---- the narrow form's shard and granule instances --------------------------------------------------------------------------------
@pytest.mark.parametrize("tuning", ["", "openai_granule_exchange=0"], ids=["granules", "partials_allgather"])
def test_narrow_sharded_tail_on_two_ranks_equals_one_rank_at_the_default(tmp_path, tuning):
    """2048 rows as two shards of one chunk each, five generations through ses_run_generations: k_es_grad_partial_ranked<false, true>
    (peer stores) and <false> with cand_out (all-gather launch), both at es_tail_wide = 0."""
    n = 2048
    script = tmp_path / "sh.py"
    script.write_text(mr.SHARDED_WORKER % (mr.ROOT, mr.SRC))
    mr._run_ranks(script, tmp_path, 1, [str(n), "batched"])
    mr._run_ranks(script, tmp_path, 2, [str(n), "batched"],
                  env={"SES_TUNING": ",".join(filter(None, ["openai_sharded_min_rows=0", KNOB + "=0", tuning]))})
    ref = np.load(tmp_path / f"sh_{n}_w1_r0.npz")
    assert len(ref["best"]) == 5 and np.isfinite(ref["best"]).all()
    for r in range(2):
        got = np.load(tmp_path / f"sh_{n}_w2_r{r}.npz")
        assert bool(got["sharded"]), (r, "the shard form was not available")
        for key in ("elite", "m", "v", "best"):
            assert_bit_equal(got[key], ref[key], f"rank {r}: {key}")
        lo = int(got["first"])
        assert_bit_equal(got["theta"], ref["theta"][lo:lo + got["theta"].shape[0]], f"rank {r}: theta")
        assert tuple(int(x) for x in got["exchanges"]) == ((0, 10) if not tuning else (5, 5)), got["exchanges"]
