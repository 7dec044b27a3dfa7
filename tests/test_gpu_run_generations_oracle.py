"""ses_run_generations (the product loop, csrc/ses_generations.hip) against a host oracle, one generation at a time, on every
tail path a single GPU takes.

Each case builds a ses_gen_state the way _GenerationBatch does on one GPU, runs k = 1 per call, reads back what the call
left (fitness, best, parents / theta / Adam moments of the next generation, alias_state, work_i32 = [rank | elite ids |
parent indices | alias flags], the host scalars) and compares it with an oracle built from that generation's inputs:
  * resets: co.init_states_uniform(env seed, generation key);
  * per-episode returns: a separate ses_rollout(want_episodes) of the current population on those resets (itself bit-exact
    against the C oracle; for CartPole at small n also co.rollout_cartpole here);
  * fitness = float32(sequential float64 sum over episodes / E), rank by the stable rule, best = max: bit-exact;
  * openai_es: ses_openai_generation on a second handle given the oracle fitness and the same state and keys -- the unfused
    tail, held to float64 by test_gpu_es_tail_f64.py -- must equal the batched call bit for bit;
  * simple_evolution / simple_genetic: elites = rows `ids` of co.perturb(parents, parent map, pop_sigma, gen), the in-place
    float32 elite sum with the alias rule, the next population co.perturb(..., gen + 1): bit-exact.
Every case runs with the tail's fused knob ("fused_episode_mean" / "fused_elite_tail") at 1 and at 0: both must equal the
oracle.  The sizes straddle where the launch shapes change: the counting rank's slice length jt (64 -> 128 between 5837 and
5838), the counting rank -> tile sort at 8193 rows, the single-workgroup elite tail at 512 rows.  Beyond single generations:
one k = 8 call equals eight k = 1 calls, and the per-generation reset fallback above 64 MB (k = 13 at 65 536 rows with own
resets) equals 13 single calls.
"""
import math

import numpy as np
import pytest
import torch

from oracle import c_oracle as co
from oracle import strategies_np as snp

pytestmark = pytest.mark.gpu

OPENAI, EVOLUTION, GENETIC = 0, 1, 2              # SES_STRATEGY_*
KNOB = {OPENAI: "fused_episode_mean", EVOLUTION: "fused_elite_tail", GENETIC: "fused_elite_tail"}
LR = 0.05
# name -> (env, S, A, discrete, gru, extra HipES arguments); P in the comment
NETS = {"cartpole": ("CartPole-v1", 4, 2, True, False, {}),                         # 226
        "cartpole_gru": ("CartPole-v1", 4, 2, True, True, {}),                      # 6562
        "lander": ("LunarLanderContinuous-v2", 8, 4, False, False, {}),             # 420 = 0 mod 4
        "spread3": ("simple_spread", 18, 5, True, False, {"n_agents": 3}),          # 773 = 1 mod 4
        "mountaincar": ("MountainCar-v0", 2, 3, True, False, {}),                   # 195 = 3 mod 4
        "acrobot": ("Acrobot-v1", 6, 3, True, False, {})}                           # 323
# hand-built first hidden unit (w1 row 0) for policies whose random perturbations give spread-out returns: CartPole balances on
# (theta, dtheta) and drifts, Acrobot pumps along dtheta2, MountainCar pushes along the velocity
FEATURES = {"cartpole": [0.0, 0.0, 0.3, 1.0], "acrobot": [0, 0, 0, 0, 0, 8.0], "mountaincar": [0.0, 2000.0]}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_bit_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {bad.sum()} of {bad.size} elements differ, first at {at}: {got[at]!r} vs {want[at]!r}")


def handle(net, T, E):
    from ses import HipES
    env, S, A, disc, gru, extra = NETS[net]
    return HipES(env, S, A, disc, gru, max_step=T, eval_ep_num=E, **extra)


def feature_policy(net, P, S, A):
    """w1 row 0 = FEATURES[net], action A-1 (and 0 against it when A = 3) follows the sign of that hidden unit"""
    th = np.zeros(P, np.float32)
    th[:S] = FEATURES[net]
    w2 = 32 * S + 32
    th[w2 + (A - 1) * 32] = 1.0
    if A == 3:
        th[w2] = -1.0
    return th


def parent_map(kind, n, ke):
    """the strategies' constant maps (offspring_strategies.py _gen_offsprings): < 0 = parent -1 - idx verbatim"""
    idx = np.zeros(n, np.int32)
    if kind == OPENAI:
        idx[0] = -1
    elif kind == EVOLUTION:
        idx[0] = idx[1] = -1
    else:
        per = n // ke
        for e in range(ke):
            idx[e * per] = -1 - e
            idx[e * per + 1:(e + 1) * per] = e
    return idx


class Batch:
    """One ses_gen_state on one GPU, laid out like _GenerationBatch.__init__ (learning_strategies/evolution/loop.py)."""

    def __init__(self, es, c, parents0, theta0, m0=None, v0=None, adam_t=0):
        from ses import _lib
        self.es, self.c = es, c
        kind, n, ke, P = c["kind"], c["n"], c["ke"], es.P
        st = self.st = _lib.SesGenState()
        st.strategy, st.n, st.mode = kind, n, c["mode"]
        st.elite_num = ke if kind != OPENAI else 0
        st.shared_init, st.init_width = int(c["shared"]), es.init_dim
        st.init_lo, st.init_hi = es.init_range
        st.seed, st.env_seed = c["seed"], c["env_seed"]
        st.learning_rate, st.sigma_decay = LR, c["decay"]
        st.sigma = st.pop_sigma = c["sigma"]
        st.pop_gen, st.adam_t, st.cur = c["gen0"], adam_t, 0
        keep = self.keep = {"theta": [dev(theta0), es.empty(n, P)], "parents": [dev(parents0), es.empty(*parents0.shape)]}
        if kind == OPENAI:
            keep["m"], keep["v"] = [dev(m0), es.empty(P)], [dev(v0), es.empty(P)]
        else:
            self.map = parent_map(kind, n, ke)
            keep["map"] = dev(self.map)
            keep["wi"] = es.zeros(n + 3 * ke, dtype=torch.int32)      # (zeros: the parts a path leaves alone compare equal)
            keep["wf"] = es.zeros(ke, P)
            st.parent_map, st.work_i32, st.work_f32 = keep["map"].data_ptr(), keep["wi"].data_ptr(), keep["wf"].data_ptr()
            if kind == EVOLUTION:
                keep["alias"] = dev(np.ones(1, np.int32))                # every slot starts as the same module object
                st.alias_state = keep["alias"].data_ptr()
        keep["fitness"] = es.zeros(n)
        keep["init"] = es.zeros(1 if c["shared"] else n, es.E, es.init_dim)
        st.fitness, st.init = keep["fitness"].data_ptr(), keep["init"].data_ptr()
        for i in (0, 1):
            st.theta[i], st.parents[i] = keep["theta"][i].data_ptr(), keep["parents"][i].data_ptr()
            if kind == OPENAI:
                st.adam_m[i], st.adam_v[i] = keep["m"][i].data_ptr(), keep["v"][i].data_ptr()

    def run(self, k):
        best = self.es.empty(k)
        best.fill_(float("nan"))
        self.es.run_generations(self.st, k, best)
        self.es.sync()
        return host(best)

    def state(self):
        """host copies of the current generation's buffers and the host scalars"""
        st, keep, cur = self.st, self.keep, self.st.cur
        s = {"theta": host(keep["theta"][cur]), "parents": host(keep["parents"][cur]), "fitness": host(keep["fitness"]),
             "sigma": st.sigma, "pop_sigma": st.pop_sigma, "pop_gen": int(st.pop_gen),
             "adam_t": int(st.adam_t)}
        for name in ("m", "v", "alias", "wi", "wf"):
            if name in keep:
                s[name] = host(keep[name][cur] if name in ("m", "v") else keep[name])
        return s


def initial(es, c, rng):
    """(parents0, theta0, m0, v0, adam_t): a current population drawn from its parents as the strategies draw it"""
    kind, n, ke, P = c["kind"], c["n"], c["ke"], es.P
    if c.get("mu") == "feature":
        mu = feature_policy(c["net"], P, es.S, es.A) + (rng.randn(P) * 0.01).astype(np.float32)
    elif c.get("mu") == "feature_exact":
        mu = feature_policy(c["net"], P, es.S, es.A)
    else:
        mu = (rng.randn(P) * 0.3).astype(np.float32)
    parents = (rng.randn(ke, P) * 0.3).astype(np.float32) if kind == GENETIC else mu[None]
    theta = co.perturb(parents, parent_map(kind, n, ke), np.float32(c["sigma"]), c["seed"], c["gen0"], 0, n)
    if kind != OPENAI:
        return parents, theta, None, None, 0
    m = (rng.randn(P) * 1e-3).astype(np.float32)
    v = (rng.rand(P) * 1e-5).astype(np.float32)
    return parents[0].copy(), theta, m, v, 3


def oracle_returns(ref, c, theta, gen):
    """the generation's resets and per-episode returns: float32 resets, float64[n, E] returns"""
    lo, hi = ref.init_range
    init = co.init_states_uniform(c["env_seed"], gen, 0, 1 if c["shared"] else c["n"], ref.E, ref.init_dim, c["shared"], lo, hi)
    if c["shared"]:
        init = init[0]
    fit, ep, _ = ref.rollout(dev(theta), dev(init), mode=c["mode"], want_episodes=True)
    fit, ep = host(fit), host(ep)
    if c["net"] in ("cartpole", "cartpole_gru") and c["n"] * ref.E <= 1024:
        _, ep_c, _ = co.rollout_cartpole(theta, init, ref.E, ref.max_step, gru=ref.gru, mode=c["mode"])
        assert_bit_equal(ep, ep_c, "ses_rollout per-episode returns vs the C oracle")
    want = snp.episode_fitness(ep)
    assert_bit_equal(fit, want, "ses_rollout fitness vs the sequential float64 episode mean")
    return init, want


def check_generation(b, ref, note):
    """one k = 1 call of the batched loop against the oracle of that generation; returns what the oracle saw"""
    c, es = b.c, b.es
    kind, n, ke, P = c["kind"], c["n"], c["ke"], es.P
    s0 = b.state()
    gen, sigma, pop_sigma = s0["pop_gen"], s0["sigma"], s0["pop_sigma"]
    what = f"{note} gen {gen}"
    _, fit = oracle_returns(ref, c, s0["theta"], gen)
    best = b.run(1)
    s1 = b.state()
    assert_bit_equal(s1["fitness"], fit, f"{what}: fitness")
    assert_bit_equal(best[:1], fit.max(keepdims=True), f"{what}: best")
    assert s1["pop_gen"] == gen + 1, (what, s1["pop_gen"])
    info = {"fit": fit}
    if kind == OPENAI:
        t = s0["adam_t"] + 1
        a = LR * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.99 ** t)               # optimizers.py:43-47, as the C loop forms it
        nxt_sigma = sigma * c["decay"]
        out = (ref.empty(P), ref.empty(P), ref.empty(P))
        rbest = ref.zeros(1)
        theta = ref.openai_generation(dev(fit), c["seed"], gen, LR, sigma, a, (dev(s0["parents"]), dev(s0["m"]), dev(s0["v"])),
                                      out, np.float32(nxt_sigma), gen + 1, 0, n, best=rbest)
        ref.sync()
        for name, got, want in (("mu", s1["parents"], out[0]), ("m", s1["m"], out[1]), ("v", s1["v"], out[2]),
                                ("theta_next", s1["theta"], theta), ("best (unfused tail)", best[:1], rbest)):
            assert_bit_equal(got, host(want), f"{what}: {name} vs ses_openai_generation on the oracle fitness")
        if n <= 8193:
            want = co.perturb(s1["parents"][None], None, np.float32(nxt_sigma), c["seed"], gen + 1, 0, n)
            want[0] = s1["parents"]
            assert_bit_equal(s1["theta"], want, f"{what}: theta_next vs the C oracle's perturbation of the new mu")
        assert (s1["sigma"], s1["pop_sigma"], s1["adam_t"]) == (nxt_sigma, nxt_sigma, t), what
        return info
    pop = co.perturb(s0["parents"], b.map, np.float32(pop_sigma), c["seed"], gen, 0, n)
    assert_bit_equal(s0["theta"], pop, f"{what}: current population vs co.perturb(parents, map)")
    rank = snp.stable_rank(fit)
    evo = kind == EVOLUTION
    ids, pidx, alias, state = snp.elite_select(rank, ke, b.map, int(s0["alias"][0]) if evo else None)
    wi = s1["wi"]
    assert_bit_equal(wi[:n], rank, f"{what}: rank")
    assert_bit_equal(wi[n:n + ke], ids, f"{what}: elite ids")
    assert_bit_equal(wi[n + ke:n + 2 * ke], pidx, f"{what}: elite parent indices")
    rows = pop[ids]
    if evo:
        assert_bit_equal(wi[n + 2 * ke:n + 3 * ke], alias, f"{what}: alias flags")
        assert int(s1["alias"][0]) == state, (what, "alias_state", int(s1["alias"][0]), state)
        if not c["fused"] or n > 512:                               # the generic tail materialises the elite rows
            assert_bit_equal(s1["wf"], rows, f"{what}: elite rows")
        parents = snp.elite_mean(rows, alias)[None]
        info["alias_effect"] = not np.array_equal(bits(parents[0]), bits(snp.elite_mean(rows)))
        nxt_sigma = new_pop_sigma = sigma * c["decay"]              # sigma decays BEFORE the next population is drawn
    else:
        parents = rows
        nxt_sigma, new_pop_sigma = sigma * c["decay"], sigma        # ... and AFTER it for simple_genetic
    assert_bit_equal(s1["parents"], parents, f"{what}: next parents")
    want = co.perturb(parents, b.map, np.float32(new_pop_sigma), c["seed"], gen + 1, 0, n)
    assert_bit_equal(s1["theta"], want, f"{what}: next population")
    assert (s1["sigma"], s1["pop_sigma"]) == (nxt_sigma, new_pop_sigma), what
    info.update(ids=ids, alias=alias)
    return info


def run_case(c, gens=2):
    """the case with its fused knob at 1 and at 0: each generation equals the oracle; both runs end in the same bits"""
    ref = handle(c["net"], c["T"], c["E"])
    finals, infos = {}, {}
    try:
        for fused in (1, 0):
            es = handle(c["net"], c["T"], c["E"])
            try:
                es.set_tuning(KNOB[c["kind"]], fused)
                cc = dict(c, fused=fused)
                b = Batch(es, cc, *initial(es, cc, np.random.RandomState(c["n"] + 7 * c["ke"])))
                infos[fused] = [check_generation(b, ref, f"{c['id']} {KNOB[c['kind']]}={fused}") for _ in range(gens)]
                finals[fused] = b.state()
            finally:
                es.close()
    finally:
        ref.close()
    for name in ("theta", "parents", "fitness", "m", "v", "alias", "wi"):
        if name in finals[1]:
            assert_bit_equal(finals[1][name], finals[0][name], f"{c['id']}: {name}, fused vs unfused")
    return infos


def case(cid, kind, net, n, ke=0, E=1, T=60, shared=True, mode=0, sigma=0.1, decay=0.99, seed=11, env_seed=3, gen0=5, **kw):
    return dict(id=cid, kind=kind, net=net, n=n, ke=ke, E=E, T=T, shared=shared, mode=mode, sigma=sigma, decay=decay,
                seed=seed, env_seed=env_seed, gen0=gen0, **kw)


# ---- openai_es -----------------------------------------------------------------------------------------------------------------
OPENAI_CASES = [
    case("n2", OPENAI, "cartpole", 2, E=1),
    case("n3-E8", OPENAI, "cartpole", 3, E=8, shared=False),
    case("n131-E5", OPENAI, "cartpole", 131, E=5, T=100),
    case("n4096-E5-fixed-headline", OPENAI, "cartpole", 4096, E=5, T=500, mode=1, sigma=0.3, mu="feature"),
    case("n5837-jt64", OPENAI, "cartpole", 5837, E=1, T=40, shared=False),
    case("n5838-jt128-E8", OPENAI, "cartpole", 5838, E=8, T=30),
    case("n8192-E5", OPENAI, "cartpole", 8192, E=5, T=30, shared=False),
    case("n8193-sort", OPENAI, "cartpole", 8193, E=1, T=40),
    case("n3000-ties-at-cap", OPENAI, "cartpole", 3000, E=1, T=10, sigma=0.05, ties=True),
    case("lander-P420", OPENAI, "lander", 150, E=2, T=40),
    case("spread3-P773", OPENAI, "spread3", 233, E=3, T=25),
    case("mountaincar-P195", OPENAI, "mountaincar", 300, E=2, T=180, mu="feature", sigma=0.3, shared=False),
]


@pytest.mark.parametrize("c", OPENAI_CASES, ids=[c["id"] for c in OPENAI_CASES])
def test_openai_generations_equal_the_oracle(c):
    infos = run_case(c)
    fit = infos[1][0]["fit"]
    assert len(np.unique(fit)) > 1 or c["n"] == 2, "the returns should not all tie"
    if c.get("ties"):                                                # most rows end at the step cap: the tie rule decides
        assert (fit == c["T"]).mean() > 0.4, (fit == c["T"]).mean()


# ---- simple_evolution: n = offspring + 1, elite_num in {1, 10, min(n, 1024)} ---------------------------------------------------------
EVO_CASES = []
for i, off in enumerate((1, 96, 256, 511, 512, 1024)):
    n = off + 1
    for j, ke in enumerate(sorted({1, min(10, n), min(n, 1024)})):
        net = ("cartpole", "acrobot", "cartpole_gru")[(i + j) % 3]
        kw = dict(mu="feature", T=120, sigma=0.2) if net != "cartpole_gru" else dict(T=30, sigma=0.1)
        if net == "acrobot":
            kw.update(T=150)
        EVO_CASES.append(case(f"{net}-n{n}-k{ke}", EVOLUTION, net, n, ke=ke, E=2 if i % 2 else 1, shared=(i + j) % 2 == 0, **kw))
# slots 0 and 1 (mu and elite 0, one module object in the reference) among the elites in consecutive generations with a child
# between them, so the alias flag changes the mean: seeds found with the C oracle, own resets, E = 1, from generation 0
ALIAS_CASES = [case("alias-k97", EVOLUTION, "cartpole", 97, ke=97, T=500, shared=False, sigma=0.3, decay=1.0, seed=9, env_seed=0,
                    gen0=0, mu="feature_exact"),
               case("alias-k10", EVOLUTION, "cartpole", 97, ke=10, T=500, shared=False, sigma=3.0, decay=1.0, seed=0, env_seed=0,
                    gen0=0, mu="feature_exact")]


@pytest.mark.parametrize("c", EVO_CASES, ids=[c["id"] for c in EVO_CASES])
def test_simple_evolution_generations_equal_the_oracle(c):
    run_case(c)


@pytest.mark.parametrize("c", ALIAS_CASES, ids=[c["id"] for c in ALIAS_CASES])
def test_simple_evolution_alias_quirk_in_consecutive_generations(c):
    infos = run_case(c, gens=2)
    for fused in (1, 0):
        for g, info in enumerate(infos[fused]):
            assert info["ids"][0] in (0, 1) and info["alias"].any() and info["alias_effect"], \
                (c["id"], fused, g, info["ids"][:4], "the arrangement this case exists for did not happen")


# ---- simple_genetic: n = k * (offspring / k) on both sides of 512 --------------------------------------------------------------------
GEN_CASES = []
for off in (500, 530):
    for j, ke in enumerate((1, 4, 16)):
        net = "cartpole_gru" if (off, ke) == (530, 4) else "cartpole"
        GEN_CASES.append(case(f"{net}-off{off}-k{ke}", GENETIC, net, ke * (off // ke), ke=ke, E=1 + j, T=60, shared=j != 1,
                              sigma=0.2))


@pytest.mark.parametrize("c", GEN_CASES, ids=[c["id"] for c in GEN_CASES])
def test_simple_genetic_generations_equal_the_oracle(c):
    run_case(c)


# ---- chunking: one k = 8 call == eight k = 1 calls ----------------------------------------------------------------------------------
CHUNK_CASES = [case("openai-n131", OPENAI, "cartpole", 131, E=5, T=60),
               case("evolution-n97", EVOLUTION, "cartpole", 97, ke=10, E=2, T=120, shared=False, mu="feature", sigma=0.2),
               case("genetic-n100", GENETIC, "cartpole", 100, ke=4, E=1, T=60)]


def _same_state(a, b, what):
    for name in a:
        if isinstance(a[name], np.ndarray):
            assert_bit_equal(b[name], a[name], f"{what}: {name}")
        else:
            assert a[name] == b[name], (what, name, a[name], b[name])


@pytest.mark.parametrize("c", CHUNK_CASES, ids=[c["id"] for c in CHUNK_CASES])
def test_one_call_of_eight_generations_equals_eight_calls(c):
    ref = handle(c["net"], c["T"], c["E"])
    es1, es8 = handle(c["net"], c["T"], c["E"]), handle(c["net"], c["T"], c["E"])
    try:
        cc = dict(c, fused=1)
        start = initial(es1, cc, np.random.RandomState(5))
        b1, b8 = Batch(es1, cc, *start), Batch(es8, cc, *start)
        best1 = [float(check_generation(b1, ref, f"{c['id']} single")["fit"].max()) for _ in range(8)]
        best8 = b8.run(8)
        assert_bit_equal(best8, np.array(best1, np.float32), f"{c['id']}: best per generation")
        _same_state(b1.state(), b8.state(), c["id"])
    finally:
        for h in (es1, es8, ref):
            h.close()


def test_resets_drawn_per_generation_above_64_mb_equal_the_batched_draw():
    """own resets of 65 536 rows x 5 episodes x 4 floats: k = 1 draws them with ses_init_states_uniform_gens into the handle's
    buffer, k = 13 (68 MB) one generation at a time into the caller's st->init -- which then holds the last generation's"""
    c = case("fallback-n65536", OPENAI, "cartpole", 65536, E=5, T=40, shared=False, fused=1)
    ref = handle("cartpole", c["T"], c["E"])
    es1, es13 = handle("cartpole", c["T"], c["E"]), handle("cartpole", c["T"], c["E"])
    try:
        start = initial(es1, c, np.random.RandomState(3))
        b1, b13 = Batch(es1, c, *start), Batch(es13, c, *start)
        fit = check_generation(b1, ref, "fallback single")["fit"]
        assert len(np.unique(fit)) > 5, "the returns must depend on the resets"
        best1 = [float(fit.max())]
        best1 += [float(b1.run(1)[0]) for _ in range(12)]
        best13 = b13.run(13)
        assert_bit_equal(best13, np.array(best1, np.float32), "best per generation")
        s1, s13 = b1.state(), b13.state()
        lo, hi = es13.init_range
        want = co.init_states_uniform(c["env_seed"], c["gen0"] + 12, 0, c["n"], c["E"], es13.init_dim, False, lo, hi)
        assert_bit_equal(host(b13.keep["init"]), want, "st->init after the per-generation fallback")
        _same_state(s1, s13, "k = 13 vs 13 x k = 1")
    finally:
        for h in (es1, es13, ref):
            h.close()
