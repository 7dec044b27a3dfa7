"""The launch form of a rollout is decided once, by the rules of csrc/ses_rollout_plan.h; ses_rollout_plan evaluates them without a
device.  Every form computes the same bits, so before this hook only the clock saw a rule move.  The expected values below were
worked out by hand from the rules as they stood inside ses_rollout.hip (default knobs unless said; CartPole MLP: P = 226): they
pin the project's measured crossovers, and the population sizes sit on both sides of each."""
import pytest

from ses import _lib
from ses._lib import (GRU_FORM_EPISODE_PARALLEL, GRU_FORM_LOCKSTEP, GRU_FORM_LOCKSTEP_MULTI2, GRU_FORM_LOCKSTEP_MULTI4, GRU_FORM_MFMA,
                      GRU_FORM_MFMA4, GRU_FORM_SEQUENTIAL, MODE_EPISODIC, MODE_FIXED_LENGTH, PLAN_BOX2D_MLP, PLAN_CARTPOLE_MLP_F64,
                      PLAN_CARTPOLE_MLP_MIX, PLAN_CARTPOLE_MLP_PAIR, PLAN_CARTPOLE_MLP_PURE, PLAN_GRU, PLAN_OTHER, SesConfig, SesError)

EPISODIC, FIXED = MODE_EPISODIC, MODE_FIXED_LENGTH


def cartpole(E, gru=0, lanes_per_env=0, physics64=0):
    return SesConfig(_lib.ENV_CARTPOLE, 4, 2, 1, gru, 0, 500, E, 0, lanes_per_env, 1, physics64)


def lander(E, gru=0, discrete=0):
    return SesConfig(_lib.ENV_LUNARLANDER, 8, 4, discrete, gru, 0, 300, E, 0, 0, 1, 0)


def walker(E):
    return SesConfig(_lib.ENV_BIPEDALWALKER, 24, 4, 0, 0, 0, 1600, E, 0, 0, 1, 0)


def plan(cfg, n_rows, mode=EPISODIC, **knobs):
    return _lib.rollout_plan(cfg, n_rows, mode, **knobs)


def pure(p):
    assert p.family == PLAN_CARTPOLE_MLP_PURE and p.lanes_light == 0 and p.waves_light == 0 and p.waves_rest == 0
    return p.lanes_rest


def split(p):
    assert p.family in (PLAN_CARTPOLE_MLP_MIX, PLAN_CARTPOLE_MLP_PAIR)
    return p.lanes_light, p.lanes_rest


@pytest.mark.parametrize("mode", [EPISODIC, FIXED])
@pytest.mark.parametrize("n_rows, E, lanes, packed", [
    (96, 5, 16, 1),             # 480 envs: 120 lone waves
    (512, 5, 16, 1),            # 2560 envs
    (1024, 5, 8, 1),            # 5120 envs: 640 waves, within one per SIMD
    (3072, 5, 8, 0),            # 15 360 envs: 1920 waves, two on most SIMDs
    (16384, 1, 8, 0),
    (5120, 5, 4, 0),            # 25 600 envs
    (49153, 1, 4, 0),           # past the cost model: 4 lanes per env
])
def test_cartpole_mlp_pure_splits(n_rows, E, lanes, packed, mode):
    p = plan(cartpole(E), n_rows, mode)
    assert pure(p) == lanes and p.packed == packed and p.block == 64 and not p.own_rows_ok


def test_cartpole_mlp_8_16_mix():
    for mode in (EPISODIC, FIXED):
        p = plan(cartpole(5), 2048, mode)                                   # 10 240 envs
        assert p.family == PLAN_CARTPOLE_MLP_MIX and split(p) == (8, 16)
        assert (p.waves_light, p.waves_rest) == (1024, 512) and not p.own_rows_ok


def test_cartpole_mlp_pair_from_16385_envs():
    p = plan(cartpole(1), 16385, FIXED)
    assert p.family == PLAN_CARTPOLE_MLP_PAIR and split(p) == (16, 4)
    assert (p.waves_light, p.waves_rest) == (1024, 769) and p.heavy_packed == 1 and p.handover == 1 << 30
    assert not p.own_rows_ok                                                # 80 rows of 226 floats exceed 56 KiB
    p = plan(cartpole(2), 9001, FIXED)
    assert p.family == PLAN_CARTPOLE_MLP_PAIR and p.own_rows_ok            # 42 rows


def test_cartpole_mlp_pair_at_the_benchmark_population():
    p = plan(cartpole(5), 4096, FIXED)                                      # 20 480 envs
    assert p.family == PLAN_CARTPOLE_MLP_PAIR and split(p) == (16, 4)
    assert (p.waves_light, p.waves_rest) == (1024, 1024) and p.own_rows_ok and p.heavy_packed == 1
    p = plan(cartpole(5), 4096, EPISODIC)
    assert p.family == PLAN_CARTPOLE_MLP_MIX and split(p) == (16, 4) and (p.waves_light, p.waves_rest) == (1024, 1024)
    assert not p.own_rows_ok
    p = plan(cartpole(5), 4096, FIXED, fused_perturb_rollout=0)
    assert p.family == PLAN_CARTPOLE_MLP_PAIR and not p.own_rows_ok
    p = plan(cartpole(5), 4096, FIXED, rollout_heavy_prio_steps=0)          # (the hand-over stays off: nothing left of the pair)
    assert p.family == PLAN_CARTPOLE_MLP_MIX and split(p) == (16, 4) and not p.own_rows_ok
    p = plan(cartpole(5), 4096, FIXED, rollout_heavy_packed=0)
    assert p.family == PLAN_CARTPOLE_MLP_PAIR and p.heavy_packed == 0
    p = plan(cartpole(1), 20481, FIXED)                                     # a second heavy wave somewhere: its cost is 1252.4
    assert (p.lanes_light, p.lanes_rest) != (16, 4)


def test_cartpole_mlp_overrides():
    assert pure(plan(cartpole(5, lanes_per_env=2), 96)) == 2
    p = plan(cartpole(5), 96, rollout_block=256)
    assert pure(p) == 16 and p.block == 256 and not p.packed
    assert not plan(cartpole(5), 96, rollout_packed=0).packed
    p = plan(cartpole(5), 3072, rollout_packed=1)
    assert pure(p) == 8 and p.packed


def test_cartpole_mlp_float64_dynamics():
    for n_rows, lanes in ((10239, 8), (10240, 4)):
        p = plan(cartpole(1, physics64=1), n_rows)
        assert p.family == PLAN_CARTPOLE_MLP_F64 and p.lanes_rest == lanes and not p.own_rows_ok


@pytest.mark.parametrize("n_rows, E, want_cartpole, want_lander", [
    (97, 5, GRU_FORM_EPISODE_PARALLEL, GRU_FORM_EPISODE_PARALLEL),
    (97, 1, GRU_FORM_LOCKSTEP, GRU_FORM_LOCKSTEP),
    (4096, 5, GRU_FORM_LOCKSTEP, GRU_FORM_LOCKSTEP_MULTI4),
    (1536, 5, None, GRU_FORM_LOCKSTEP_MULTI2),
    (1535, 5, None, GRU_FORM_LOCKSTEP),
    (4096, 7, GRU_FORM_MFMA4, GRU_FORM_LOCKSTEP_MULTI4),
    (4096, 9, GRU_FORM_LOCKSTEP, GRU_FORM_LOCKSTEP),                       # (lander: E > 8, one offspring per wave)
    (4096, 12, GRU_FORM_MFMA, GRU_FORM_MFMA),
])
def test_gru_forms(n_rows, E, want_cartpole, want_lander):
    cases = [(lander(E, gru=1), want_lander), (lander(E, gru=1, discrete=1), want_lander)]
    if want_cartpole is not None:
        cases.append((cartpole(E, gru=1), want_cartpole))
    for cfg, want in cases:
        p = plan(cfg, n_rows)
        assert p.family == PLAN_GRU and p.gru_form == want
        p = plan(cfg, n_rows, gru_sequential=1)
        assert p.family == PLAN_GRU and p.gru_form == GRU_FORM_SEQUENTIAL


def test_box2d_mlp_wave_shapes():
    def shape(cfg, n_rows, **knobs):
        p = plan(cfg, n_rows, **knobs)
        assert p.family == PLAN_BOX2D_MLP
        return p.box2d_lpe, p.box2d_epw
    assert shape(walker(5), 4096) == (2, 20)
    for discrete in (0, 1):
        assert shape(lander(5, discrete=discrete), 120) == (64, 1)
        assert shape(lander(5, discrete=discrete), 4096) == (4, 10)
        assert shape(lander(5, discrete=discrete), 4096, box2d_lanes_per_env=8) == (8, 8)
        assert shape(lander(5, discrete=discrete), 4096, box2d_lanes_per_env=8, box2d_envs_per_wave=16) == (8, 8)


def test_the_other_envs_are_left_to_their_units():
    for cfg in (SesConfig(_lib.ENV_PENDULUM, 3, 1, 0, 0, 0, 200, 5, 0, 0, 1, 0),
                SesConfig(_lib.ENV_SIMPLE_SPREAD, 12, 5, 1, 0, 0, 25, 5, 0, 0, 2, 0),
                SesConfig(_lib.ENV_WATERWORLD, 242, 2, 0, 0, 0, 500, 5, 0, 0, 5, 0),
                SesConfig(_lib.ENV_PURSUIT, 147, 5, 1, 0, 0, 500, 5, 0, 0, 8, 0)):
        p = plan(cfg, 4096)
        assert p.family == PLAN_OTHER
        assert all(getattr(p, name) == 0 for name, _ in p._fields_)


def test_refusals_need_no_device():
    with pytest.raises(SesError, match="ses_rollout_plan: CartPole needs num_state=4, got 5"):
        plan(SesConfig(_lib.ENV_CARTPOLE, 5, 2, 1, 0, 0, 500, 5, 0, 0, 1, 0), 96)
    with pytest.raises(SesError, match="ses_rollout_plan: BipedalWalker needs gru=0"):
        plan(SesConfig(_lib.ENV_BIPEDALWALKER, 24, 4, 0, 1, 0, 1600, 5, 0, 0, 1, 0), 96)
    with pytest.raises(SesError, match="SES_ENV_NONE is no env"):
        plan(SesConfig(_lib.ENV_NONE, 4, 2, 1, 0, 0, 500, 5, 0, 0, 1, 0), 96)
    with pytest.raises(SesError, match="n_rows must be >= 1"):
        plan(cartpole(5), 0)
    with pytest.raises(SesError, match="bad mode 2"):
        plan(cartpole(5), 96, 2)
    with pytest.raises(SesError, match="lanes_per_env must be"):
        plan(cartpole(5, lanes_per_env=3), 96)
