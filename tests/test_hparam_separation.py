"""The premise of tests/test_gpu_hparam_anchor.py, checked on the CPU with the fp64 oracle alone: with tests/hparam_anchor.LOUD_REGS,
on every (model, data, k, epochs, rate) that module trains, each of the six pairwise swaps and four "one regulariser = 0" mutants that
the model can feel moves some state array AND some epoch loss by at least 10 x the bar the GPU side is held to there -- so a kernel
or a piece of plumbing with that mutation cannot pass.  A mutant the model cannot feel (its buildModel never names the parameter:
hparam_anchor.USES, written from the reference's sources) must change nothing at all, which pins that table."""
import numpy as np
import pytest

from tests import hparam_anchor as ha
from tests import util
from tests.hostmirror import config, recommender


def test_loud_regs_are_java_floats_pairwise_a_factor_of_two_apart():
    for regs in (ha.LOUD_REGS, ha.SIM_REGS):
        assert len(regs) == 4 and all(x == float(np.float32(x)) for x in regs)
        s = sorted(regs)
        assert all(b >= 2 * a for a, b in zip(s, s[1:]))
        assert len(ha.MUTANTS) == 10 and len({ha.mutate(regs, m) for m in ha.MUTANTS}) == 10
    assert (util.REG, util.REGC, util.LR) == tuple(float(np.float32(x)) for x in (1e-4, 1e-3, 2e-2))    # the other tests' values stay


def _separation(base, other):
    (bl, bs), (ol, os_) = base, other
    state = max(float(np.max(np.abs(bs[n] - os_[n]))) for n in bs)
    loss = max(abs(a - b) / abs(a) for a, b in zip(bl, ol))
    return state, loss


@pytest.mark.parametrize("model,key,k,bars", ha.premise_recipes(), ids=lambda v: str(v) if not isinstance(v, tuple) else "bars")
def test_every_mutant_a_model_can_feel_is_ten_bars_away_and_the_others_change_nothing(model, key, k, bars):
    base = ha.reference(model, key, k)
    assert all(np.isfinite(base[0])) and all(np.isfinite(a).all() for a in base[1].values())
    state_bar, loss_bar = bars
    for m in ha.MUTANTS:
        state, loss = _separation(base, ha.run_oracle(model, key, k, ha.mutate(ha.regs_for(model), m)))
        if ha.applicable(model, m):
            assert state > 0.0 and state >= ha.SEPARATION * state_bar, (ha.mutant_id(m), state, state_bar)
            assert loss > 0.0 and loss >= ha.SEPARATION * loss_bar, (ha.mutant_id(m), loss, loss_bar)
        else:
            assert state == 0.0 and loss == 0.0, (ha.mutant_id(m), state, loss)


def test_every_gpu_case_has_its_premise_checked():
    covered = {(m, key, k) for m, key, k, _ in ha.premise_recipes()}
    assert {(c.model, c.key, c.k) for c in ha.CASES + ha.PLUMBING} == covered
    assert {c.model for c in ha.CASES} == set(ha.USES)


def test_setting_conf_options_reach_their_own_fields(tmp_path):
    """`reg.lambda=0.05 -u 0.03 -i 0.07 -b 0.15 -c 0.31` through the host mirror's parser: each option in its own field, the main value
    in none of them (the C++ host's Conf has no entry point without a GPU: the driver run in the GPU module covers it)."""
    p = tmp_path / "s.conf"
    p.write_text(ha.CONF_LINE + "\n")
    c = recommender.Conf(config.FileConfiger(str(p)))
    assert (c.regU, c.regI, c.regB, c.regC) == ha.LOUD_REGS
    assert c.reg == float(np.float32(0.05)) and c.reg not in ha.LOUD_REGS
    p.write_text("reg.lambda=0.05 -i 0.07\n")                 # an option left out falls back to the main value
    c = recommender.Conf(config.FileConfiger(str(p)))
    assert (c.regU, c.regI, c.regB, c.regC) == (c.reg, ha.LOUD_REGS[1], c.reg, c.reg)


def test_the_setting_conf_recipe_separates_every_mutant_in_the_printed_measures(tmp_path):
    """The config-to-kernel tests of the GPU module compare MAE / RMSE after CONF_ITERS bold-driver epochs of 5-fold CV on DePaulMovie
    at 1e-12: every mutant of the reg.lambda line (CAMF_CU feels all ten) must move both by 10 x that, with the oracle as the engine."""
    from tests.hostmirror import main

    def measures(line, sub):
        (tmp_path / sub).mkdir()
        conf = ha.depaul_conf(tmp_path / sub, ha.CONF_ALGO, line)
        avg, _, _ = main.run(conf, engine_factory=util.OracleEngine, log=lambda *a: None, conf_overrides={"num_iters": ha.CONF_ITERS})
        return avg
    assert ha.conf_line(ha.LOUD_REGS) != ha.CONF_LINE          # (java floats printed in full; same values once parsed:)
    base, same = measures(ha.CONF_LINE, "base"), measures(ha.conf_line(ha.LOUD_REGS), "same")
    assert (base["MAE"], base["RMSE"]) == (same["MAE"], same["RMSE"]) and np.isfinite(base["RMSE"])
    for m in ha.MUTANTS:
        assert ha.applicable("CAMF_CU", m)
        got = measures(ha.conf_line(ha.mutate(ha.LOUD_REGS, m)), ha.mutant_id(m))
        for key in ("MAE", "RMSE"):
            assert abs(got[key] - base[key]) >= ha.SEPARATION * 1e-12, (ha.mutant_id(m), key, got[key], base[key])
