"""tests/eval_anchor.py on the CPU: its predict and evalRatings restatements against the C oracle, the Python restatement and the
reference's own source run at non-unit rating scales; the rounding premise of every case tests/test_gpu_eval_anchor.py runs; and the proof
that the data can see the defects that module is there to catch -- each reference mutant moves a measure (or, for the prediction
mutants, a prediction) by at least 10 x the bar the GPU side is held to."""
import gzip
import json
import os

import numpy as np
import pytest

from oracle import oracle_c, oracle_np
from tests import eval_anchor as ea
from tests import test_reference_src_golden as src

SEPARATION = 10.0
GOLD = json.loads(gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_evalratings_scales.json.gz")).read())["cases"]
CPU_CASES = [c for c in ea.SWEEP_CASES if c.model in ea.MF_MODELS and c.k in (1, 65) and not c.f64]


def scale_id(s):
    return "%g-%g" % s


def _oracles(p):
    """(C oracle, Python restatement) over the case's state as float64"""
    c = p.case
    st = {n: np.array(a, dtype=np.float64) for n, a in p.state.items()}
    ctx = np.zeros(len(p.u), np.int32) if c.model in ea.TWO_D else p.ctx

    def make(gm):
        orc = oracle_c.Oracle(c.model, c.k, ea.N_USERS, ea.N_ITEMS, ea.N_CONDS, p.u, p.j, ctx, p.ratings[ea.SCALES[0]], ea.CTX_PTR,
                              ea.CTX_CONDS, {n: a.copy() for n, a in st.items()}, gm, 0.0, 0.0, 0.0, 0.0)
        m = oracle_np.MODELS[c.model](c.k, ea.N_USERS, ea.N_ITEMS, ea.N_CONDS, [list(x) for x in ea.CTX_LISTS], gm, 0.0, 0.0, 0.0, 0.0)
        for n, a in st.items():
            setattr(m, n, a.tolist())
        return orc, m
    return make, ctx


@pytest.mark.parametrize("case", CPU_CASES, ids=ea.case_id)
def test_restatement_agrees_with_both_oracles_on_every_scale(case):
    """predictions within the per-tuple bar (the oracles add in the reference's order), counts equal, measures within their bars"""
    p = ea.problem(case)
    make, ctx = _oracles(p)
    for s in ea.SCALES:
        orc, m = make(p.gm[s])
        ev, bars = p.evals[s], ea.measure_bars(p.evals[s], p.bar[s], *s)
        res, preds = orc.eval_ratings(p.u, p.j, ctx, p.ratings[s], *s, want_preds=True)
        want = np.clip(p.pred[s], *s)
        raw = np.array([orc.predict(int(a), int(b), int(c)) for a, b, c in zip(p.u, p.j, ctx)])
        assert np.all(np.abs(raw - p.pred[s]) <= p.bar[s])
        assert preds is not None and np.all(np.abs(preds - want) <= p.bar[s]) and np.ptp(preds) > 0
        res2 = oracle_np.eval_ratings(m, list(zip(p.u.tolist(), p.j.tolist(), ctx.tolist(), p.ratings[s].tolist())), *s)
        for got in (res, res2):
            assert got["n"] == ev.n == case.n
            for name in ea.MEASURES:
                assert abs(got[name] - ev.measures[name]) <= bars[name], (s, name, got[name], ev.measures[name], bars[name])


def test_every_gpu_case_meets_the_rounding_premise():
    """no reference prediction within 1e3 bars of a rounding boundary (q + 0.5) * minRate: both sides round every tuple the same way"""
    worst = np.inf
    for case in ea.ALL_CASES:
        p = ea.problem(case)            # asserts the premise as it builds
        for s in ea.SCALES:
            assert p.evals[s].n == case.n and np.isfinite(list(p.evals[s].measures.values())).all()
            worst = min(worst, ea.rounding_margin(p.evals[s], p.bar[s], s[0]))
    print("smallest distance to a rounding boundary: %.3g bars" % worst)
    assert worst >= ea.PREMISE_MARGIN
    assert {c.model for c in ea.SWEEP_CASES} == set(ea.MF_MODELS + ea.EXT_MODELS) and {c.k for c in ea.SWEEP_CASES} == set(ea.KS)
    assert {c.n for c in ea.SIZE_CASES} == set(ea.NS)


def test_the_premise_check_sees_a_prediction_on_a_boundary():
    ev = ea.eval_ratings_ref(np.array([2.25 + 1e-12, 3.1]), np.array([2.0, 3.0]), 0.5, 5.0)
    assert ea.rounding_margin(ev, 1e-14, 0.5) < ea.PREMISE_MARGIN
    with pytest.raises(AssertionError):
        ea.assert_rounding_premise(ev, 1e-14, 0.5)


# ---- the mutants -------------------------------------------------------------------------------------------------------------------

EVAL_MUTANTS = {"round-unscaled": ea.SCALES[1:], "round-before-clip": ea.SCALES, "nmae-over-max": ea.SCALES}   # scales each applies to


# (a handful of tuples need not hold a prediction that a given mutant rounds differently: the n = 1 .. 5 cases are left out)
@pytest.mark.parametrize("case", CPU_CASES + [c for c in ea.SIZE_CASES if c.model in ea.MF_MODELS and c.n >= 100], ids=ea.case_id)
@pytest.mark.parametrize("mutant", sorted(EVAL_MUTANTS))
def test_evalratings_mutants_move_a_measure_by_ten_bars(case, mutant):
    p = ea.problem(case)
    for s in EVAL_MUTANTS[mutant]:
        ev, bars = p.evals[s], ea.measure_bars(p.evals[s], p.bar[s], *s)
        mut = ea.eval_ratings_ref(p.pred[s], p.ratings[s], *s, mutant=mutant)
        ratio = max(abs(mut.measures[name] - ev.measures[name]) / bars[name] for name in ea.MEASURES)
        assert ratio >= SEPARATION, (mutant, s, ratio)


@pytest.mark.parametrize("case", ea.NAN_CASES, ids=ea.case_id)
def test_counting_a_nan_prediction_is_seen(case):
    """the reference skips a NaN prediction; a sum that takes it in is NaN, a count that takes it in is off by the number of them"""
    p = ea.problem(case)
    for s in ea.SCALES:
        pred = p.pred[s].copy()
        pred[p.u == 5] = np.nan
        ev = ea.eval_ratings_ref(pred, p.ratings[s], *s)
        mut = ea.eval_ratings_ref(pred, p.ratings[s], *s, mutant="nan-counted")
        assert 0 < ev.n == case.n - np.count_nonzero(p.u == 5) < mut.n == case.n
        assert np.isfinite(list(ev.measures.values())).all() and np.isnan(list(mut.measures.values())).all()


PREDICT_MUTANTS = {"no-bu": ea.HAS_BU, "no-bj": ea.HAS_BJ, "ic-by-user": ("CAMF_CUCI",)}


@pytest.mark.parametrize("case", CPU_CASES, ids=ea.case_id)
@pytest.mark.parametrize("mutant", sorted(PREDICT_MUTANTS))
def test_prediction_mutants_move_the_predictions_and_a_measure_by_ten_bars(case, mutant):
    p = ea.problem(case)
    s = ea.SCALES[1]
    pred, _, _ = ea.predict_ref(case.model, p.state, p.gm[s], p.u, p.j, p.ctx, mutant=mutant)
    if case.model not in PREDICT_MUTANTS[mutant]:
        assert np.array_equal(pred, p.pred[s])                     # the model has no such term: nothing changes
        return
    moved = np.abs(pred - p.pred[s]) / p.bar[s]
    assert np.median(moved) >= SEPARATION and np.count_nonzero(moved >= SEPARATION) >= 0.5 * case.n
    ev, bars = p.evals[s], ea.measure_bars(p.evals[s], p.bar[s], *s)
    mut = ea.eval_ratings_ref(pred, p.ratings[s], *s)
    assert max(abs(mut.measures[name] - ev.measures[name]) / bars[name] for name in ea.MEASURES) >= SEPARATION


# ---- the constructed ties ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", ea.TIE_MODELS)
def test_constructed_ties_are_exact_and_round_half_up(model):
    st, gm, u, j, ctx, want = ea.tie_problem(model, False)
    if model in ea.MF_MODELS:
        pred, _, _ = ea.predict_ref(model, st, gm, u, j, ctx)
    else:
        pred, _ = ea.reference_predictions(model, st, gm, u, j, ctx, ea.train_tuples(model), 1, False)
    assert np.array_equal(pred, want)
    for s in ea.SCALES:
        lo, hi = s
        ev = ea.eval_ratings_ref(pred, ea.tie_ratings(len(u), s), *s)
        assert ev.n == len(u)                                      # +inf bounds to maxRate and is counted
        x = ev.pred / lo
        ties = x - np.floor(x) == 0.5
        assert np.count_nonzero(ties) >= 3 and np.all(ev.rpred[ties] == ev.pred[ties] + lo / 2)      # half a level goes up
        assert np.all(ev.pred[u == 3] == hi) and ev.pred.min() == lo and ev.pred.max() == hi
        assert np.count_nonzero(want > hi) >= 2 and np.count_nonzero(want < lo) >= 2
        for mutant in ("round-unscaled", "round-before-clip", "nmae-over-max"):
            if mutant == "round-unscaled" and lo == 1.0:
                continue
            mut = ea.eval_ratings_ref(pred, ea.tie_ratings(len(u), s), *s, mutant=mutant)
            assert any(mut.measures[name] != ev.measures[name] for name in ea.MEASURES), (s, mutant)
    lo = 0.5
    assert want[0] == 2.25 and np.floor(want[0] / lo + 0.5) * lo == 2.5 and np.floor(want[0] / lo) * lo == 2.0


def test_all_nan_gives_nan_measures_and_a_zero_count():
    ev = ea.eval_ratings_ref(np.full(4, np.nan), np.ones(4), 0.5, 5.0)
    assert ev.n == 0 and all(np.isnan(v) for v in ev.measures.values())


# ---- the restatements against the reference's own evalRatings, run at 0.5 .. 5 and 2 .. 10 ------------------------------------------

@pytest.mark.parametrize("case", GOLD, ids=lambda c: "%s-%g-%g" % (c["model"], c["min_rate"], c["max_rate"]))
def test_interpreted_reference_source_at_non_unit_scales_bit_for_bit(case):
    """one interpreted buildModel() epoch, then evalRatings() with minRate / maxRate = the fixture's: the C oracle and the Python
    restatement reproduce the model and the five measures bit for bit (they sum in the reference's order); eval_anchor's evalRatings
    does too when given the oracle's predictions, and its own predict is within the per-tuple bar"""
    u, j, ctx, r, ctx_ptr, ctx_conds, state = src._inputs(case)
    p, gm, lo, hi = case["problem"], src.fx(case["global_mean"]), case["min_rate"], case["max_rate"]
    assert (lo, hi) in ea.SCALES[1:] and case["iters"] == 1
    orc = oracle_c.Oracle(case["model"], case["k"], p["n_users"], p["n_items"], p["n_conds"], u, j, ctx, r, ctx_ptr, ctx_conds, state, gm,
                          case["regU"], case["regI"], case["regB"], case["regC"])
    losses, lrates, _ = orc.build_model(1, case["lrate"], bold_driver=case["bold_driver"])
    src._check(case, losses, lrates, orc.state)
    tu, tj, tc, tr = src._test_tuples(case)
    assert set(np.unique(tr / lo)) <= set(range(1, int(hi / lo) + 1)) and set(np.unique(tr)) - {1.0, 2.0, 3.0, 4.0, 5.0}     # ratings on the scale
    want = {name: src.fx(v) for name, v in case["eval_ratings"].items()}
    assert want["MPE"] == 0.0
    res = orc.eval_ratings(tu, tj, tc, tr, lo, hi)
    conds = [ctx_conds[ctx_ptr[x]:ctx_ptr[x + 1]].tolist() for x in range(len(ctx_ptr) - 1)]
    m = oracle_np.MODELS[case["model"]](case["k"], p["n_users"], p["n_items"], p["n_conds"], conds, gm, 0.0, 0.0, 0.0, 0.0)
    final = {n: np.array([src.fx(x) for x in v]).reshape(src.SHAPES(case)[n]) for n, v in case["final"].items()}
    for n, a in final.items():
        setattr(m, n, a.tolist())
    res2 = oracle_np.eval_ratings(m, list(zip(tu.tolist(), tj.tolist(), tc.tolist(), tr.tolist())), lo, hi)
    exact = np.array([m.predict(a, b, c) for a, b, c in zip(tu.tolist(), tj.tolist(), tc.tolist())])
    ev = ea.eval_ratings_ref(exact, tr, lo, hi)
    for got in (res, res2, dict(ev.measures, n=ev.n)):
        assert got["n"] == len(tr)
        for name in ea.MEASURES:
            assert float(got[name]).hex() == case["eval_ratings"][name], name
    # eval_anchor's own predictions, then the measures within the derived bars
    pred, S, mm = ea.predict_ref(case["model"], final, gm, tu, tj, tc, ctx_ptr, ctx_conds)
    bar = ea.predict_bar(S, mm, case["k"], True)
    assert np.all(np.abs(pred - exact) <= bar)
    own = ea.eval_ratings_ref(pred, tr, lo, hi)
    bars = ea.measure_bars(own, bar, lo, hi)
    for name in ea.MEASURES:
        assert abs(own.measures[name] - want[name]) <= bars[name], name
    # the fixture can tell the scale-blind rounding and the NMAE over maxRate alone from the reference's
    blind = ea.eval_ratings_ref(exact, tr, lo, hi, mutant="round-unscaled").measures
    assert blind["rMAE"] != want["rMAE"] or blind["rRMSE"] != want["rRMSE"]
    assert ea.eval_ratings_ref(exact, tr, lo, hi, mutant="nmae-over-max").measures["NMAE"] != want["NMAE"]
