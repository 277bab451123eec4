"""tests/lrmf_ref.py against the reference's own run (tests/golden/reference_lrmf.json.gz, minted by tests/tools/mint_reference_lrmf.py):
userExp, P, Q and loss after each iteration, every predict, what librec makes of stored zeros; the numpy forms against the scalar ones."""
import math

import numpy as np
import pytest

from tests import bpr_ref as bref
from tests import lrmf_ref as lref
from tests.util import same_bits_exact


@pytest.fixture(scope="module")
def runs():
    return lref.golden_runs()


def test_golden_file_holds_the_runs_the_restatement_is_pinned_to(runs):
    assert sorted(r["name"] for r in runs) == ["handmade k=1", "handmade k=2", "handmade_finite k=1", "handmade_finite k=2",
                                               "knn_matrix k=10", "knn_matrix k=3"]
    for r in runs:
        # the user whose only cell is a stored zero ends the reference's run in iteration 1 (a non-finite loss)
        assert len(r["iters"]) == (1 if r["name"].startswith("handmade k") else 3), r["name"]


def test_stored_zeros_as_librec_has_them(runs):
    """the iterator yields a stored 0.0, getColumns(u) leaves it out, and it adds exp(0) = 1 to userExp[u]"""
    for r in runs:
        m = lref.LRMF(r["n_users"], r["n_items"], r["cells"])
        assert m.cells == r["entries"], r["name"]                    # the iterator: rows ascending, columns ascending, zeros among them
        assert m.columns == r["columns"], r["name"]
        assert same_bits_exact(np.array(m.user_exp), r["user_exp"]), r["name"]
    hand = next(r for r in runs if r["name"] == "handmade k=1")
    assert (1, 3, 0.0) in hand["entries"] and (6, 1, 0.0) in hand["entries"]
    assert hand["columns"][1] == [0, 1] and hand["columns"][6] == [] and hand["columns"][5] == []
    want = bref.fdlibm_exp(3.0) + bref.fdlibm_exp(3.5) + 1.0         # user 1: two cells and the stored zero's exp(0)
    assert same_bits_exact([hand["user_exp"][1]], [want]) and hand["user_exp"][6] == 1.0 and hand["user_exp"][5] == 0.0


def test_only_stored_zero_user_makes_the_reference_non_finite(runs):
    for r in runs:
        if r["name"].startswith("handmade k"):
            it = r["iters"][0]
            assert not math.isfinite(it["loss"]) and not np.all(np.isfinite(it["P"][6])), r["name"]
            assert np.all(np.isfinite(it["P"][:6]))                  # the other users' rows are as finite as ever
        else:
            assert all(math.isfinite(it["loss"]) for it in r["iters"])


def test_restatement_equals_the_golden_runs(runs):
    for r in runs:
        m = lref.LRMF(r["n_users"], r["n_items"], r["cells"])
        P, Q = r["P0"].tolist(), r["Q0"].tolist()
        for t, it in enumerate(r["iters"]):
            loss = m.epoch(P, Q, r["lrate"], r["reg_u"], r["reg_i"])
            assert same_bits_exact(np.array(P), it["P"]) and same_bits_exact(np.array(Q), it["Q"]), (r["name"], t)
            assert same_bits_exact([loss], [it["loss"]]), (r["name"], t, loss, it["loss"])
        assert same_bits_exact(lref.scores(P, Q), r["predict"]), r["name"]


def test_numpy_epoch_has_the_scalar_epochs_bits(runs):
    for r in runs:
        m = lref.LRMF(r["n_users"], r["n_items"], r["cells"])
        P, Q = r["P0"].copy(), r["Q0"].copy()
        for t, it in enumerate(r["iters"]):
            loss, terms = m.epoch_np(P, Q, r["lrate"], r["reg_u"], r["reg_i"])
            assert same_bits_exact(P, it["P"]) and same_bits_exact(Q, it["Q"]) and same_bits_exact([loss], [it["loss"]]), (r["name"], t)
            assert terms.shape == (len(m.cells) * (r["k"] + 1),)


def test_exp_vec_equals_the_scalar_exp():
    inf, nan = math.inf, math.nan
    xs = np.concatenate([np.random.default_rng(20270210).uniform(-40.0, 40.0, 200000),
                         np.random.default_rng(20270211).uniform(-760.0, 720.0, 50000),
                         [0.0, -0.0, inf, -inf, nan, 709.782712893384, 709.7827128933841, -745.1332191019411, -745.1332191019412, -710.0,
                          -709.0, -708.0, 699.9999, 700.0, 1e-10, -1e-10, 0.3, -0.3, 0.4, 0.35, 1.0, -1.0, 1.03, 1.04, 1.1, 5e-324, 1e300]])
    got = lref.exp_vec(xs)
    want = np.array([bref.fdlibm_exp(x) for x in xs.tolist()])
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert same_bits_exact(got[ok], want[ok])


def test_java_division_and_gd():
    inf = math.inf
    assert lref.jdiv(1.0, 0.0) == inf and lref.jdiv(-1.0, 0.0) == -inf and math.isnan(lref.jdiv(0.0, 0.0)) and lref.jdiv(1.0, -0.0) == -inf
    assert lref.gd(0.0) == 0.25 and lref.gd(800.0) == 0.0 and lref.gd(-800.0) == 0.0     # g(-800) = 1 / (1 + Inf) = 0.0


def test_levels_rule():
    cells = [(0, 0, 1.0), (0, 1, 1.0), (1, 1, 0.0), (1, 2, 1.0), (2, 3, 1.0), (4, 2, 1.0), (4, 3, 1.0)]
    assert lref.levels(5, 4, cells) == [1, 2, 1, 0, 3]               # user 1 hangs on user 0 through a stored zero; user 3 has no cell
