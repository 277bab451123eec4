"""The CPU restatement of SlopeOne (tests/slopeone_ref.py) against the run of the reference's own source
(tests/golden/reference_slopeone.json.gz, tests/tools/mint_reference_slopeone.py), bit for bit, and against hand-derived answers."""
import math

import numpy as np
import pytest

from tests import slopeone_ref as sref
from tests.util import same_bits_exact

RUNS = sref.golden_runs()


def bits(x):
    return float(x).hex()


@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_restatement_equals_the_reference_run(run):
    nu, ni = run["n_users"], run["n_items"]
    rows = sref.rows_of(run["u"], run["i"], run["r"], nu)
    dev, card = sref.build(rows, ni)
    assert np.array_equal(card, run["card"])
    assert same_bits_exact(dev, run["dev"]), np.argwhere(dev.view(np.int64) != run["dev"].view(np.int64))[:5]
    gm, lo, hi = run["global_mean"], run["min_rate"], run["max_rate"]
    free = [[sref.predict(dev, card, rows, u, j, gm) for j in range(ni)] for u in range(nu)]
    bounded = [[sref.predict(dev, card, rows, u, j, gm, True, lo, hi) for j in range(ni)] for u in range(nu)]
    assert same_bits_exact(free, run["predict"])
    assert same_bits_exact(bounded, run["predict_bounded"])


def test_golden_file_holds_the_cases_it_is_for():
    knn, hand = RUNS
    assert (knn["n_users"], knn["n_items"]) == (26, 42)
    zero = (knn["card"] > 0) & (knn["dev"] == 0.0)
    assert zero.any() and not np.signbit(knn["dev"][zero]).any()          # zero deviations: +0.0 on both sides
    assert (zero & zero.T).any()
    assert (knn["card"].sum(axis=0) == 0).any()                            # an empty item
    assert any(v != round(v) for v in knn["r"].tolist())                   # fractional cells
    assert (knn["predict"] != knn["predict_bounded"]).any() or (hand["predict"] != hand["predict_bounded"]).any()
    off = ~np.eye(hand["n_items"], dtype=bool)
    assert ((hand["card"] == 0) & off).any()                               # a pair without a common user
    assert (hand["predict"] == hand["global_mean"]).any()


def test_pair_walk_equals_the_user_loop():
    """the per-pair formulation (what the GPU kernel computes: one side summed, the other mirrored) is the reference's loop bit for bit"""
    for run in RUNS:
        rows = sref.rows_of(run["u"], run["i"], run["r"], run["n_users"])
        cols = sref.cols_of(run["u"], run["i"], run["r"], run["n_items"])
        dev, card = sref.build(rows, run["n_items"])
        for a in range(run["n_items"]):
            for b in range(a + 1, run["n_items"]):
                dab, dba, k = sref.pair(cols[a], cols[b])
                assert (bits(dab), bits(dba), k) == (bits(dev[a, b]), bits(dev[b, a]), card[a, b]) and card[b, a] == k
        part = sref.build_rows(cols, [0, run["n_items"] - 1])
        for a, (d, c) in part.items():
            assert same_bits_exact(d, dev[a]) and np.array_equal(c, card[a])


def test_two_users_two_items():
    rows = [[(0, 4.0), (1, 2.5)], [(0, 5.0 / 3.0), (1, 3.0)]]
    dev, card = sref.build(rows, 2)
    want = ((4.0 - 2.5) + (5.0 / 3.0 - 3.0)) / 2
    assert dev[0, 1] == want and dev[1, 0] == -want and dev[0, 0] == dev[1, 1] == 0.0
    assert card.tolist() == [[0, 2], [2, 0]]


def test_equal_columns_give_positive_zero_on_both_sides():
    rows = [[(0, 5.0 / 3.0), (1, 5.0 / 3.0)], [(0, 2.0), (1, 2.0)]]
    dev, card = sref.build(rows, 2)
    assert card[0, 1] == card[1, 0] == 2
    assert bits(dev[0, 1]) == bits(dev[1, 0]) == bits(0.0)
    assert sref.pair([(0, 5.0 / 3.0), (1, 2.0)], [(0, 5.0 / 3.0), (1, 2.0)]) == (0.0, 0.0, 2)
    assert not math.copysign(1.0, sref.pair([(0, 1.0), (1, 2.0)], [(0, 2.0), (1, 1.0)])[1]) < 0   # +1 - 1: a zero sum of non-zero terms


def test_disjoint_pair_has_no_cardinality():
    rows = [[(0, 4.0)], [(1, 2.0)]]
    dev, card = sref.build(rows, 2)
    assert card.tolist() == [[0, 0], [0, 0]] and not dev.any()
    assert sref.predict(dev, card, rows, 0, 1, 3.25) == 3.25               # nothing to add: globalMean


def test_lone_item_gives_global_mean():
    rows = [[(0, 4.0), (1, 2.0)], [(1, 5.0)], []]
    dev, card = sref.build(rows, 2)
    assert sref.predict(dev, card, rows, 1, 1, 3.5) == 3.5                  # the only item is j itself
    assert sref.predict(dev, card, rows, 2, 0, 3.5) == 3.5                  # no ratings at all
    assert sref.predict(dev, card, rows, 1, 0, 3.5) == (2.0 + 5.0) * 1.0 / 1.0


def test_bounded_prediction_is_clamped():
    rows = [[(0, 5.0), (1, 1.0)], [(1, 4.0)], [(0, 1.5)]]
    dev, card = sref.build(rows, 2)
    assert sref.predict(dev, card, rows, 1, 0, 3.0) == 8.0
    assert sref.predict(dev, card, rows, 1, 0, 3.0, True, 1.0, 5.0) == 5.0
    assert sref.predict(dev, card, rows, 2, 1, 3.0) == -2.5
    assert sref.predict(dev, card, rows, 2, 1, 3.0, True, 1.0, 5.0) == 1.0
