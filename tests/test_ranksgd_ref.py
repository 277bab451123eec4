"""tests/ranksgd_ref.py against the golden file minted from RankSGD.java (tests/tools/mint_reference_ranksgd.py): the item list, every
random() value, the accepted j per cell, P, Q, the loss and the stream state of three iterations, bit for bit; the epoch by levels has
the sequential epoch's bits.  What the reference makes of numRates and of stored zeros is asserted from the recorded facts."""
import math

import numpy as np
import pytest

from tests import ranksgd_ref as rr
from tests.util import same_bits_exact

RUNS = rr.golden_runs()


def test_the_reference_divides_by_an_unassigned_field():
    """`numRates` is declared and never assigned: the recorded value is 0 and every probability +Infinity, in HashMap order"""
    gd = rr.golden()
    ref = [r for r in gd["runs"] if r["num_rates"] == "reference"] + gd["lists"]
    assert len(ref) == 4
    for r in ref:
        assert r["num_rates_value"] == 0 and r["size"] > 0
        assert all(float.fromhex(p) == math.inf for p in r["probs"]) and r["probs"]
    by = {r["name"]: r for r in ref}
    assert by["handmade"]["items"] == [0, 1, 2, 3, 4]
    assert by["ties"]["items"] == [1, 17, 33, 2, 18, 34, 3, 19, 35]        # bucket order of a 16-slot table, not ascending ids
    assert by["escape"]["items"][0] == 32
    for r in gd["runs"]:
        if r["num_rates"] == "size":
            assert r["num_rates_value"] == r["size"]


def test_stored_zeros_take_no_part():
    run = next(r for r in RUNS if r["name"].startswith("handmade"))
    assert len(run["cells"]) == 13 and run["size"] == 11                    # two stored zeros
    assert run["column_size"] == [3, 2, 2, 2, 2, 0] and run["rows"] == [0, 1, 2, 3, 4]
    assert run["column_size"] == rr.column_sizes(run["n_items"], run["cells"])


def test_the_ties_list_is_not_in_ascending_id_order():
    run = next(r for r in RUNS if r["name"].startswith("ties"))
    assert run["items"] != sorted(run["items"]) and run["probs"] == sorted(run["probs"])
    assert run["items"] == [17, 33, 18, 34, 3, 19, 35, 1, 2]


@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_restatement_equals_the_golden_run(run):
    m = rr.RankSGD(run["n_users"], run["n_items"], run["cells"], run["num_rates"])
    assert m.items == run["items"] and same_bits_exact(m.probs, run["probs"])
    assert [u for u, row in enumerate(m.rows) if row] == run["rows"] and m.n_cells == run["size"]
    P, Q = run["P0"].tolist(), run["Q0"].tolist()
    P2, Q2 = run["P0"].copy(), run["Q0"].copy()
    rnd = rr.JavaStream(rr.random_state(run["seed"]))
    any_equal = 0
    for it in run["iters"]:
        state0 = rnd.state
        tri, used = m.sample_iteration(rnd)
        assert [t[2] for t in tri] == it["j"] and rnd.state == it["state"] and used == len(it["randoms"])
        chk = rr.JavaStream(state0)
        assert [rr.next_double(chk) for _ in range(used)] == it["randoms"]
        loss = rr.epoch(P, Q, tri, run["lrate"])
        assert same_bits_exact([loss], [it["loss"]])
        assert same_bits_exact(np.array(P), it["P"]) and same_bits_exact(np.array(Q), it["Q"])
        loss2, _ = rr.epoch_by_levels(P2, Q2, tri, run["lrate"])
        assert same_bits_exact([loss2], [loss]) and same_bits_exact(P2, it["P"]) and same_bits_exact(Q2, it["Q"])
        any_equal += sum(t[1] == t[2] for t in tri)
    if run["name"].startswith(("escape", "knn_matrix")):
        assert any_equal > 0                                                # j == i happened in the reference's own run


def test_try_keeps_the_first_entry_that_reaches_the_number_and_reports_none():
    rnd = rr.JavaStream(rr.random_state(5))
    got = [rr.try_item(rnd, [7, 8], [0.25, 0.5]) for _ in range(2000)]
    assert set(got) == {7, 8, -1} and 800 < got.count(-1) < 1200 and rnd.draws == 4000


def test_assign_rules():
    rows = [[1, 2, 3], [], [5]]
    # a rated item that contains() misses is accepted: [1, 2, 3] has capacity 4 = [1, 2, 3, 0]; 3 is found, so take a row of 5
    five = [[10, 11, 12, 13, 14]]
    assert not rr.contains(five[0], 14) and rr.contains(five[0], 12)
    js, used = rr.assign(five, [14, 12, 14, 10, 3, 14, 14, 11, 9])
    assert js == [14, 14, 3, 14, 14] and used == 7                          # the cell on item 14 took j == i
    js, used = rr.assign(rows, [1, -1, 7, 0, 2, 4, 5, -1, 6])               # -1 after a rejection: one more rejection
    assert js == [7, 0, 4, 6] and used == 9
    with pytest.raises(rr.FirstTryMiss):
        rr.assign(rows, [7, -1])
