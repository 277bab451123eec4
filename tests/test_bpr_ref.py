"""tests/bpr_ref.py against the reference's own run (tests/golden/reference_bpr.json.gz, minted by tests/tools/mint_reference_bpr.py):
the sampler's triples and stream states, P, Q and loss after each of three iterations, every predict, what librec makes of the rows;
the fdlibm exp / log restatements against libm."""
import math

import numpy as np
import pytest

from oracle import oracle_np
from tests import bpr_ref as bref
from tests.util import same_bits_exact


@pytest.fixture(scope="module")
def runs():
    return bref.golden_runs()


def test_golden_file_holds_the_runs_the_restatement_is_pinned_to(runs):
    assert sorted(r["name"] for r in runs) == ["handmade k=1", "handmade k=2", "knn_matrix k=10", "knn_matrix k=3"]
    for r in runs:
        assert len(r["iters"]) == 3 and all(len(it["triples"]) == r["n_users"] * 100 for it in r["iters"])


def test_stored_zeros_and_contains_as_librec_has_them(runs):
    """getCount() == len(getIndex()) on every row (a stored 0.0 is in neither: no slot past the count can be drawn as item 0), and
    contains() is the whole-capacity binary search, which misses entries"""
    missed = 0
    for r in runs:
        m = bref.BPR(r["n_users"], r["n_items"], r["cells"])
        assert r["row_count"] == r["index_len"] == [len(row) for row in m.rows], r["name"]
        for u in range(r["n_users"]):
            assert [int(bref.contains(m.rows[u], j)) for j in range(r["n_items"])] == r["contains"][u], (r["name"], u)
            missed += sum(1 for j in m.rows[u] if not r["contains"][u][j])
    hand = next(r for r in runs if r["name"] == "handmade k=1")
    assert hand["row_count"] == [3, 2, 1, 2, 3, 0, 0]     # user 1's stored zero is gone; users 5 (no cell) and 6 (a stored zero) are empty
    assert missed > 0                                      # the knn_matrix rows have entries contains() cannot find


def test_restatement_equals_the_golden_runs(runs):
    for r in runs:
        m = bref.BPR(r["n_users"], r["n_items"], r["cells"])
        rnd = bref.JavaStream(bref.random_state(r["seed"]))
        P, Q = r["P0"].tolist(), r["Q0"].tolist()
        same_ij = 0
        for t, it in enumerate(r["iters"]):
            tri = m.sample_iteration(rnd)
            assert tri == it["triples"], (r["name"], t)
            assert rnd.state == it["state"], (r["name"], t)
            loss = bref.epoch(P, Q, tri, r["lrate"], r["reg_u"], r["reg_i"])
            assert same_bits_exact(np.array(P), it["P"]) and same_bits_exact(np.array(Q), it["Q"]), (r["name"], t)
            assert same_bits_exact([loss], [it["loss"]]), (r["name"], t, loss, it["loss"])
            same_ij += sum(1 for _, i, j in tri if i == j)
        assert same_bits_exact(bref.scores(P, Q), r["predict"]), r["name"]
        if r["name"].startswith("knn_matrix"):
            assert same_ij > 0      # an item contains() misses was drawn as j beside itself as i: two adds to one row


def test_init_model_equals_the_reference_draw():
    g = bref.golden()["init"]
    nu, ni, k = g["n_users"], g["n_items"], g["k"]
    P, Q = bref.init_model(oracle_np.JavaRandom(g["seed"]), nu, ni, k)
    assert same_bits_exact(P, bref.unhex(g["P"], nu, k)) and same_bits_exact(Q, bref.unhex(g["Q"], ni, k))


def _ulps(a, b):
    if a == b:
        return 0
    return abs(bref._bits(a) - bref._bits(b))     # same sign, finite


def test_fdlibm_exp_against_libm():
    """within 1 ulp of the correctly rounded value everywhere; the share of identical results is printed, no threshold is set on it"""
    xs = np.random.default_rng(20261210).uniform(-40.0, 40.0, 100000)
    same = 0
    for x in xs.tolist():
        a, b = bref.fdlibm_exp(x), math.exp(x)
        assert _ulps(a, b) <= 1, (x, a, b)
        same += a == b
    print("fdlibm exp == libm exp at %.3f %% of %d arguments in [-40, 40]" % (100.0 * same / len(xs), len(xs)))
    inf, nan = math.inf, math.nan
    assert bref.fdlibm_exp(0.0) == 1.0 and bref.fdlibm_exp(-0.0) == 1.0
    assert bref.fdlibm_exp(inf) == inf and bref.fdlibm_exp(-inf) == 0.0 and math.isnan(bref.fdlibm_exp(nan))
    assert bref.fdlibm_exp(709.782712893384) == math.exp(709.782712893384) and bref.fdlibm_exp(709.7827128933841) == inf
    assert bref.fdlibm_exp(-745.1332191019411) == 5e-324 and bref.fdlibm_exp(-745.1332191019412) == 0.0
    assert bref.fdlibm_exp(-710.0) == math.exp(-710.0)            # a subnormal result: the 2^-1000 path
    assert bref.fdlibm_exp(1e-10) == 1.0 + 1e-10 and bref.fdlibm_exp(0.5) == math.exp(0.5)


def test_fdlibm_log_edges_and_the_oracle_log():
    inf, nan = math.inf, math.nan
    assert bref.fdlibm_log(0.0) == -inf and bref.fdlibm_log(-0.0) == -inf and math.isnan(bref.fdlibm_log(-1.0))
    assert bref.fdlibm_log(inf) == inf and math.isnan(bref.fdlibm_log(nan)) and bref.fdlibm_log(1.0) == 0.0
    assert _ulps(bref.fdlibm_log(5e-324), math.log(5e-324)) <= 1
    for x in np.random.default_rng(20261211).uniform(1e-6, 50.0, 20000).tolist():
        assert bref.fdlibm_log(x) == oracle_np.fdlibm_log(x)      # the restatement the project already pins nextGaussian with
        assert _ulps(bref.fdlibm_log(x), math.log(x)) <= 1


def test_next_int_known_answers_and_the_rejection_branch():
    r = bref.JavaStream(bref.random_state(42))
    assert [r.next_int(10) for _ in range(5)] == [0, 3, 8, 4, 0]      # new java.util.Random(42).nextInt(10), the JDK's known answers
    r = bref.JavaStream(bref.random_state(7))
    v = [r.next_int((1 << 30) + 1) for _ in range(2000)]
    assert all(0 <= x <= 1 << 30 for x in v) and r.draws > 2000 + 500   # about half of the draws are rejected
    r = bref.JavaStream(bref.random_state(7))
    assert [r.next_int(1) for _ in range(10)] == [0] * 10 and r.draws == 10


def test_levels_rule():
    tri = [(0, 0, 1), (1, 1, 2), (0, 2, 3), (2, 3, 0), (3, 4, 4)]
    assert bref.levels(4, 5, tri) == [1, 2, 3, 4, 1]


def test_level_wise_epoch_has_the_sequential_epochs_bits(runs):
    for r in runs:
        P, Q = r["P0"].copy(), r["Q0"].copy()
        for t, it in enumerate(r["iters"]):
            loss, terms = bref.epoch_by_levels(P, Q, it["triples"], r["lrate"], r["reg_u"], r["reg_i"])
            assert same_bits_exact(P, it["P"]) and same_bits_exact(Q, it["Q"]) and same_bits_exact([loss], [it["loss"]]), (r["name"], t)
            assert terms.shape == (r["n_users"] * 100, r["k"] + 1) and np.all(terms >= 0.0)
