"""tests/nmf_ref.py (the CPU restatement the GPU tests compare against) equals the run of the reference's own NMF source
(tests/golden/reference_nmf.json.gz, minted by tests/tools/mint_reference_nmf.py) bit for bit: W, H and the loss of every iteration,
the predictions, and initModel()'s draws."""
import numpy as np

from tests import nmf_ref as nref
from tests.hostmirror.javarand import JavaRandom
from tests.util import same_bits_exact


def test_iterations_and_predictions_match_the_reference_run():
    runs = nref.golden_runs()
    assert [r["name"] for r in runs] == ["knn_matrix k=3", "knn_matrix k=10", "handmade k=2"]
    for run in runs:
        nu, ni = run["n_users"], run["n_items"]
        rows, cols = nref.rows_of(run["u"], run["i"], run["r"], nu), nref.cols_of(run["u"], run["i"], run["r"], ni)
        W, Ht = run["W0"].copy(), np.ascontiguousarray(run["H0"].T)
        assert len(run["iters"]) == 3
        for n, it in enumerate(run["iters"]):
            loss = nref.iterate(W, Ht, rows, cols)
            assert same_bits_exact(W, it["W"]), (run["name"], n)
            assert same_bits_exact(Ht.T, it["H"]), (run["name"], n)
            assert same_bits_exact([loss], [it["loss"]]), (run["name"], n, loss, it["loss"])
        lo, hi = run["min_rate"], run["max_rate"]
        pred = [[nref.predict(W, Ht, u, j) for j in range(ni)] for u in range(nu)]
        bounded = [[nref.predict(W, Ht, u, j, True, lo, hi) for j in range(ni)] for u in range(nu)]
        assert same_bits_exact(pred, run["predict"]) and same_bits_exact(bounded, run["predict_bounded"]), run["name"]
        assert (run["predict"] < lo).any()           # the bound is at work


def test_rows_without_entries_stay_and_updates_move_the_rest():
    run = nref.golden_runs()[2]                      # handmade: user 5 has no ratings
    it = run["iters"][0]
    assert same_bits_exact(it["W"][5], run["W0"][5]) and not same_bits_exact(it["W"][0], run["W0"][0])


def test_init_model_draws():
    g = nref.golden()["init"]
    nu, ni, k = g["n_users"], g["n_items"], g["k"]
    W, Ht = nref.init_model(JavaRandom(g["seed"]), nu, ni, k)
    assert same_bits_exact(W, nref.unhex(g["W"], nu, k))
    assert same_bits_exact(Ht.T, nref.unhex(g["H"], k, ni))
    assert 0.0 <= W.min() and W.max() < 0.01
