"""tests/slim_ref.py (the CPU restatement the GPU tests compare against) equals the run of the reference's own SLIM source
(tests/golden/reference_slim.json.gz, minted by tests/tools/mint_reference_slim.py) bit for bit: the neighbour lists in iteration order,
initModel()'s listed cells of W, W after iterations 1, 2 and 5, every iteration's loss and every score."""
import numpy as np
import pytest

from tests import slim_ref as sref
from tests.hostmirror.javarand import JavaRandom
from tests.util import same_bits_exact

RUNS = sref.golden_runs()
KNN_RUNS = [(knn, l1, l2) for knn in (0, 1, 3, 5, 12, 1000) for l1, l2 in ((1.0, 1.0), (0.1, 0.5), (0.0, 0.0))]


def flat(W):
    return np.concatenate([np.asarray(w, dtype=np.float64) for w in W]) if len(W) else np.zeros(0)


def test_the_golden_file_covers_the_issue_s_cases():
    got = [(r["knn"], r["l1"], r["l2"]) for r in RUNS if r["matrix"] == "knn_matrix"]
    assert got == [(k, sref.f32(a), sref.f32(b)) for k, a, b in KNN_RUNS]
    assert [r["knn"] for r in RUNS if r["matrix"] == "edge_matrix"] == [3, 4, 6, 7, 12, 13, 24, 25]
    assert sref.golden()["hashset_initial_capacity"] == 3           # new HashSet(3): a table of 4 slots
    # a list length on each side of every growth step of the value set (4 -> 8 -> 16 -> 32 -> 64 slots)
    lens = {len(lst) for r in RUNS for lst in r["neighbors"]}
    assert {3, 4, 6, 7, 12, 13, 24, 25} <= lens
    edge = next(r for r in RUNS if r["matrix"] == "edge_matrix")
    assert any(v == 0.0 for _, _, v in edge["cells"])                # a stored zero cell
    s = sref.Slim(edge["n_users"], edge["n_items"], edge["cells"])
    missed = [(u, k) for u in range(s.nu) for k, f in s.found[u].items() if not f]
    # a user whose row length is no power of two has an entry contains() misses, and that entry is a neighbour of some column
    assert any(len(s.rows[u]) & (len(s.rows[u]) - 1) and any(k in lst for lst in edge["neighbors"]) for u, k in missed)
    assert any(x < 0 for r in RUNS for w in r["W"].values() for x in flat(w))  # the negative branch of the update is taken


@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_restatement_equals_the_reference_run(run):
    s = sref.Slim(run["n_users"], run["n_items"], run["cells"])
    nbr = s.neighbors(run["knn"], run["measure"], run["shrinkage"])
    assert s.treeified == 0
    assert nbr == run["neighbors"]
    W = sref.init_weights(JavaRandom(1), run["n_users"], run["n_items"], sref.INIT_FACTORS, nbr)
    assert same_bits_exact(flat(W), flat(run["W0"]))
    assert 1 <= len(run["loss"]) <= 5
    for it, want in enumerate(run["loss"], 1):
        loss = s.iterate(nbr, W, run["l1"], run["l2"])
        assert same_bits_exact([loss], [want]), (it, loss, want)
        if it in run["W"]:
            assert same_bits_exact(flat(W), flat(run["W"][it])), it
    assert sorted(run["W"]) == [it for it in (1, 2, 5) if it <= len(run["loss"])]
    # SLIM.isConverged: the run ended early exactly where last_loss - loss < 1e-5 after the first iteration
    stops = [it for it in range(2, len(run["loss"]) + 1) if run["loss"][it - 2] - run["loss"][it - 1] < 1e-5]
    assert (stops[0] == len(run["loss"])) if stops else len(run["loss"]) == 5
    assert same_bits_exact(s.scores(nbr, W), run["predict"])


def test_all_items_list_and_the_diagonal_coordinate():
    run = next(r for r in RUNS if r["knn"] == 0)
    s = sref.Slim(run["n_users"], run["n_items"], run["cells"])
    live = [j for j in range(s.ni) if s.cols[j]]
    assert len(live) < s.ni and all(lst == live for lst in run["neighbors"])   # train.columns(): the empty item is not in it
    j = live[0]
    t = run["neighbors"][j].index(j)
    assert run["W0"][j][t] == 0.0 and run["W"][1][j][t] != 0.0                  # coordinate i == j IS updated


def test_float_options_widen():
    assert sref.f32(0.1) != 0.1 and sref.f32(0.5) == 0.5
