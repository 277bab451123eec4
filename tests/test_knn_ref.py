"""The CPU restatement (tests/knn_ref.py) reproduces, bit for bit, what the reference itself computed (tests/golden/reference_knn.json.gz,
minted by tests/tools/mint_reference_knn.py): happy.coding.math.Sims run from its bytecode on hand-made, DePaul and Frappe common
lists; and ItemKNN / UserKNN run from their source -- every similarity measure through Recommender.correlation (shrinkage, cos-binary,
an unknown measure name), the means, and predict(u, j, c, true) for every (u, j) at several knn, the HashMap order included."""
import gzip
import json
import math
import os

import pytest

from tests import knn_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_knn.json.gz")


def _golden():
    return json.loads(gzip.open(GOLDEN, "rb").read())


def _cases():
    return _golden()["cases"]


@pytest.mark.parametrize("method", ["pcc", "cos", "msd", "cpc", "exjaccard"])
def test_sims_bit_exact_to_bytecode(method):
    cases = _cases()
    assert len(cases) > 50
    seen_inf = False
    for c in cases:
        a = [float.fromhex(x) for x in c["a"]]
        b = [float.fromhex(x) for x in c["b"]]
        got = knn_ref.sims(method, a, b, float.fromhex(c["median"]))
        want = c[method]
        if want == "nan":
            assert math.isnan(got), (method, c)
        else:
            assert got.hex() == want, (method, c, got.hex())
            seen_inf |= math.isinf(float.fromhex(want))
    if method == "cos":
        assert seen_inf  # the hand-made underflow pairs give +-Infinity


def _knn_matrix():
    km = _golden()["knn_matrix"]
    u = [c[0] for c in km["cells"]]
    i = [c[1] for c in km["cells"]]
    r = [float.fromhex(c[2]) for c in km["cells"]]
    return km["n_users"], km["n_items"], u, i, r


def test_frappe_pairs_present():
    assert sum(1 for c in _cases() if c.get("source") == "frappe") >= 50


@pytest.mark.parametrize("model", ["ItemKNN", "UserKNN"])
def test_similarities_and_means_bit_exact_to_reference_source(model):
    nu, ni, u, i, r = _knn_matrix()
    kind = "item" if model == "ItemKNN" else "user"
    rows = knn_ref.rows_of(u, i, r, kind, nu, ni)
    n = len(rows)
    runs = [m for m in _golden()["models"] if m["model"] == model]
    assert {knn_ref.measure_name(m["measure"]) for m in runs} == set(knn_ref.MEASURES)
    for run in runs:
        S = knn_ref.build_corrs(rows, nu if kind == "item" else ni, run["measure"], run["shrinkage"])
        got = [0.0 if math.isnan(S[a, b]) else float(S[a, b]) for a in range(n) for b in range(a + 1, n)]  # SymmMatrix.get: 0 if unset
        assert [x.hex() for x in got] == run["corrs"], (run["measure"], run["shrinkage"])
        for a in range(n):  # correlation() itself, pair by pair (the scalar statement of the same method)
            for b in range(a + 1, n):
                if rows[a] and rows[b]:
                    c = knn_ref.correlation(rows[a], rows[b], run["measure"], run["shrinkage"])
                    assert (0.0 if math.isnan(c) else c).hex() == run["corrs"][a * n - a * (a + 1) // 2 + (b - a - 1)]
        gm = float.fromhex(run["global_mean"])
        assert [float(x).hex() for x in knn_ref.row_means(rows, gm)] == run["means"]


@pytest.mark.parametrize("model", ["ItemKNN", "UserKNN"])
def test_predictions_bit_exact_to_reference_source(model):
    nu, ni, u, i, r = _knn_matrix()
    kind = "item" if model == "ItemKNN" else "user"
    rows = knn_ref.rows_of(u, i, r, kind, nu, ni)
    lists = knn_ref.lists_of(u, i, r, kind, nu, ni)
    runs = [m for m in _golden()["models"] if m["model"] == model and "predict" in m]
    assert len(runs) == 2
    cut_into_kept_table = 0
    for run in runs:
        gm = float.fromhex(run["global_mean"])
        S = knn_ref.build_corrs(rows, nu if kind == "item" else ni, run["measure"], run["shrinkage"])
        means = knn_ref.row_means(rows, gm)
        for knn, grid in run["predict"].items():
            for a in range(nu):
                for b in range(ni):
                    got = knn_ref.predict(kind, S, means, lists, a, b, int(knn), gm, True, 1.0, 5.0)
                    assert float(got).hex() == grid[a][b], (run["measure"], knn, a, b)
            # the fixture exercises the table clear() keeps: a cut to knn <= 12 of a map that grew to 64 slots
            owner_sizes = [len(lists[o]) for o in range(len(lists))]
            cut_into_kept_table += int(0 < int(knn) <= 12 and max(owner_sizes) > 24)
    if model == "ItemKNN":  # users with 25+ rated items; UserKNN's item lists are shorter (26 users)
        assert cut_into_kept_table > 0
