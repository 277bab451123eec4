"""The CPU restatement (tests/knn_ref.py) reproduces, bit for bit, what the reference itself computed (tests/golden/reference_knn.json.gz,
minted by tests/tools/mint_reference_knn.py): happy.coding.math.Sims run from its bytecode on hand-made, DePaul and Frappe common
lists; and ItemKNN / UserKNN run from their source -- every similarity measure through Recommender.correlation (shrinkage, cos-binary,
an unknown measure name), the means, and predict(u, j, c, true) for every (u, j) at several knn, the HashMap order included."""
import gzip
import json
import math
import os

import numpy as np
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


class _Row:
    """one similarity row S[target] that answers both predict()'s S[target, e] and predict_fast()'s S[target]"""

    def __init__(self, target, row):
        self.target, self.row = target, row

    def __getitem__(self, key):
        if isinstance(key, tuple):
            assert key[0] == self.target
            return self.row[key[1]]
        assert key == self.target
        return self.row


def _adversarial_ids(rng, m):
    """m distinct ascending ids that crowd HashMap buckets: residues of 16..512, low / high halves of jhash, small-table bins first"""
    style = rng.integers(0, 5)
    if style == 0:  # plain random
        ids = rng.choice(4 * m + 64, size=m, replace=False)
    elif style == 1:  # a crowded residue class of 16..512, among random fillers
        mod = int(rng.choice([16, 32, 64, 128, 256, 512]))
        c = int(rng.integers(0, mod))
        crowd = c + mod * rng.choice(max(m, 16), size=int(rng.integers(1, 14)), replace=False)
        ids = np.unique(np.r_[crowd, rng.choice(4 * m + 64, size=m, replace=False)])
    elif style == 2:  # ids below and above 65 536, where jhash flips the low bit (k ^ k >>> 16)
        c = int(rng.integers(0, 64)) & ~1
        lo = c + 1 + 64 * rng.choice(64, size=int(rng.integers(0, 10)), replace=False)
        hi = 65536 + c + 64 * rng.choice(64, size=int(rng.integers(0, 10)), replace=False)
        ids = np.unique(np.r_[lo, hi, 65536 + rng.choice(8 * m + 64, size=m, replace=False)])
    elif style == 3:  # the first puts all in one bin of 16 slots (treeifyBin resizes), then fillers
        c = int(rng.integers(0, 16))
        ids = np.unique(np.r_[c + 16 * np.arange(int(rng.integers(8, 20))), 400 + rng.choice(4 * m + 64, size=m, replace=False)])
    else:  # two residue classes mod 64 that split mod 128: crowded at 64 slots, not above
        c = int(rng.integers(0, 64))
        ids = np.unique(np.r_[c + 64 * rng.choice(4 * m + 64, size=m, replace=False), rng.choice(8 * m + 8, size=m // 2 + 1, replace=False)])
    rng.shuffle(ids)
    return np.sort(ids[:m])


def _random_case(rng):
    m = int(300 * rng.random() ** 2) + int(rng.integers(0, 2))
    ids = _adversarial_ids(rng, m)
    n_ent = int(ids.max()) + 2 if len(ids) else 2
    target = n_ent - 1
    style = rng.integers(0, 3)
    if style == 0:
        sims = rng.uniform(-0.2, 1.0, len(ids))
    elif style == 1:  # large tie blocks at the cut
        sims = rng.choice([0.25, 0.5, 0.75, 1.0], len(ids))
    else:
        sims = rng.uniform(0.0, 1.0, len(ids))
    sims[rng.random(len(ids)) < 0.05] = np.nan   # unset
    sims[rng.random(len(ids)) < 0.03] = 0.0
    rates = rng.integers(1, 6, len(ids)).astype(np.float64) / rng.choice([1.0, 2.0, 3.0], len(ids))
    rates[rng.random(len(ids)) < 0.03] = 0.0
    row = np.full(n_ent, np.nan)
    row[ids] = sims
    means = rng.uniform(1.0, 5.0, n_ent)
    cells = list(zip(ids.tolist(), rates.tolist()))
    return _Row(target, row), means, [cells], target


def _same(a, b):
    return a.hex() == b.hex() or (math.isnan(a) and math.isnan(b))


def _both(kind, S, means, lists, u, j, knn, gm, bound):
    out = []
    for f in (knn_ref.predict, knn_ref.predict_fast):
        try:
            out.append(f(kind, S, means, lists, u, j, knn, gm, bound, 1.0, 5.0))
        except knn_ref.Treeified:
            out.append("treeified")
    return out


def test_predict_fast_equals_predict_adversarial():
    """predict_fast == predict (JavaIntHashMap) on 2 000 seeded cases of up to 300 candidates with bucket-crowding ids, at knn in
    {0, 1, 2, m-1, m, m+1, 10^6}: the same bits, and Treeified for exactly the same (case, knn)"""
    rng = np.random.default_rng(20261015)
    seen = {"treeified": 0, "cut": 0, "m>=64": 0}
    for case in range(2000):
        S, means, lists, target = _random_case(rng)
        kind = "item" if case % 2 == 0 else "user"
        u, j = (0, target) if kind == "item" else (target, 0)
        m = sum(1 for e, r in lists[0] if S.row[e] > 0 and r > 0)
        seen["m>=64"] += m >= 64
        for knn in sorted({0, 1, 2, max(m - 1, 0), m, m + 1, 10 ** 6}):
            want, got = _both(kind, S, means, lists, u, j, knn, 3.5, case % 3 == 0)
            assert (want == "treeified") == (got == "treeified"), (case, knn, want, got)
            if want == "treeified":
                seen["treeified"] += 1
            else:
                assert _same(got, want), (case, knn, want, got)
                seen["cut"] += 0 < knn < m
    print(seen)
    assert seen["treeified"] >= 50 and seen["cut"] >= 1000 and seen["m>=64"] >= 500


@pytest.mark.parametrize("model", ["ItemKNN", "UserKNN"])
def test_predict_fast_equals_predict_reference_matrix(model):
    """every tuple of the reference run's matrix, for every measure of the fixture, at knn in {0, 1, 2, m-1, m, m+1, 10^6}"""
    nu, ni, u, i, r = _knn_matrix()
    kind = "item" if model == "ItemKNN" else "user"
    rows = knn_ref.rows_of(u, i, r, kind, nu, ni)
    lists = knn_ref.lists_of(u, i, r, kind, nu, ni)
    for run in [m for m in _golden()["models"] if m["model"] == model]:
        gm = float.fromhex(run["global_mean"])
        S = knn_ref.build_corrs(rows, nu if kind == "item" else ni, run["measure"], run["shrinkage"])
        means = knn_ref.row_means(rows, gm)
        for a in range(nu):
            for b in range(ni):
                owner, target = (a, b) if kind == "item" else (b, a)
                m = sum(1 for e, v in lists[owner] if S[target, e] > 0 and v > 0)
                for knn in sorted({0, 1, 2, max(m - 1, 0), m, m + 1, 10 ** 6}):
                    want, got = _both(kind, S, means, lists, a, b, knn, gm, True)
                    assert want != "treeified" and got != "treeified"
                    assert _same(got, want), (run["measure"], run["shrinkage"], knn, a, b)
