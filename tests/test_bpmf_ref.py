"""tests/bpmf_ref.py (the CPU restatement the GPU tests compare with) against tests/golden/reference_bpmf.json.gz, which
tests/tools/mint_reference_bpmf.py minted by executing the reference: BPMF.java from source, librec and happy.coding from bytecode.
Every recorded value, bit for bit."""
import numpy as np
import pytest

from tests import bpmf_ref as ref

G = ref.golden()


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False   # (a NaN is a NaN: Java keeps neither its sign nor its payload, and float.hex() records neither)
    return np.array_equal(np.where(np.isnan(a), 0.0, a).view(np.int64), np.where(np.isnan(b), 0.0, b).view(np.int64))


def test_gaussian_stream_equals_happy_coding_randoms():
    g = G["gaussian"]
    r = ref.Stream.seeded(g["seed"])
    assert [r.gaussian().hex() for _ in range(len(g["draws"]))] == g["draws"]


@pytest.mark.parametrize("case", G["gamma"], ids=lambda c: "alpha=%g" % float.fromhex(c["alpha"]))
def test_gamma_equals_the_bytecode(case):
    r = ref.Stream.seeded(case["seed"])
    assert [ref.gamma(r, float.fromhex(case["alpha"]), 2.0).hex() for _ in range(len(case["draws"]))] == case["draws"]


@pytest.mark.parametrize("case", G["cholesky"], ids=lambda c: c["name"])
def test_cholesky_equals_the_bytecode(case):
    n = case["n"]
    A = ref.unhex(case["A"], n, n)
    for fn in (ref.cholesky, ref.cholesky_literal):
        L = fn(A)
        if case["upper"] is None:
            assert L is None
        else:
            assert L is not None and _same(L.T, ref.unhex(case["upper"], n, n)), fn.__name__


def test_cholesky_cases_cover_null_and_a_zero_diagonal():
    by = {c["name"]: c for c in G["cholesky"]}
    assert by["indefinite"]["upper"] is None and by["n1_negative"]["upper"] is None and by["nan_entry"]["upper"] is None
    assert by["semidefinite"]["upper"] is not None and float.fromhex(by["semidefinite"]["upper"][3]) == 0.0   # a zero diagonal: no null
    assert by["n1_zero"]["upper"] == [0.0.hex()]


@pytest.mark.parametrize("case", G["cov"], ids=lambda c: c["name"])
def test_cov_and_column_mean_equal_the_bytecode(case):
    X = ref.unhex(case["X"], case["rows"], case["k"])
    assert _same(ref.column_mean(X), ref.unhex(case["mean"], case["k"]))
    assert _same(ref.cov(X), ref.unhex(case["cov"], case["k"], case["k"]))


@pytest.mark.parametrize("case", G["wishart"], ids=lambda c: "p=%d" % c["p"])
def test_wishart_equals_the_source_method(case):
    p = case["p"]
    r = ref.Stream.seeded(case["seed"])
    W = ref.wishart(r, ref.unhex(case["scale"], p, p), float.fromhex(case["df"]))
    assert _same(W, ref.unhex(case["W"], p, p))
    assert r.gaussian().hex() == case["next_gaussian"]   # the stream stands where the reference's does


def test_wishart_p7_leaves_out_a_term_of_sparse_inner():
    """the p = 7 case (and every run at k = 10) reaches SparseVector.inner over 5 indices, where contains() misses index 4"""
    assert [k for k in range(5) if not ref.contains(list(range(5)), k)] == [4]
    assert [n for n in range(1, 11) if any(not ref.contains(list(range(n)), k) for k in range(n))] == [5, 9, 10]
    assert ref.sparse_inner([1.0] * 5, [1.0] * 5) == 4.0


def test_the_k17_run_reaches_sparse_inner_where_contains_misses_other_indices(monkeypatch):
    """a hyper step at k = 17 calls SparseVector.inner over every length 1 .. 16: besides 5, 9 and 10 (what k = 10 and the p = 7 case
    reach) contains() misses indices at 11 (8, 9, 10) and 13 (12), and the run's P, Q and loss hold those sums to the reference"""
    run = next(r for r in G["runs"] if r["k"] == 17)
    missed = {n: [k for k in range(n) if not ref.contains(list(range(n)), k)] for n in range(1, 17)}
    assert {n: v for n, v in missed.items() if v} == {5: [4], 9: [8], 10: [8, 9], 11: [8, 9, 10], 13: [12]}
    seen, inner = [], ref.sparse_inner
    monkeypatch.setattr(ref, "sparse_inner", lambda a, b: (seen.append(len(a)), inner(a, b))[1])
    nu, k = run["n_users"], run["k"]
    P = ref.unhex(run["P0"], nu, k)
    ref.hyper_side(ref.Stream.seeded(run["seed_gibbs"]), P, ref.inv(ref.cov(P)), ref.column_mean(P))
    assert set(seen) == set(range(1, 17)) and seen.count(11) >= 2 and seen.count(13) >= 2
    assert ref.sparse_inner([1.0] * 11, [1.0] * 11) == 8.0 and ref.sparse_inner([1.0] * 13, [1.0] * 13) == 12.0


@pytest.mark.parametrize("n", [17, 33, 64])
def test_cholesky_and_its_literal_walk_agree_past_the_golden_sizes(n):
    """the golden cases stop at n = 10: above that the row-wise form the runs use is held to the element-by-element walk"""
    b = np.random.default_rng(20261240 + n).standard_normal((n, n))
    A = b @ b.T + n * np.eye(n)
    L, lit = ref.cholesky(A), ref.cholesky_literal(A)
    assert L is not None and lit is not None and _same(L, lit) and not np.isnan(L).any() and (np.diag(L) > 0.0).all()
    A[n - 1, n - 1] = -1.0                                   # no factor: both say so
    assert ref.cholesky(A) is None and ref.cholesky_literal(A) is None


@pytest.mark.parametrize("run", G["runs"], ids=lambda r: "%s-k%d" % (r["name"], r["k"]))
def test_build_model_equals_the_source(run):
    nu, ni, k = run["n_users"], run["n_items"], run["k"]
    cells = ref.golden_cells(run)
    from oracle.oracle_np import JavaRandom
    P, Q = ref.init_model(JavaRandom(run["seed_init"]), nu, ni, k)
    assert _same(P, ref.unhex(run["P0"], nu, k)) and _same(Q, ref.unhex(run["Q0"], ni, k))   # librec's own stream
    m = ref.BPMF(nu, ni, cells, float.fromhex(run["global_mean"]))
    assert [len(r) for r in m.rows] == run["row_count"] and [len(c) for c in m.cols] == run["col_count"]
    rnd = ref.Stream.seeded(run["seed_gibbs"])
    hy = m.init_hyper(P, Q)
    for t, it in enumerate(run["iters"]):
        loss = m.iterate(rnd, P, Q, hy)
        assert _same(P, ref.unhex(it["P"], nu, k)), "P after iteration %d" % (t + 1)
        assert _same(Q, ref.unhex(it["Q"], ni, k)), "Q after iteration %d" % (t + 1)
        assert float(loss).hex() == it["loss"], "loss after iteration %d" % (t + 1)
    want = np.array([[float.fromhex(x) for x in row] for row in run["predict"]])
    got = np.array([[ref.predict(P, Q, m.gm, u, j) for j in range(ni)] for u in range(nu)])
    assert _same(got, want)


def test_handmade_matrix_has_the_edge_rows():
    run = next(r for r in G["runs"] if r["name"] == "handmade")
    assert run["row_count"].count(0) >= 2 and run["col_count"].count(0) >= 1 and 1 in run["row_count"]
    cells = ref.golden_cells(run)
    assert any(v == 0.0 for _, _, v in cells) and any(v < 0.0 for _, _, v in cells)


def test_generated_matrix_has_the_edge_rows_and_both_sides_longer_than_k():
    run = next(r for r in G["runs"] if r["name"] == "generated")
    assert run["k"] == 17 and run["n_users"] > 17 and run["n_items"] > 17 and len(run["iters"]) == 3
    cells = ref.golden_cells(run)
    assert run["row_count"].count(0) == 1 and run["col_count"].count(0) == 1 and sum(1 for _, _, v in cells if v == 0.0) == 1
    per_user = [sum(1 for c in cells if c[0] == u) for u in range(run["n_users"])]
    assert all(4 <= n <= 8 for n in per_user if n) and sum(per_user) > sum(run["row_count"])   # the stored zero is no entry of row()
