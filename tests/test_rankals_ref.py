"""tests/rankals_ref.py (the CPU restatement the GPU tests compare against) equals the run of the reference's own RankALS source
(tests/golden/reference_rankals.json.gz, minted by tests/tools/mint_reference_rankals.py) bit for bit: P and Q after every iteration,
the predictions, DenseMatrix.inv() on the table's matrices, initModel()'s draws; and its hoisted form (what the device runs) equals its
literal form bit for bit.  The fixtures of tests/test_gpu_rankals_anchor.py (tests/rankals_fixtures.py) are held to their conditions
here, without a GPU."""
import numpy as np
import pytest

from oracle import oracle_np
from tests import nmf_ref, rankals_fixtures as fx, rankals_ref as rref
from tests.util import same_bits_exact

RUNS = rref.golden_runs()


def test_literal_form_matches_the_reference_run():
    assert [r["name"] for r in RUNS] == ["%s k=%d sw=%s" % (m, k, sw) for m, ks in (("knn_matrix", (3, 10)), ("handmade", (1, 2)))
                                         for k in ks for sw in ("on", "off")]
    for run in RUNS:
        nu, ni = run["n_users"], run["n_items"]
        m = rref.RankALS(nu, ni, run["cells"], run["sw"])
        assert m.users == run["rows"] and [len(r) for r in m.rows] == run["row_count"], run["name"]
        assert same_bits_exact(m.s, run["s"]) and same_bits_exact([m.sum_s], [run["sum_s"]]), run["name"]
        P, Q = run["P0"].copy(), run["Q0"].copy()
        assert len(run["iters"]) == 3
        for n, it in enumerate(run["iters"]):
            m.iterate_literal(P, Q)
            assert same_bits_exact(P, it["P"]), (run["name"], n)
            assert same_bits_exact(Q, it["Q"]), (run["name"], n)
        pred = [[rref.predict(P, Q, u, j) for j in range(ni)] for u in range(nu)]
        assert same_bits_exact(pred, run["predict"]) and same_bits_exact(rref.scores(P, Q), run["predict"]), run["name"]


def test_what_librec_makes_of_the_handmade_matrix():
    """a stored zero takes no part: it is neither in row() / getCount() nor in rows() nor in columnSize().  The user whose only cell is
    a stored zero and the user without a cell keep their drawn rows; the item without a cell is solved"""
    run = next(r for r in RUNS if r["name"] == "handmade k=2 sw=on")
    assert run["rows"] == [0, 1, 2, 3, 4] and run["row_count"] == [3, 2, 1, 2, 3, 0, 0]
    assert run["column_size"] == [3, 2, 2, 2, 2, 0] and run["s"].tolist() == [3.0, 2.0, 2.0, 2.0, 2.0, 0.0]
    it = run["iters"][0]
    assert same_bits_exact(it["P"][5:], run["P0"][5:]) and not same_bits_exact(it["P"][2], run["P0"][2])
    assert not same_bits_exact(it["Q"][5], run["Q0"][5])
    off = next(r for r in RUNS if r["name"] == "handmade k=2 sw=off")
    assert off["s"].tolist() == [1.0] * 6 and off["sum_s"] == 6.0


def test_hoisted_form_equals_the_literal_form():
    for run in RUNS:
        m = rref.RankALS(run["n_users"], run["n_items"], run["cells"], run["sw"])
        P, Q = run["P0"].copy(), run["Q0"].copy()
        for n, it in enumerate(run["iters"]):
            m.iterate(P, Q)
            assert same_bits_exact(P, it["P"]) and same_bits_exact(Q, it["Q"]), (run["name"], n)


def test_hoisted_form_equals_the_literal_form_on_a_random_matrix():
    rng = np.random.default_rng(20261108)
    nu, ni, k = 40, 30, 5
    cells = [(u, j, float(rng.integers(-1, 6))) for u in range(nu) for j in range(ni) if rng.random() < 0.2]
    assert any(v == 0.0 for _, _, v in cells) and any(v < 0 for _, _, v in cells)
    for sw in (True, False):
        m = rref.RankALS(nu, ni, cells, sw)
        Pa, Qa = 0.1 * rng.standard_normal((nu, k)), 0.1 * rng.standard_normal((ni, k))
        Pb, Qb = Pa.copy(), Qa.copy()
        for _ in range(2):
            m.iterate_literal(Pa, Qa)
            m.iterate(Pb, Qb)
            assert same_bits_exact(Pa, Pb) and same_bits_exact(Qa, Qb)


def test_inv_matches_the_table():
    table = rref.golden_inv()
    assert {c["name"] for c in table} >= {"row_swap", "pivot_tie", "zero_column_0", "zero_column_1", "n1_zero", "nan_entry", "well_10x10"}
    for c in table:
        assert same_bits_exact(rref.inv(c["A"]), c["inv"]), c["name"]
    by = {c["name"]: c for c in table}
    assert by["singular_2x2"]["inv"].tolist() == [[0.0, 0.5], [1.0, -0.5]]          # the early return: I as it stands
    assert by["zero_column_0"]["inv"].tolist() == np.eye(3).tolist() and by["n1_zero"]["inv"][0, 0] == np.inf
    assert np.isnan(by["nan_entry"]["inv"]).any() and by["nan_pivot_column"]["inv"].tolist() == np.eye(2).tolist()


def test_init_model_draws():
    g = rref.golden()["init"]
    nu, ni, k = g["n_users"], g["n_items"], g["k"]
    P, Q = rref.init_model(oracle_np.JavaRandom(g["seed"]), nu, ni, k)
    assert same_bits_exact(P, rref.unhex(g["P"], nu, k)) and same_bits_exact(Q, rref.unhex(g["Q"], ni, k))
    m = rref.RankALS(nu, ni, [(c[0], c[1], float.fromhex(c[2])) for c in g["cells"]], g["sw"])
    assert same_bits_exact(m.s, rref.unhex(g["s"], ni)) and same_bits_exact([m.sum_s], [float.fromhex(g["sum_s"])])


def test_array_form_for_large_matrices_equals_the_list_form():
    """from_csr, UserSums and user_moments_fast (what tools/bench_rankals.py restates samples with) give the bits of the plain form"""
    rng = np.random.default_rng(20261111)
    nu, ni, k = 40, 30, 4
    cells = [(u, j, float(rng.integers(-1, 6))) for u in range(nu) for j in range(ni) if rng.random() < 0.25]
    u, i, r = (np.array(x) for x in zip(*cells))
    rows, cols = nmf_ref.rows_of(u, i, r, nu), nmf_ref.cols_of(u, i, r, ni)
    a, b = rref.RankALS(nu, ni, cells, True), rref.from_csr(nu, ni, rows, cols, True)
    assert a.users == b.users and same_bits_exact(a.s, b.s) and a.sum_s == b.sum_s
    Pa, Qa = 0.1 * rng.standard_normal((nu, k)), 0.1 * rng.standard_normal((ni, k))
    Pb, Qb = Pa.copy(), Qa.copy()
    sum_sq, m = a.p_step(Pa, Qa)
    ms = rref.UserSums(b, Qb, rows)
    for x in a.users:
        assert same_bits_exact(np.concatenate([m[x][:3], m[x][3]]), np.concatenate([ms[x][:3], ms[x][3]])), x
    b.p_step(Pb, Qb)
    assert same_bits_exact(Pa, Pb)
    mom_a, mom_b = a.user_moments(Pa, m), rref.user_moments_fast(b, Pb, ms)
    assert all(same_bits_exact(x, y) for x, y in zip(mom_a, mom_b))
    for j in range(ni):
        assert same_bits_exact(a.solve_item(Pa, m, sum_sq, mom_a, j), b.solve_item(Pb, ms, sum_sq, mom_b, j)), j


# ---- the fixtures of tests/test_gpu_rankals_anchor.py -----------------------------------------------------------------------------------
def test_per_is_derived_from_the_kernels_constants():
    c = fx.kernel_constants()
    assert c["RANKALS_MAX_K"] == 64 and c["RANKALS_CHUNK"] == 64 and c["RANKALS_STAGE_MIN"] == 1024 and c["RANKALS_TILE"] == 16
    assert [fx.per_of(k) for k in (1, 8, 16, 17, 32, 33, 63, 64)] == [64, 64, 64, 60, 32, 33, 63, 64]
    assert all(fx.per_of(k) != c["RANKALS_CHUNK"] for k in fx.BORDER_KS[1:])       # the staging borders no other test puts an entry on


@pytest.mark.parametrize("k", fx.BORDER_KS)
def test_per_border_matrix_has_the_borders(k):
    per, tile = fx.per_of(k), fx.kernel_constants()["RANKALS_TILE"]
    nu, ni, cells = fx.per_border_matrix(k)
    for sw in (True, False):
        m = rref.RankALS(nu, ni, cells, sw)
        ul, il = [len(x) for x in m.rows], [len(x) for x in m.cols]
        assert ul[1:4] == [per, per + 1, 2 * per] and il[1:4] == [per, per + 1, 2 * per]
        assert ni % tile == 0 and len(m.users) % tile == 0 and m.users == list(range(nu))       # every last pass is a full tile
        assert max(ul[:1] + ul[4:]) < per and max(il[:1] + il[4:]) < per and min(ul) >= 3 and min(il) >= 1
    stored = [(j, v) for u, j, v in cells if u == 3]
    assert len(stored) == 2 * per + 1 and sum(1 for _, v in stored if v == 0.0) == 1 and sum(1 for _, v in stored if v < 0) == 1
    assert [j for j, v in m.rows[3]].index(next(j for j, v in stored if v < 0)) == per          # it opens the second staged chunk
    assert all(v > 0 for u, _, v in cells if u != 3)
    P0, Q0, out = fx.per_border_run(k, True)
    assert all(np.isfinite(P).all() and np.isfinite(Q).all() for P, Q in out)
