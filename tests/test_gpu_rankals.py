"""RankALS on the GPU through the C ABI: P, Q and every score bit for bit against the run of the reference's own source
(tests/golden/reference_rankals.json.gz) and, on a generated matrix that takes every path of the kernels, against the CPU restatement
(tests/rankals_ref.py); the device inversion against librec's DenseMatrix.inv(); top-N lists and measures against selections from the
restatement's scores; run-to-run reproducibility; the refusals; and the driver's ranking measures on DePaul (cv -k 5) against the
restatement over the same folds."""
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from carskit_amd import capi, dao
from oracle import oracle_np, rank_oracle
from tests import rankals_ref as rref
from tests.hostmirror import splitter
from tests.util import assert_same_rankings, same_bits, same_bits_exact, to2d, with_env

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carskit_amd", "bin", "carskit-mi355x")
GOLDEN = os.path.join(ROOT, "tests", "golden")

CHUNK = 64    # RANKALS_CHUNK: entries of a row or column staged per pass
RUNS = rref.golden_runs()


def all_tuples(nu, ni):
    return np.repeat(np.arange(nu, dtype=np.int32), ni), np.tile(np.arange(ni, dtype=np.int32), nu)


def instance(k, nu, ni, cells, P=None, Q=None):
    h = capi.RankALSInstance(k, nu, ni)
    h.set_ratings([c[0] for c in cells], [c[1] for c in cells], [c[2] for c in cells])
    if P is not None:
        h.set_model(P, Q)
    return h


@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_golden_runs_match_the_reference_run(run):
    nu, ni = run["n_users"], run["n_items"]
    h = instance(run["k"], nu, ni, run["cells"], run["P0"], run["Q0"])
    for n, it in enumerate(run["iters"]):
        h.iterate(run["sw"])
        P, Q = h.model()
        assert same_bits_exact(P, it["P"]), (n, np.argwhere(P != it["P"])[:5])
        assert same_bits_exact(Q, it["Q"]), (n, np.argwhere(Q != it["Q"])[:5])
    tu, tj = all_tuples(nu, ni)
    assert same_bits_exact(h.predict(tu, tj).reshape(nu, ni), run["predict"])
    ms = h.last_iter_ms()
    assert len(ms) == 5 and all(x >= 0.0 for x in ms) and sum(ms[:4]) > 0.0
    h.close()


# ---- kernel edges -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_matrix():
    """300 users x 260 items, values m / 3.  User 0 and item 0 are empty; user 1 and item 1 have one entry; user 2 / item 2 exactly CHUNK;
    user 3 / item 3 CHUNK + 1; user 4 and item 4 have 250 entries (three chunks and a part), and user 4's row holds one stored zero
    (a 251st cell, item 5) and one negative value (item 6); the others 5..20 entries."""
    rng = np.random.default_rng(20261109)
    nu, ni = 300, 260
    val = lambda: float(rng.integers(3, 16)) / 3.0  # noqa: E731
    cells = {}
    for u in range(5, nu):
        for j in rng.choice(np.arange(5, ni), int(rng.integers(5, 21)), replace=False).tolist():
            cells[(u, j)] = val()
    for j in range(6, 6 + 250):
        cells[(4, j)] = val()
    cells[(4, 5)] = 0.0
    cells[(4, 6)] = -2.0 / 3.0
    for j, cnt in ((2, CHUNK), (3, CHUNK + 1), (4, 250)):
        for u in rng.choice(np.arange(5, nu), cnt, replace=False).tolist():
            cells[(u, j)] = val()
    cells[(7, 1)] = val()
    for u, cnt in ((1, 1), (2, CHUNK), (3, CHUNK + 1)):
        for j in rng.choice(np.arange(7, ni), cnt, replace=False).tolist():
            cells[(u, j)] = val()
    return nu, ni, sorted((u, j, v) for (u, j), v in cells.items())


def test_edge_matrix_has_the_edges():
    nu, ni, cells = edge_matrix()
    m = rref.RankALS(nu, ni, cells, True)
    ul, il = [len(x) for x in m.rows], [len(x) for x in m.cols]
    assert ul[:5] == [0, 1, CHUNK, CHUNK + 1, 250] and il[:5] == [0, 1, CHUNK, CHUNK + 1, 250]
    assert (4, 5, 0.0) in cells and dict(m.rows[4])[6] < 0 and 5 not in dict(m.rows[4])
    assert m.users == list(range(1, nu)) and 3000 <= len(cells) <= 6000 and min(ul[5:]) >= 5


@functools.lru_cache(maxsize=None)
def edge_reference(k, sw):
    """the restatement's P and Q after one and two iterations from a seeded start (computed once per (k, sw))"""
    nu, ni, cells = edge_matrix()
    rng = np.random.default_rng(100 + k)
    P0, Q0 = 0.1 * rng.standard_normal((nu, k)), 0.1 * rng.standard_normal((ni, k))
    m = rref.RankALS(nu, ni, cells, sw)
    P, Q, out = P0.copy(), Q0.copy(), []
    for _ in range(2):
        m.iterate(P, Q)
        out.append((P.copy(), Q.copy()))
    return P0, Q0, out


@pytest.mark.parametrize("sw", [True, False], ids=["sw_on", "sw_off"])
@pytest.mark.parametrize("k", [1, 2, 10, 33, 64])
def test_kernel_edges(k, sw):
    """k = 1: inv's n = 1 branch; 2: the smallest elimination; 10: the default; 33: no multiple of any lane tile; 64: the LDS limit"""
    nu, ni, cells = edge_matrix()
    P0, Q0, want = edge_reference(k, sw)
    h = instance(k, nu, ni, cells, P0, Q0)
    for n, (Pw, Qw) in enumerate(want):
        h.iterate(sw)
        P, Q = h.model()
        assert same_bits_exact(P, Pw), (n, np.argwhere(P != Pw)[:5])
        assert same_bits_exact(Q, Qw), (n, np.argwhere(Q != Qw)[:5])
    assert same_bits_exact(P[0], P0[0]) and not same_bits_exact(Q[0], Q0[0])   # the empty user keeps its row, the empty item is solved
    h.close()


@functools.lru_cache(maxsize=None)
def zero_column_reference(k, sw):
    """Q[:, 0] = 1 for every item: with q_0 = 1, sum_cqq[a][0] = sum_cq[a], sum_sq[0] = sum_s, sum_cq[0] = sum_c and sum_sqq[a][0] =
    sum_sq[a] as the same chains, so M[a][0] = (cq[a] * sum_s - cq[a] * sum_s) - sq[a] * c + sq[a] * c is exactly 0 for every user
    while y is not: column 0 has no pivot, inv() returns the identity at once and P[u] = y.  Returns Q0, the restatement's P and Q
    after one pass, and per user of rows() the column at which inv() stopped and y."""
    nu, ni, cells = edge_matrix()
    rng = np.random.default_rng(200 + k)
    P0, Q0 = 0.1 * rng.standard_normal((nu, k)), 0.1 * rng.standard_normal((ni, k))
    Q0[:, 0] = 1.0
    m = rref.RankALS(nu, ni, cells, sw)
    sum_sq, sum_sqq = m.item_moments(Q0)
    seen = {}
    for u in m.users:
        cqq, cq, cqr, sqr, sum_sr, sum_cr, sum_c = m.user_sums(Q0, u)
        M = cqq * m.sum_s - np.outer(cq, sum_sq) - np.outer(sum_sq, cq) + sum_sqq * sum_c
        y = cqr * m.sum_s - cq * sum_sr - sum_sq * sum_cr + sqr * sum_c
        stopped = []
        rref.inv(M, stopped)
        seen[u] = (M, stopped, y)
    P, Q = P0.copy(), Q0.copy()
    m.iterate(P, Q)
    return P0, Q0, P, Q, seen


@pytest.mark.parametrize("sw", [True, False], ids=["sw_on", "sw_off"])
@pytest.mark.parametrize("k", [2, 10, 64])
def test_user_solve_whose_first_column_has_no_pivot(k, sw):
    """the early return of the inversion at column 0 in every user's solve, with a non-zero y: the new row is y itself, and the room of
    `mat` is reused for it right after the routine returns"""
    nu, ni, cells = edge_matrix()
    P0, Q0, Pw, Qw, seen = zero_column_reference(k, sw)
    for u, (M, stopped, y) in seen.items():
        assert not M[:, 0].any() and stopped == [0], u
        assert same_bits_exact(Pw[u], y), u
    assert sum(1 for _, _, y in seen.values() if y[0] != 0.0) > len(seen) // 2 and all(y[1:].any() for _, _, y in seen.values())
    h = instance(k, nu, ni, cells, P0, Q0)
    h.iterate(sw)
    P, Q = h.model()
    assert same_bits_exact(P, Pw), np.argwhere(P != Pw)[:5]
    assert same_bits(Q, Qw), np.argwhere(Q != Qw)[:5]       # (a NaN of the Q step, if any, stands where the restatement has one)
    h.close()


# ---- the inversion ------------------------------------------------------------------------------------------------------------------
# Every double that is a number, an infinity or a zero must have the reference's bits; a NaN must stand where the reference has a NaN.
# Which NaN is not compared: IEEE 754 leaves the sign and payload of a generated NaN to the platform (the host that minted the table
# generates the negative quiet NaN, gfx950 the positive one), and Java's own Double.doubleToLongBits collapses every NaN to one pattern.
def test_inversion_matches_the_golden_table():
    h = capi.RankALSInstance(2, 2, 2)
    for c in rref.golden_inv():
        got = h.invert(c["A"][None])[0]
        assert same_bits(got, c["inv"]), (c["name"], got, c["inv"])
        if not np.isnan(c["inv"]).any():
            assert same_bits_exact(got, c["inv"]), c["name"]
    h.close()


def inversion_batch(n, count=200):
    """random matrices; every fifth gets a duplicated row scaled by a power of two, every fifth (offset 1) equal magnitudes in a pivot
    column (the first of them must win), every fifth (offset 2; n >= 3) a lower-left zero block whose last column is zero too, so that
    the column after the block has no pivot and the identity comes back as it stands mid-way"""
    rng = np.random.default_rng(5000 + n)
    A = rng.standard_normal((count, n, n))
    for t in range(count):
        if t % 5 == 0:
            a, b = rng.choice(n, 2, replace=False).tolist()
            A[t, b] = A[t, a] * 2.0 ** int(rng.integers(-3, 4))
        elif t % 5 == 1:
            c = int(rng.integers(0, n))
            rows = rng.choice(np.arange(c, n), min(2, n - c), replace=False)
            A[t, rows, c] = np.abs(A[t, :, c]).max() * 1.5 * rng.choice([-1.0, 1.0], len(rows))
        elif t % 5 == 2 and n >= 3:
            b = int(rng.integers(1, n - 1))
            A[t, b:, :b + 1] = 0.0
    return A


@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 9, 10, 16, 17, 32, 33, 64])
def test_inversion_batch_matches_the_restatement(n):
    A = inversion_batch(n)
    stopped, want = [], np.empty_like(A)
    for t in range(len(A)):
        want[t] = rref.inv(A[t], stopped)
    if n >= 3:
        assert len(stopped) >= 30 and min(stopped) >= 1      # the early return, mid-way
    h = capi.RankALSInstance(2, 2, 2)
    got = h.invert(A)
    bad = [t for t in range(len(A)) if not same_bits(got[t], want[t])]
    assert not bad, (n, bad[:10])
    h.close()


# ---- reproducibility ---------------------------------------------------------------------------------------------------------------
def test_same_model_same_bits():
    nu, ni, cells = edge_matrix()
    P0, Q0, _ = edge_reference(10, True)
    h = instance(10, nu, ni, cells)
    out = []
    for _ in range(2):
        h.set_model(P0, Q0)
        h.iterate(True)
        h.iterate(True)
        out.append(h.model())
    assert same_bits_exact(out[0][0], out[1][0]) and same_bits_exact(out[0][1], out[1][1])
    h.close()


# ---- top-N -------------------------------------------------------------------------------------------------------------------------
def check_rankings(h, scores, train, test, tol=1e-12, **kw):
    """lists (items and scores) exactly those selected from `scores`; the 21 measures within the tolerance tests/test_gpu_ranking.py
    uses for fp64 state"""
    res, lists = h.eval_rankings(train, test, with_lists=True, **kw)
    thold, num_recs = kw.get("bin_thold", -1.0), kw.get("num_recs", 10)
    cand, queries = capi.rank_plan(h.n_users, h.n_items, train, test, thold, kw.get("num_ignore", 0))
    want = rref.top_lists(cand, queries, scores, thold, num_recs)
    assert set(lists) == set(want) and len(want) > 0
    for key in want:
        assert [i for i, _ in lists[key]] == [i for i, _ in want[key]], key
        assert same_bits_exact([s for _, s in lists[key]], [s for _, s in want[key]]), key
    tup = lambda d: list(zip(*[np.asarray(a).tolist() for a in d]))  # noqa: E731
    ref, ref_lists = rank_oracle.eval_rankings(lambda u, j, c: float(scores[u, j]), tup(train), tup(test), **kw)
    assert ref_lists == want
    for m in rank_oracle.MEASURES:
        a, b = res[m], ref[m]
        print("%s gpu %r ref %r" % (m, a, b))
        assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol, (m, a, b)
    assert res["D5"] == res["D10"] == res["DN"] == 0.0
    return lists


def contextual_split(cells, n_ctx, seed, test_share=0.25):
    """(u, j, ctx, r) train and test tuples over the cells of a 2-D matrix: a cell appears in one to three contexts"""
    rng = np.random.default_rng(seed)
    tr, te = [], []
    for u, j, v in cells:
        for c in rng.choice(n_ctx, int(rng.integers(1, 4)), replace=False).tolist():
            (te if rng.random() < test_share else tr).append((u, j, c, v if v != 0.0 else 1.0))
    arr = lambda ts: (np.array([t[0] for t in ts], np.int32), np.array([t[1] for t in ts], np.int32),  # noqa: E731
                      np.array([t[2] for t in ts], np.int32), np.array([t[3] for t in ts]))
    return arr(sorted(tr)), arr(sorted(te))


# (the split's seed: one with which every setting below leaves at least one list, also on the 7 x 6 matrix with its 3 ignored items)
@pytest.mark.parametrize("name,seed", [("knn_matrix k=3 sw=on", 11), ("knn_matrix k=10 sw=off", 11), ("handmade k=2 sw=on", 14)])
def test_eval_rankings_on_golden_models(name, seed):
    run = next(r for r in RUNS if r["name"] == name)
    h = instance(run["k"], run["n_users"], run["n_items"], run["cells"], run["iters"][-1]["P"], run["iters"][-1]["Q"])
    scores = run["predict"]                                     # the golden scores belong to the last iteration's model
    with pytest.raises(capi.CmiError) as e:
        h.last_iter_ms()                                        # neither an iteration nor an evaluation yet
    assert e.value.code == capi.E_INVALID
    train, test = contextual_split(run["cells"], 4, seed)
    for kw in (dict(bin_thold=-1.0, num_recs=10), dict(bin_thold=-1.0, num_recs=5, strategy="uc"), dict(bin_thold=0.05, num_recs=10, num_ignore=3)):
        check_rankings(h, scores, train, test, **kw)
    ms = h.last_iter_ms()                                       # an evaluation without an iteration: the fifth time alone
    assert ms[:4] == (0.0, 0.0, 0.0, 0.0) and ms[4] > 0.0
    h.close()


@functools.lru_cache(maxsize=None)
def score_model(k=10):
    """8 users x 520 items at k factors, drawn; user 7 has no train cell and a zero row: every score 0.0, ties in candidate order"""
    rng = np.random.default_rng(20261110)
    nu, ni = 8, 520
    P, Q = rng.standard_normal((nu, k)), rng.standard_normal((ni, k))
    P[7] = 0.0
    return nu, ni, k, P, Q, rref.scores(P, Q)


@functools.lru_cache(maxsize=None)
def score_split(n_cand):
    """(train, test, cells) over score_model()'s 8 x 520 matrix with n_cand candidates, the items of the training tuples: user 4 has
    four contexts with a different exclusion set in each, user 7 no train cell; every case of one n_cand shares these arrays"""
    nu, ni = 8, 520
    rng = np.random.default_rng(n_cand)
    cand = sorted(rng.choice(ni, n_cand, replace=False).tolist())
    tr, te = [], []
    for p, j in enumerate(cand):                                   # the candidates are the items of the training tuples
        tr.append((int(rng.integers(0, nu - 1)), j, int(rng.integers(0, 4))))
    for c in range(4):                                             # user 4: four contexts, a different exclusion set in each
        for j in cand[c::7]:
            tr.append((4, j, c))
    tr = sorted(set(tr))
    seen = set(tr)
    for u in range(nu):
        for c in range(4):
            for j in rng.choice(cand, 3, replace=False).tolist():
                if (u, j, c) not in seen:
                    te.append((u, j, c, 5.0))
    train = tuple(np.array(x, dt) for x, dt in zip(zip(*[(u, j, c, 3.0) for u, j, c in tr]), (np.int32, np.int32, np.int32, np.float64)))
    test = tuple(np.array(x, dt) for x, dt in zip(zip(*sorted(set(te))), (np.int32, np.int32, np.int32, np.float64)))
    cells = sorted(set((u, j, 3.0) for u, j, _ in tr))
    assert not any(u == 7 for u, _, _ in cells)
    return train, test, cells


def check_score_kernel_and_selection_edges(factory, k, n_cand, num_recs):
    """`factory(k, nu, ni, cells, P, Q)` returns a handle of a factor model whose predict is rowMult, with the cells and the model set
    and no iteration run.  Its predict over all 8 x 520 cells and its evaluation of score_split(n_cand) (lists, score bits, measures,
    whole and in batches of 3 queries) against the restatement's scores of score_model(k)."""
    nu, ni, k, P, Q, scores = score_model(k)
    train, test, cells = score_split(n_cand)
    h = factory(k, nu, ni, cells, P, Q)
    tu, tj = all_tuples(nu, ni)
    assert same_bits_exact(h.predict(tu, tj).reshape(nu, ni), scores)
    lists = check_rankings(h, scores, train, test, bin_thold=-1e9, num_recs=num_recs)
    plan_cand, queries = capi.rank_plan(nu, ni, train, test, -1e9, 0)
    assert len(plan_cand) == n_cand
    ex4 = {c: tuple(e) for u, c, _, e in queries if u == 4}
    assert len(ex4) == 4 and len(set(ex4.values())) == 4           # one group of four queries, four exclusion lists
    assert max(len(v) for v in lists.values()) == min(num_recs, max(n_cand - len(e) for _, _, _, e in queries))
    seven = [v for key, v in lists.items() if key[0] == 7]
    assert seven and all([i for i, _ in v] == plan_cand[:len(v)] for v in seven)   # every score 0.0: candidate order
    batched = with_env(lambda: h.eval_rankings(train, test, bin_thold=-1e9, num_recs=num_recs, with_lists=True), CMI_RANK_BATCH=3)
    assert batched[1] == lists                                     # batches that cut user 4's group: the same lists
    h.close()


@pytest.mark.parametrize("n_cand,num_recs", [(63, 10), (64, 70), (65, 10), (513, 70), (513, 10)])
def test_score_kernel_and_selection_edges(n_cand, num_recs):
    """63, 64, 65 and 513 candidates (513: three blocks of the score kernel); lists of 10 (the streaming selection) and 70 (one pass per
    rank); a user with four contexts whose exclusions differ; a user without a row.  The factor counts up to the kernel's limit, the
    block border and the selection switch, for this model and the three that share the kernel: tests/test_gpu_topn_score_edges.py"""
    check_score_kernel_and_selection_edges(instance, 10, n_cand, num_recs)


def test_a_reused_handle_answers_like_a_fresh_one():
    """One handle evaluates split A, A again (the plan's arrays resident), A in batches of 7 queries, another split B (a new plan), A
    again, then iterates and evaluates A; every result equals, entry for entry, that of a handle that has evaluated nothing before."""
    run = next(r for r in RUNS if r["name"] == "knn_matrix k=10 sw=on")

    def handle(model):
        return instance(run["k"], run["n_users"], run["n_items"], run["cells"], model["P"], model["Q"])

    def evaluate(h, split, batch):
        return with_env(lambda: h.eval_rankings(split[0], split[1], bin_thold=-1.0, num_recs=10, with_lists=True), CMI_RANK_BATCH=batch)

    A, B = contextual_split(run["cells"], 4, 11), contextual_split(run["cells"], 4, 12)
    one, fresh = handle(run["iters"][0]), []
    for n, (split, batch) in enumerate([(A, None), (A, None), (A, 7), (B, None), (A, None)], 1):
        new = handle(run["iters"][0])
        fresh.append(evaluate(new, split, batch))
        new.close()
        assert_same_rankings(evaluate(one, split, batch), fresh[-1], "step %d" % n)
    assert len(fresh[0][1]) > 0 and fresh[0][1].keys() != fresh[3][1].keys()
    one.iterate(run["sw"])                                         # the second iteration, on the used handle
    new = handle(run["iters"][1])
    assert same_bits_exact(one.model()[0], run["iters"][1]["P"]) and same_bits_exact(one.model()[1], run["iters"][1]["Q"])
    assert_same_rankings(evaluate(one, A, None), evaluate(new, A, None), "after iterate")
    new.close()
    one.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    with pytest.raises(capi.CmiError) as e:
        capi.RankALSInstance(65, 3, 3)
    assert e.value.code == capi.E_UNSUPPORTED and "k <= 64" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        capi.RankALSInstance(2, 2, 0)
    assert e.value.code == capi.E_INVALID
    h = capi.RankALSInstance(2, 3, 3)
    with pytest.raises(capi.CmiError) as e:
        h.set_ratings([0, 0], [1, 1], [1.0, 2.0])
    assert e.value.code == capi.E_INVALID and "duplicate" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        h.set_ratings([0, 3], [0, 1], [1.0, 2.0])
    assert e.value.code == capi.E_INVALID and "out of range" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        h.iterate(True)
    assert e.value.code == capi.E_INVALID and "cmi_rankals_set_ratings first" in str(e.value)
    for call in (h.model, lambda: h.predict([0], [1]), h.last_iter_ms):
        with pytest.raises(capi.CmiError) as e:
            call()
        assert e.value.code == capi.E_INVALID
    h.set_ratings([0, 1, 2, 0], [1, 1, 0, 0], [1.0, 2.0, 3.0, 2.0])
    with pytest.raises(capi.CmiError) as e:
        h.iterate(True)
    assert e.value.code == capi.E_INVALID and "cmi_rankals_set_model first" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        h.set_model(np.zeros((3, 2)), None)                          # the first call sets both
    assert e.value.code == capi.E_INVALID
    with pytest.raises(capi.CmiError) as e:
        h.set_model(np.zeros((3, 3)), np.zeros((3, 2)))
    assert e.value.code == capi.E_INVALID and "shape" in str(e.value)
    h.set_model(np.ones((3, 2)), np.ones((3, 2)))
    with pytest.raises(capi.CmiError) as e:
        h.predict([0], [3])
    assert e.value.code == capi.E_INVALID
    with pytest.raises(capi.CmiError) as e:
        h.invert(np.zeros((1, 65, 65)))
    assert e.value.code == capi.E_UNSUPPORTED and "n <= 64" in str(e.value)
    h.iterate(False)                                                 # the handle still works
    assert np.isfinite(h.model()[0]).all()
    h.close()


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def _driver_conf(tmp_path, threshold, extra=""):
    shutil.copyfile(os.path.join(GOLDEN, "depaul_ratings_compact.csv"), tmp_path / "ratings.txt")
    conf = open(os.path.join(GOLDEN, "depaul_setting.conf")).read().replace("PLACEHOLDER_SET_BY_TEST", str(tmp_path / "ratings.txt"))
    assert "num.max.iter=100" in conf and "num.factors=10" in conf and "--rand-seed 1" in conf and "item.ranking=off" in conf
    assert "-threshold -1" in conf and "-verbose off" in conf
    conf = conf.replace("recommender=biasedmf", "recommender=rankals").replace("num.max.iter=100", "num.max.iter=4")
    conf = conf.replace("-threshold -1", "-threshold %s" % threshold).replace("-verbose off", "-verbose off" + extra)
    (tmp_path / "rankals.conf").write_text(conf + "RankALS=-sw on\n")
    return str(tmp_path / "rankals.conf")


def test_driver_parity_depaul(tmp_path):
    """cv -k 5, num.max.iter = 4: three iterations a fold (the loop is `iter < numIters`), evaluated as a top-N run although
    item.ranking is off; --save-model leaves P and Q of every fold in the MF classes' file format"""
    k = 10
    p = subprocess.run([EXE, "-c", _driver_conf(tmp_path, "0", " --save-model"), "--precise"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    m = re.search(r"PRECISE RankALS folds=5 Pre10=(\S+) Rec10=(\S+) AUC10=(\S+) MAP10=(\S+) NDCG10=(\S+) MRR10=(\S+)", p.stdout)
    assert m and "Final Results by RankALS, Pre5: " in p.stdout, p.stdout[-500:]
    dao.transform(str(tmp_path / "ratings.txt"), str(tmp_path / "train.csv"))
    d = dao.DataDAO(str(tmp_path / "train.csv")).rating_data()
    labels, nf = splitter.split_folds(d.n, 5, 1)
    want = {}
    for f in range(1, nf + 1):
        tr, te = splitter.kth_fold(d, labels, f)
        u, i, r = to2d(tr.u, tr.j, tr.r)
        model = rref.RankALS(d.n_users, d.n_items, list(zip(u.tolist(), i.tolist(), r.tolist())), True)
        P, Q = rref.init_model(oracle_np.JavaRandom(1), d.n_users, d.n_items, k)
        for _ in range(3):
            model.iterate(P, Q)
        scores = rref.scores(P, Q)
        tup = lambda x: list(zip(x.u.tolist(), x.j.tolist(), x.ctx.tolist(), x.r.tolist()))  # noqa: E731
        res, _ = rank_oracle.eval_rankings(lambda a, b, c: float(scores[a, b]), tup(tr), tup(te), bin_thold=0.0, num_recs=10)
        for name in ("Pre10", "Rec10", "AUC10", "MAP10", "NDCG10", "MRR10"):
            want[name] = want.get(name, 0.0) + res[name] / nf
    for g, name in zip(m.groups(), ("Pre10", "Rec10", "AUC10", "MAP10", "NDCG10", "MRR10")):
        print(name, g, want[name])
        assert abs(float(g) - want[name]) <= 1e-12, (name, g, want[name])
    saved = tmp_path / "CARSKit.Workspace" / "RankALS" / ("model fold [%d].cmi" % nf)      # the last fold's model, still in P and Q
    assert saved.exists(), os.listdir(tmp_path / "CARSKit.Workspace")
    pmf = capi.Instance("PMF", k, d.n_users, d.n_items, 0, flags=capi.FLAG_STATE_F64)
    pmf.load_model(str(saved))
    assert same_bits_exact(pmf.get_state("P").reshape(P.shape), P) and same_bits_exact(pmf.get_state("Q").reshape(Q.shape), Q)
    pmf.close()


def test_driver_refuses_a_negative_threshold(tmp_path):
    p = subprocess.run([EXE, "-c", _driver_conf(tmp_path, "-1")], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "Final Results" not in p.stdout
    assert "val.binary.threshold=-1.0, ratings must be binarized first! Try set a non-negative value." in p.stderr, p.stderr
