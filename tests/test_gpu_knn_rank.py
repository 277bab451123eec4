"""Top-N scores and evaluation of ItemKNN / UserKNN on the GPU: ranking(u, j) against tests/golden/reference_knn_rank.json.gz (the
reference's own run with isRankingPred = true), bit for bit; eval_rankings on the golden models; the score kernel's edges (owner lists
of 0, 1, 63, 64, 65, 130 entries and, for ItemKNN, one more than the LDS staging tile holds; 63, 64, 65 and 513 candidates; lists of 10
and 70; knn 0, 5, 20; a user with four contexts; batches of 3 queries) against the restatement (tests/knn_rank_ref.py) over the
similarities the device built; rating mode untouched by an evaluation; and the refusals."""
import functools

import numpy as np
import pytest

from carskit_amd import capi
from tests import knn_rank_ref, knn_ref, topn_baselines as tb
from tests.test_gpu_knn_predict import Case, Ids, spaced_ids
from tests.test_gpu_rankals import all_tuples, check_rankings, contextual_split, score_split
from tests.util import same_bits_exact, with_env

pytestmark = pytest.mark.gpu

RUNS = tb.knn_rank_runs()
KNN_STAGE = 512  # knn_kernels.hpp: the entries of a user's row ItemKNN stages in LDS


def built(run):
    h = capi.KNNInstance(run["kind"], run["n_users"], run["n_items"])
    h.set_ratings(run["u"], run["i"], run["r"])
    h.build(run["measure"], run["shrinkage"], 1.0, 5.0)
    return h


@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_ranking_matches_the_reference_run(run):
    h = built(run)
    tu, tj = all_tuples(run["n_users"], run["n_items"])
    for knn, want in run["ranking"].items():
        got = h.ranking(tu, tj, knn, run["global_mean"]).reshape(want.shape)
        assert same_bits_exact(got, want), (run["name"], knn, np.argwhere(got != want)[:5])
    h.close()


@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_eval_rankings_on_golden_models(run):
    h = built(run)
    with pytest.raises(capi.CmiError) as e:
        h.last_rank_ms()                                        # no evaluation yet
    assert e.value.code == capi.E_INVALID
    train, test = contextual_split(run["cells"], 4, tb.SPLIT_SEED)
    knns = sorted(run["ranking"])
    for n, kw in enumerate(tb.SETTINGS):
        for knn in (knns[1 + n], knns[-1]):                     # a cut that bites and none
            check_rankings(tb.Scored(h, knn, run["global_mean"]), run["ranking"][knn], train, test, **kw)
    assert h.last_rank_ms() > 0.0
    h.close()


# ---- the score kernel's edges ----------------------------------------------------------------------------------------------------------
EDGE_LENGTHS = {"item": (1, 63, 64, 65, 130, KNN_STAGE + 1, 30, 0), "user": (0, 1, 63, 64, 65, 130)}
EDGE_GM = 3.125


@functools.lru_cache(maxsize=None)
def edge_matrix(kind):
    """A 2-D matrix over 520 items whose query users are 0 .. 7, the users of score_split().  ItemKNN (48 users): user q's row has
    EDGE_LENGTHS["item"][q] items, user 7 none.  UserKNN (140 users): item j's column has EDGE_LENGTHS["user"][j % 20] users for
    j % 20 < 6, user 7 has no cell (no similarity: every score is the global mean).  Ratings are small integers and thirds, so PCC gives
    negative and exactly zero similarities."""
    rng = np.random.default_rng(20261020 + (kind == "user"))
    ni = 520
    nu = 48 if kind == "item" else 140
    cells = {}
    rate = lambda: float(rng.integers(1, 6)) / (3.0 if rng.random() < 0.2 else 1.0)  # noqa: E731
    if kind == "item":
        for u in range(nu):
            n = EDGE_LENGTHS["item"][u] if u < 8 else int(rng.integers(20, 60))
            for j in rng.choice(ni, n, replace=False).tolist():
                cells[(u, j)] = rate()
    else:
        users = np.array([u for u in range(nu) if u != 7])
        for j in range(ni):
            n = EDGE_LENGTHS["user"][j % 20] if j % 20 < 6 else int(rng.integers(5, 40))
            for u in rng.choice(users, n, replace=False).tolist():
                cells[(u, j)] = rate()
    cl = sorted(cells.items())
    return nu, ni, np.array([k[0] for k, _ in cl], np.int32), np.array([k[1] for k, _ in cl], np.int32), np.array([v for _, v in cl])


@functools.lru_cache(maxsize=None)
def edge_handle(kind):
    nu, ni, u, i, r = edge_matrix(kind)
    h = capi.KNNInstance(kind, nu, ni)
    h.set_ratings(u, i, r)
    h.build("pcc", -1)
    return h


@functools.lru_cache(maxsize=None)
def edge_model(kind):
    """(S read back from the device, means, lists): the restatement's input"""
    nu, ni, u, i, r = edge_matrix(kind)
    rows = knn_ref.rows_of(u, i, r, kind, nu, ni)
    S = edge_handle(kind).similarity()
    assert (S < 0).any() and (S == 0.0).any() and np.isnan(S).any()
    return S, knn_ref.row_means(rows, EDGE_GM), knn_ref.lists_of(u, i, r, kind, nu, ni)


@functools.lru_cache(maxsize=None)
def edge_scores(kind, knn):
    """the restatement's ranking(u, j) of the query users 0 .. 7 over all 520 items (the other rows are not evaluated: NaN)"""
    nu, ni = edge_matrix(kind)[:2]
    S, means, lists = edge_model(kind)
    sc = np.full((nu, ni), np.nan)
    for u in range(8):
        for j in range(ni):
            sc[u, j] = knn_rank_ref.ranking_fast(kind, S, means, lists, u, j, knn, EDGE_GM)
    return sc


@pytest.mark.parametrize("kind", ["item", "user"])
def test_edge_matrix_has_the_edges(kind):
    nu, ni, u, i, r = edge_matrix(kind)
    lists = knn_ref.lists_of(u, i, r, kind, nu, ni)
    lens = {len(x) for x in lists}
    assert set(EDGE_LENGTHS[kind]) <= lens
    if kind == "item":
        assert [len(lists[q]) for q in range(8)] == list(EDGE_LENGTHS["item"])
    else:
        assert not any(a == 7 for a in u.tolist())
        train, _, _ = score_split(63)  # the smallest candidate set still meets every column length
        assert set(EDGE_LENGTHS["user"]) <= {len(lists[j]) for j in set(train[1].tolist())}
    sc = edge_scores(kind, 5)
    assert np.all(sc[7] == EDGE_GM)  # nothing to score with: the global mean everywhere
    tu, tj = all_tuples(8, ni)
    for knn in (0, 5, 20):
        got = edge_handle(kind).ranking(tu, tj, knn, EDGE_GM).reshape(8, ni)
        assert same_bits_exact(got, edge_scores(kind, knn)[:8]), (kind, knn, np.argwhere(got != edge_scores(kind, knn)[:8])[:5])


@pytest.mark.parametrize("knn", [0, 5, 20])
@pytest.mark.parametrize("n_cand,num_recs", [(63, 10), (64, 70), (65, 10), (513, 70), (513, 10)])
@pytest.mark.parametrize("kind", ["item", "user"])
def test_score_kernel_and_selection_edges(kind, n_cand, num_recs, knn):
    h = tb.Scored(edge_handle(kind), knn, EDGE_GM)
    scores = edge_scores(kind, knn)
    train, test, _ = score_split(n_cand)
    lists = check_rankings(h, scores, train, test, bin_thold=-1e9, num_recs=num_recs)
    plan_cand, queries = capi.rank_plan(h.n_users, h.n_items, train, test, -1e9, 0)
    assert len(plan_cand) == n_cand
    ex4 = {c: tuple(e) for u, c, _, e in queries if u == 4}
    assert len(ex4) == 4 and len(set(ex4.values())) == 4           # one group of four queries, four exclusion lists
    seven = [v for key, v in lists.items() if key[0] == 7]
    assert seven and all([i for i, _ in v] == plan_cand[:len(v)] for v in seven)   # every score the global mean: candidate order
    batched = with_env(lambda: h.eval_rankings(train, test, bin_thold=-1e9, num_recs=num_recs, with_lists=True), CMI_RANK_BATCH=3)
    assert batched[1] == lists                                     # batches that cut user 4's group: the same lists


@pytest.mark.parametrize("kind", ["item", "user"])
def test_modes_do_not_leak(kind):
    """after an evaluation, rating-mode predict on the same handle is knn_ref.predict's, bit for bit"""
    h = edge_handle(kind)
    train, test, _ = score_split(65)
    h.eval_rankings(train, test, 5, EDGE_GM)
    S, means, lists = edge_model(kind)
    ni = edge_matrix(kind)[1]
    tu, tj = all_tuples(8, ni)
    tu, tj = tu[::7], tj[::7]
    for knn in (0, 5):
        want = [knn_ref.predict_fast(kind, S, means, lists, int(u), int(j), knn, EDGE_GM, True, 1.0, 5.0) for u, j in zip(tu, tj)]
        assert same_bits_exact(h.predict(tu, tj, knn, EDGE_GM, True, 1.0, 5.0), np.array(want)), (kind, knn)
    rank = h.ranking(tu, tj, 5, EDGE_GM)
    assert not same_bits_exact(np.clip(rank, 1.0, 5.0), np.array(want))  # and the two modes do differ on this matrix


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["item", "user"])
def test_a_treeifying_list_is_refused_naming_the_tuple(kind):
    """the builder of tests/test_gpu_knn_predict.py: 60 fillers, then 9 ids that share their low 7 bits in a 128-slot table"""
    ids = Ids()
    nine = ids.block(spaced_ids(0, 60, 64, (5,)) + [128 + 5 + 128 * k for k in range(9)])
    fine = ids.block(spaced_ids(0, 60, 64, (5,)) + [128 + 5 + 128 * k for k in range(8)])
    c = Case(kind, ids.next + 8, seed=7)
    o_nine, o_fine = c.owner(nine), c.owner(fine)
    t = c.target(c.n_ent - 1, 1.0, 1.0)
    c.finish()
    try:
        with pytest.raises(knn_ref.Treeified):
            knn_ref.hashmap_grow(np.asarray(nine, np.int64))
        u, j = c.uj([o_nine, o_fine], [t, t])
        user, item = int(u[0]), int(j[0])
        with pytest.raises(capi.CmiError) as e:
            c.h.ranking(u, j, 0, 3.25)
        assert e.value.code == capi.E_UNSUPPORTED and "1 tuple(s) would treeify" in str(e.value), str(e.value)
        assert "(user %d, item %d)" % (user, item) in str(e.value), str(e.value)
        assert np.isfinite(c.h.ranking(u[1:], j[1:], 0, 3.25)).all()  # the handle goes on
        # the same tuple inside an evaluation: (user, item) is scored when the user has a test tuple and the item a training tuple
        other_user = int(u[1]) if kind == "item" else user - 1
        train = (np.array([other_user], np.int32), np.array([item], np.int32), np.array([0], np.int32), np.array([3.0]))
        test = (np.array([user], np.int32), np.array([item], np.int32), np.array([0], np.int32), np.array([5.0]))
        with pytest.raises(capi.CmiError) as e:
            c.h.eval_rankings(train, test, 0, 3.25)
        assert e.value.code == capi.E_UNSUPPORTED and "(user %d, item %d)" % (user, item) in str(e.value), str(e.value)
    finally:
        c.close()


def test_an_owner_list_past_the_limit_is_refused_before_anything_runs():
    """UserKNN: item 0 is rated by one user more than CMI_KNN_MAX_CANDIDATES, so it may not be a candidate of an evaluation nor the
    item of a ranking tuple; an evaluation whose candidates leave it out runs"""
    limit = 16384
    nu, ni = limit + 8, 3
    u = np.concatenate([np.arange(limit + 1), [0, 1, 2, 5], [1, 2, 7]]).astype(np.int32)
    i = np.concatenate([np.zeros(limit + 1), [1, 1, 1, 1], [2, 2, 2]]).astype(np.int32)
    r = 1.0 + (np.arange(len(u)) % 5).astype(np.float64)
    h = capi.KNNInstance("user", nu, ni)
    h.set_ratings(u, i, r)
    h.build("cos", -1)
    zeros = lambda n: np.zeros(n, np.int32)  # noqa: E731
    test = (np.array([1], np.int32), np.array([2], np.int32), zeros(1), np.array([5.0]))
    with pytest.raises(capi.CmiError) as e:
        h.eval_rankings((np.array([3, 5], np.int32), np.array([0, 2], np.int32), zeros(2), np.array([3.0, 3.0])), test, 20, 3.0)
    assert e.value.code == capi.E_UNSUPPORTED and "item 0 has %d candidates" % (limit + 1) in str(e.value), str(e.value)
    with pytest.raises(capi.CmiError) as e:
        h.ranking([1], [0], 20, 3.0)
    assert e.value.code == capi.E_UNSUPPORTED and "CMI_KNN_MAX_CANDIDATES" in str(e.value), str(e.value)
    res = h.eval_rankings((np.array([0, 5], np.int32), np.array([1, 2], np.int32), zeros(2), np.array([3.0, 3.0])), test, 20, 3.0)
    assert res["n_queries"] == 1
    h.close()


def test_evaluating_before_build_is_invalid():
    run = RUNS[0]
    train, test = contextual_split(run["cells"], 4, tb.SPLIT_SEED)
    h = capi.KNNInstance("item", run["n_users"], run["n_items"])
    for step in (lambda: None, lambda: h.set_ratings(run["u"], run["i"], run["r"])):
        step()
        with pytest.raises(capi.CmiError) as e:
            h.eval_rankings(train, test, 5, run["global_mean"])
        assert e.value.code == capi.E_INVALID
        with pytest.raises(capi.CmiError) as e:
            h.ranking([0], [0], 5, run["global_mean"])
        assert e.value.code == capi.E_INVALID
    h.close()
