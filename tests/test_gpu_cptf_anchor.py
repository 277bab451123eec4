"""CPTF at the shapes tests/test_gpu_cptf.py never reaches, held to tests/cptf_ref.py and oracle/rank_oracle.py alone.

Top-N (cptf_score_kernel, cmi_cptf_eval_rankings): more than 256 staged words (the staging loop's second trip), several batches
(q0 > 0), a catalogue larger than the candidate set with ids in HashSet order, +Inf / -Inf / NaN scores under a finite and an infinite
rating range, one handle evaluated, trained, re-set and evaluated again.  Epoch and predict: the LDS budget's edge (65536 bytes and
the first size past it), long streams over dimensions of hundreds of rows (requested rows that are NOT stale), models of both signs
and planted +Inf, -Inf, NaN and -0.0 elements, predict at the block borders.

Every case's premises (what it is meant to reach) are functions that take no handle; test_the_cases_reach_what_they_are_meant_to
runs them without a GPU."""
import functools
import math

import numpy as np
import pytest

from carskit_amd import capi
from oracle import rank_oracle
from tests import cptf_ref as cref
from tests.test_gpu_cptf import CTX_FORMS, LRATE, REG, SUM_FORMS, check_rankings, cols, draw_entries, draw_model, rank_case, run_forms
from tests.util import assert_same_rankings, same_bits, same_bits_exact, with_env

gpu = pytest.mark.gpu
INF, NAN = float("inf"), float("nan")
STAGE_THREADS = 256                                                  # cptf_score_kernel stages with a 256-thread stride loop


def oracle_lists(M, ctx_keys, lo, hi, tr, te, **kw):
    """oracle/rank_oracle.py fed with cptf_ref's scores: what check_rankings compares the device with"""
    score = functools.lru_cache(maxsize=None)(lambda u, c: cref.score_items(M, u, ctx_keys[c], lo, hi))
    return rank_oracle.eval_rankings(lambda u, j, c: score(u, c)[j], tr, te, **kw)


def list_scores(lists):
    return [s for lst in lists.values() for _, s in lst]


# ---- 1. factor counts and dimension counts ----------------------------------------------------------------------------------------
KS, NDIMS = [1, 2, 63, 64, 65, 128], [2, 3, 10]
CELLS = [(k, n) for k in KS for n in NDIMS] + [(128, 4)]
# (128, 3) stages exactly 256 words, the first trip's last thread; (128, 4) stands in for it past the border, with a second trip that is
# cut short, beside the two cells of ten dimensions (and (63, 10), (64, 10))
FILLS_ONE_TRIP, PAST_ONE_TRIP = {(128, 3)}, {(128, 4), (65, 10), (128, 10)}


def staged_words(k, n_dims):
    return (n_dims - 1) * k                                          # the user's row and one row per context dimension


@functools.lru_cache(maxsize=None)
def shape_case(k, n_dims):
    """65 candidates, 4 contexts whose key rows differ (every key column takes at least two values; the rows are distinct wherever the
    dimensions leave four distinct rows: one context dimension of three conditions has three), a model whose sums fall below, inside
    and above [1, 5]: the users' rows are scaled so that their predictions lie around 0.5, 1.5, 3, 4, 6 and 9"""
    dims = [6, 65] + [3, 2, 3, 2, 3, 2, 3, 2][:n_dims - 2]
    rng = np.random.default_rng(1000 * k + n_dims)
    M = draw_model(rng, dims, k, total=3.0, spread=0.3)
    M[0] *= (np.array([0.5, 1.5, 3.0, 4.0, 6.0, 9.0]) / 3.0)[:, None]
    ctx_keys = [[(c + x) % dims[2 + x] for x in range(n_dims - 2)] for c in range(4)]
    tr, te = rank_case(65, 7 * k + n_dims)
    return dims, M, ctx_keys, tr, te


def shape_case_is_sound(k, n_dims):
    dims, M, ctx_keys, tr, te = shape_case(k, n_dims)
    assert staged_words(k, n_dims) > STAGE_THREADS or (k, n_dims) not in PAST_ONE_TRIP, (k, n_dims)
    assert staged_words(k, n_dims) == STAGE_THREADS or (k, n_dims) not in FILLS_ONE_TRIP, (k, n_dims)
    keys = np.array(ctx_keys).reshape(4, n_dims - 2)
    assert all(len(set(keys[:, x].tolist())) >= 2 for x in range(n_dims - 2))
    assert len({tuple(row) for row in keys.tolist()}) == min(4, int(np.prod(dims[2:])))
    _, lists = oracle_lists(M, ctx_keys, 1.0, 5.0, tr, te, num_recs=10)
    s = list_scores(lists)
    assert any(v in (1.0, 5.0) for v in s) and any(1.0 < v < 5.0 for v in s), (k, n_dims)    # clamped and unclamped scores both occur
    return lists


@gpu
@pytest.mark.parametrize("k,n_dims", CELLS)
def test_eval_rankings_at_the_factor_and_dimension_counts(k, n_dims):
    """(n_dims - 1) * k staged words from 1 to 1152: one trip of the staging loop, and up to five"""
    dims, M, ctx_keys, tr, te = shape_case(k, n_dims)
    shape_case_is_sound(k, n_dims)
    check_rankings(M, dims, k, ctx_keys, 1.0, 5.0, tr, te, num_recs=10)


# ---- 2. several batches -----------------------------------------------------------------------------------------------------------
BATCH = 3


def batch_cuts(n, b):
    """the batches' first queries and n: below the taper (b / 12 < 64) the pipeline cuts ceil(n / b) pieces as equal as they get"""
    m = max(1, -(-n // b))
    return [n * i // m for i in range(m)] + [n]


@functools.lru_cache(maxsize=None)
def batch_case():
    dims, k = [6, 65, 3, 2], 65
    M = draw_model(np.random.default_rng(21), dims, k, total=3.0, spread=0.3)
    M[0] *= (np.array([0.5, 1.5, 3.0, 4.0, 6.0, 9.0]) / 3.0)[:, None]
    ctx_keys = [[2, 1], [0, 0], [1, 1], [2, 0]]
    tr, te = rank_case(65, 21)
    return dims, k, M, ctx_keys, tr, te


def batch_case_is_sound(q_user, q_ctx):
    """q_user, q_ctx: the plan's queries in its order.  At least three batches of at most BATCH queries, the last of them cut short;
    no query of a later batch has the (user, context keys) of the query at its place in the first batch, which a scorer that ignores
    q0 would read, and no two consecutive batches hold the same (user, context keys) in the same order"""
    _, _, _, ctx_keys, _, _ = batch_case()
    nq = len(q_user)
    assert nq >= 10 and nq > 2 * BATCH and nq % BATCH != 0
    what = [(u, tuple(ctx_keys[c])) for u, c in zip(q_user, q_ctx)]
    assert len(set(what)) == nq                                      # users and context keys differ from query to query
    cuts = batch_cuts(nq, BATCH)
    batches = [what[a:b] for a, b in zip(cuts, cuts[1:])]
    assert len(batches) >= 3 and all(1 <= len(b) <= BATCH for b in batches) and len({len(b) for b in batches}) > 1
    assert all(a != b for a, b in zip(batches, batches[1:]))
    assert all(what[q] != what[q - q0] for q0 in cuts[1:-1] for q in range(q0, min(q0 + BATCH, nq)))


def plan_queries(dims, tr, te, **kw):
    _, queries = capi.rank_plan(dims[0], dims[1], cols(tr), cols(te), **kw)
    return [q[0] for q in queries], [q[1] for q in queries]


@gpu
def test_eval_rankings_in_several_batches():
    """CMI_RANK_BATCH=3: every batch but the first has q0 > 0, the slab's rows count from 0 in each"""
    dims, k, M, ctx_keys, tr, te = batch_case()
    batch_case_is_sound(*plan_queries(dims, tr, te))
    got = []
    for batch in (BATCH, None):
        with_env(lambda: check_rankings(M, dims, k, ctx_keys, 1.0, 5.0, tr, te, got=got, num_recs=10), CMI_RANK_BATCH=batch)
    assert got[0][0]["n_queries"] > 2 * BATCH and len(got[0][1]) > 2 * BATCH
    assert_same_rankings(got[0], got[1], "batches of 3 against one batch")


# ---- 3. a catalogue larger than the candidate set ---------------------------------------------------------------------------------
N_CATALOGUE, N_CAND = 3072, 257


@functools.lru_cache(maxsize=None)
def catalogue_ids():
    """257 item ids below 3072 with distinct buckets in the final HashSet table of 512 slots, so the candidate order is the bucket
    order whatever the order of the training tuples; the ids lie up to five tables above their bucket, so it is not the id order"""
    rng = np.random.default_rng(20261101)
    buckets = np.sort(rng.choice(512, N_CAND, replace=False))
    return (buckets + 512 * rng.integers(0, N_CATALOGUE // 512, N_CAND)).tolist()


@functools.lru_cache(maxsize=None)
def catalogue_case():
    dims, k = [6, N_CATALOGUE, 3, 2], 10
    rng = np.random.default_rng(31)
    ids = catalogue_ids()
    M = [0.85 + 0.12 * rng.standard_normal((n, k)) for n in dims]
    M[1][np.setdiff1d(np.arange(N_CATALOGUE), ids)] = 50.0           # a row that is no candidate's would head every list
    ctx_keys = [[2, 1], [0, 0], [1, 1], [2, 0]]
    tr, te = rank_case(N_CAND, 31, ids=ids)
    return dims, k, M, ctx_keys, tr, te


def catalogue_case_is_sound():
    dims, k, M, ctx_keys, tr, te = catalogue_case()
    ids = catalogue_ids()
    assert len(set(ids)) == N_CAND and max(ids) < N_CATALOGUE and sum(j >= 512 for j in ids) > 100
    assert {t[1] for t in tr} == set(ids) and {t[1] for t in te} <= set(ids)        # the train tuples reach exactly the candidates
    order = rank_oracle.java_int_hashset_order([t[1] for t in tr])
    assert order == ids and order != sorted(ids)                     # candidate order is bucket order, not id order
    assert sum(a > b for a, b in zip(order, order[1:])) > 50
    free = cref.score_items(M, 0, ctx_keys[0], -INF, INF)
    assert min(free[j] for j in range(N_CATALOGUE) if j not in set(ids)) > 5 * max(free[j] for j in ids)


@gpu
@pytest.mark.parametrize("num_ignore", [0, 2])
def test_eval_rankings_catalogue_larger_than_the_candidate_set(num_ignore):
    """n_items = 3072 against 257 (255) candidates: the transposed read's stride is the catalogue's size, the candidate's position is
    not its id; two blocks of candidates, the second with one live thread"""
    dims, k, M, ctx_keys, tr, te = catalogue_case()
    catalogue_case_is_sound()
    for hi in (5.0, 1e9):                                            # (under 1e9 nothing clamps: a foreign row's 50s would show as such)
        lists = check_rankings(M, dims, k, ctx_keys, 1.0, hi, tr, te, num_recs=10, num_ignore=num_ignore)
        assert all(i in set(catalogue_ids()) for lst in lists.values() for i, _ in lst)
    assert len({s for s in list_scores(lists)}) > len(lists)         # (unclamped: no list of ties)


# ---- 4. infinite and NaN scores ---------------------------------------------------------------------------------------------------
P_INF, N_INF = (0, 63, 64, 255, 256), (1, 64, 200)                   # candidate positions; 64 holds both infinities
SIGNS = [(a, b) for a in (0.5, -0.5, 0.0) for b in (0.5, -0.5, 0.0)]  # users 0..8, as tests/nonfinite_scores.py draws them
U_PP, U_0P = 0, 6
CTX_NAN = 2                                                          # the context whose row holds a NaN


@functools.lru_cache(maxsize=None)
def nonfinite_case():
    """k = 3, three dimensions, 257 candidates whose ids are their positions.  Factor 0 carries +Inf at P_INF, factor 1 -Inf at N_INF,
    factor 2 a finite score that lies below, inside and above [1, 5].  Context rows: all ones; a zero in factor 0 (0 * Inf for every
    user); a NaN; factor 1 negated"""
    dims, k = [9, N_CAND, 4], 3
    rng = np.random.default_rng(44)
    P = np.column_stack([np.array(SIGNS), [3.0, 0.3, 1.65, 0.64, 2.66, 0.98, 2.33, 1.3, 2.0]])
    Q = rng.uniform(0.5, 2.0, (N_CAND, k))
    Q[list(P_INF), 0] = INF
    Q[list(N_INF), 1] = -INF
    C = np.array([[1.0, 1.0, 1.0], [0.0, 1.0, 1.5], [NAN, 1.0, 1.0], [1.0, -1.0, 1.0]])
    ctx_keys = [[0], [1], [CTX_NAN], [3], [0]]
    tr, te = rank_case(N_CAND, 44, n_users=9, n_ctx=5)
    return dims, k, [P, Q, C], ctx_keys, tr, te


def nonfinite_case_is_sound():
    """on the oracle's lists alone: a +Inf entry that heads its list; -Inf candidates, which no list takes under the infinite range
    (a score enters only if it is > the threshold) and which are entries of 1.0 under [1, 5] at num_recs = 300; a 5.0 that came from
    +Inf beside a 5.0 that was clamped honestly; a NaN candidate left out; 0 * Inf and Inf - Inf"""
    dims, k, M, ctx_keys, tr, te = nonfinite_case()
    assert rank_oracle.java_int_hashset_order([t[1] for t in tr]) == list(range(N_CAND))     # positions are ids
    free = functools.lru_cache(maxsize=None)(lambda u, c: cref.score_items(M, u, ctx_keys[c], -INF, INF))
    assert math.isnan(free(U_PP, 0)[64]) and free(U_PP, 0)[63] == INF and free(U_PP, 0)[1] == -INF      # Inf - Inf
    assert math.isnan(free(U_0P, 0)[0]) and math.isnan(free(U_PP, 1)[0])                     # 0 * Inf: the user's zero, the context's
    rated = {}
    for u, j, c, _ in tr:
        rated.setdefault((u, c), set()).add(j)
    out = {}
    for (lo, hi) in ((1.0, 5.0), (-INF, INF)):
        for num_recs in (10, 300):
            out[lo, num_recs] = oracle_lists(M, ctx_keys, lo, hi, tr, te, num_recs=num_recs)[1]
    open10, open300, in10, in300 = out[-INF, 10], out[-INF, 300], out[1.0, 10], out[1.0, 300]
    assert open10 and all(c != CTX_NAN for _, c in open300)          # a NaN context row: every score a NaN, no list
    assert any(lst[0][1] == INF for lst in open10.values())
    assert all(s != -INF for s in list_scores(open300))
    seen = {"pinf_as_5": 0, "honest_5_beside": 0, "ninf_left_out": 0, "ninf_as_1": 0, "nan_left_out": 0}
    for (u, c), lst in in300.items():
        raw, listed = free(u, c), {j: s for j, s in lst}
        listed_open = {j for j, _ in open300.get((u, c), [])}
        for j in range(N_CAND):
            if j in rated.get((u, c), ()):
                continue
            seen["ninf_left_out"] += raw[j] == -INF and j not in listed_open
            seen["ninf_as_1"] += raw[j] == -INF and listed.get(j) == 1.0
            seen["nan_left_out"] += math.isnan(raw[j]) and j not in listed and j not in listed_open
        top = in10.get((u, c), [])
        from_inf = [j for j, s in top if s == 5.0 and raw[j] == INF]
        seen["pinf_as_5"] += len(from_inf)
        seen["honest_5_beside"] += bool(from_inf) and any(s == 5.0 and 5.0 < raw[j] < INF for j, s in top)
    assert all(seen.values()), seen


@gpu
@pytest.mark.parametrize("lo,hi", [(1.0, 5.0), (-INF, INF)], ids=["1..5", "unbounded"])
def test_eval_rankings_infinite_and_nan_scores(lo, hi):
    """cptf_clamp sends +Inf to max_rate and -Inf to min_rate, where they tie with honestly clamped scores in the oracle's order;
    under infinite bounds they reach the selection as they are; a NaN term (0 * Inf, Inf - Inf, a NaN row) is a NaN score, left out"""
    dims, k, M, ctx_keys, tr, te = nonfinite_case()
    nonfinite_case_is_sound()
    for num_recs in (10, 300):
        check_rankings(M, dims, k, ctx_keys, lo, hi, tr, te, num_recs=num_recs)


# ---- 5. one handle, several evaluations -------------------------------------------------------------------------------------------
@gpu
def test_one_handle_evaluates_trains_is_set_and_evaluates_again():
    """Qt is refilled at each evaluation, d_qu / d_qkeys grow with the queries: evaluate; train; evaluate; set another model and another
    key table; evaluate more queries than ever before.  Each time against the oracle fed with the model the handle holds"""
    dims, k = [6, 65, 3, 2], 10
    rng = np.random.default_rng(51)
    M0 = draw_model(rng, dims, k, total=3.0, spread=0.3)
    keys1, keys3 = [[2, 1], [0, 0], [1, 1], [2, 0]], [[0, 0], [1, 1], [2, 1], [1, 0]]
    tr1, te1 = rank_case(65, 51, n_users=2, n_ctx=3)
    tr3, te3 = rank_case(65, 52, n_users=6, n_ctx=4)
    nq1, nq3 = (len({(u, c) for u, _, c, _ in te}) for te in (te1, te3))
    assert nq3 > 2 * nq1                                             # the last evaluation outgrows the first one's query buffers
    h = capi.CPTFInstance(k, dims)
    h.set_model(M0)
    h.set_context_keys(keys1)
    h.set_rating_range(1.0, 5.0)
    first = check_rankings(M0, dims, k, keys1, 1.0, 5.0, tr1, te1, h=h, num_recs=10)
    ek, er = draw_entries(rng, dims, 200)
    h.set_entries(ek, er)
    for _ in range(2):
        h.iterate(LRATE, REG)
    M1 = h.model()
    assert all(not np.array_equal(a, b) for a, b in zip(M0, M1))
    second = check_rankings(M1, dims, k, keys1, 1.0, 5.0, tr1, te1, h=h, num_recs=10)
    M2 = draw_model(rng, dims, k, total=2.5, spread=0.3)
    h.set_model(M2)
    h.set_context_keys(keys3)
    third = check_rankings(M2, dims, k, keys3, 1.0, 5.0, tr3, te3, h=h, num_recs=10)
    h.close()
    assert first and set(first) == set(second) and len(third) > len(first)
    assert first != second                                           # a stale Qt would give the first lists again
    assert any(first[q] != third[q] for q in first if q in third)


# ---- 6. the LDS budget's edge -----------------------------------------------------------------------------------------------------
LDS_BUDGET = 64 * 1024


def lds_case(dims, seed):
    """64 entries that touch the first and the last row of every context dimension"""
    rng = np.random.default_rng(seed)
    keys = np.stack([rng.integers(0, d, 64) for d in dims], axis=1).astype(np.int32)
    keys[0, 2:], keys[1, 2:], keys[63, 2:] = 0, np.array(dims[2:]) - 1, np.array(dims[2:]) - 1
    return keys, rng.integers(1, 6, 64).astype(np.float64)


def ctx_bytes(dims, k):
    return sum(dims[2:]) * k * 8


def lds_case_is_sound(dims, want_bytes):
    keys, _ = lds_case(dims, 6)
    assert ctx_bytes(dims, 128) == want_bytes
    assert all(set(keys[:, d].tolist()) >= {0, dims[d] - 1} for d in range(2, len(dims)))


@gpu
@pytest.mark.parametrize("dims", [[3, 4, 64], [3, 4, 32, 32]], ids=["one dimension", "two dimensions"])
def test_context_rows_of_exactly_the_lds_budget_stay_in_lds(dims):
    """k = 128: 65536 bytes of dynamic LDS, asked for without an opt-in attribute; both context forms (run_forms holds ctx_in_lds() to
    the form's name) and both summation forms"""
    lds_case_is_sound(dims, LDS_BUDGET)
    keys, r = lds_case(dims, 6)
    run_forms(dims, 128, keys, r, seed=6, iters=2)


@gpu
def test_context_rows_one_row_past_the_lds_budget_travel_through_memory():
    """65 rows at k = 128: 66560 bytes, with no flag set"""
    dims = [3, 4, 65]
    lds_case_is_sound(dims, LDS_BUDGET + 8 * 128)
    keys, r = lds_case(dims, 6)
    run_forms(dims, 128, keys, r, seed=6, ctx_forms=[("global", 0)], iters=2)


# ---- 7. rows that are not stale ---------------------------------------------------------------------------------------------------
LONG_DIMS = [300, 200, 7, 5]
PAIRS = {"user then item": 100, "dimension 2 then dimension 3": 200, "every dimension": 300}       # the first entry of each planted pair


@functools.lru_cache(maxsize=None)
def long_stream():
    """600 entries: users and items drawn uniformly over 300 and 200 rows, conditions over 7 and 5 among those that differ from the
    neighbours' (two neighbours in five would share a condition otherwise): a requested row is one that was written two or more
    entries ago, or never.  Planted: neighbours whose EQUAL keys belong to DIFFERENT dimensions (no replacement from registers), and
    one pair equal in every dimension"""
    rng = np.random.default_rng(71)
    keys = np.stack([rng.integers(0, d, 600) for d in LONG_DIMS], axis=1).astype(np.int32)
    t = PAIRS["user then item"]
    keys[t, :2], keys[t + 1, :2] = (3, 7), (8, 3)
    t = PAIRS["dimension 2 then dimension 3"]
    fixed = {(t, 2): 2, (t, 3): 4, (t + 1, 2): 5, (t + 1, 3): 2}
    twin = PAIRS["every dimension"] + 1
    for d in (2, 3):
        for t in range(600):
            apart = {int(keys[t - 1, d])} if t else set()
            apart.add(fixed.get((t + 1, d)))
            keys[t, d] = fixed.get((t, d), rng.choice([x for x in range(LONG_DIMS[d]) if x not in apart]))
            if t == twin:
                keys[t, d] = keys[t - 1, d]
    keys[twin, :2] = keys[twin - 1, :2]
    keys.setflags(write=False)
    return keys, rng.integers(1, 6, 600).astype(np.float64)


def long_stream_is_sound():
    keys, _ = long_stream()
    same = keys[1:] == keys[:-1]
    assert same.any(axis=1).mean() < 0.1, same.any(axis=1).mean()    # fewer than a tenth of the neighbours share a row
    t = PAIRS["user then item"]
    assert keys[t, 0] == keys[t + 1, 1] == 3 and not same[t].any()
    t = PAIRS["dimension 2 then dimension 3"]
    assert keys[t, 2] == keys[t + 1, 3] == 2 and not same[t, 2:].any()
    assert same[PAIRS["every dimension"]].all()
    first_visit = sum(len(set(keys[:, d].tolist())) for d in (0, 1))
    assert first_visit > 400 and len(set(keys[:, 0].tolist())) < 300      # a third of the user and item rows asked for were never written


@gpu
@pytest.mark.parametrize("k", [2, 65])
def test_epoch_over_rows_written_long_ago_or_never(k):
    long_stream_is_sound()
    keys, r = long_stream()
    run_forms(LONG_DIMS, k, keys, r, seed=70 + k)


# ---- 8. signs and non-finite elements ---------------------------------------------------------------------------------------------
SIGN_DIMS = [3, 4, 2, 3]


def signed_model(k, seed):
    """standard_normal with no offset: about half the elements negative, predictions around 0"""
    rng = np.random.default_rng(seed)
    return [0.8 * rng.standard_normal((n, k)) for n in SIGN_DIMS]


def signed_model_is_sound(k):
    neg = np.mean(np.concatenate([m.ravel() for m in signed_model(k, 80 + k)]) < 0)
    assert 0.3 < neg < 0.7


@gpu
@pytest.mark.parametrize("k", [5, 65])
def test_epoch_with_factors_of_both_signs(k):
    """sgd / df * e with negative sgd, negative df and negative e (run_forms asserts that the restatement's losses stay finite)"""
    signed_model_is_sound(k)
    keys, r = draw_entries(np.random.default_rng(80 + k), SIGN_DIMS, 60)
    run_forms(SIGN_DIMS, k, keys, r, seed=0, M0=signed_model(k, 80 + k))


PLANT_DIMS = [30, 40, 7, 5]                                          # wide enough that the NaN does not reach every row
PLANTS = [("+inf", INF), ("-inf", -INF), ("nan", NAN), ("-0.0", -0.0)]


@gpu
@pytest.mark.parametrize("d", [0, 1, 2], ids=["user row", "item row", "context row"])
@pytest.mark.parametrize("name,value", PLANTS, ids=[p[0] for p in PLANTS])
def test_a_non_finite_or_negative_zero_element_gives_e_numeric_and_the_restatements_nan_pattern(name, value, d):
    """Inf / Inf, 0 * Inf and 0 / -0 in the entry's update: E_NUMERIC, the loss in bits (a NaN equals a NaN), M with NaN where the
    restatement has NaN and bit for bit elsewhere -- the infinities and signed zeros it keeps included; both summation forms, both
    context forms"""
    k, rng = 5, np.random.default_rng(90)
    keys = np.stack([rng.integers(0, n, 16) for n in PLANT_DIMS], axis=1).astype(np.int32)
    keys[9, d] = keys[3, d]                                          # the planted row is trained by entry 3 and met again by entry 9
    r = rng.integers(1, 6, 16).astype(np.float64)
    M0 = [0.8 * rng.standard_normal((n, k)) for n in PLANT_DIMS]
    M0[d][int(keys[3, d]), 2] = value
    for sname, sflag, ref_epoch in SUM_FORMS:
        want = [m.copy() for m in M0]
        want_loss = ref_epoch(want, keys, r, LRATE, REG)
        assert not math.isfinite(want_loss), (sname, want_loss)      # the restatement alone says so
        assert any(np.isnan(m).any() for m in want)
        assert any((np.isfinite(m) & (m != m0)).all(axis=1).any() for m, m0 in zip(want, M0))      # and rows trained cleanly beside them
        for cname, cflag in CTX_FORMS:
            h = capi.CPTFInstance(k, PLANT_DIMS, flags=sflag | cflag)
            h.set_entries(keys, r)
            h.set_model(M0)
            with pytest.raises(capi.CmiError) as e:
                h.iterate(LRATE, REG)
            got = h.model()
            assert h.ctx_in_lds() == (cname == "lds")
            h.close()
            assert e.value.code == capi.E_NUMERIC and same_bits([e.value.loss], [want_loss]), (sname, cname, e.value.loss, want_loss)
            for x in range(len(PLANT_DIMS)):
                assert same_bits(got[x], want[x]), (sname, cname, x, np.argwhere(got[x] != want[x])[:5])


# ---- 9. predict at the block borders ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_predict_at_the_block_borders(n):
    """a block of 256 tuples: one tuple, one short of a block, a block, a block and one"""
    dims, k = [3, 4, 2, 3, 2], 65
    rng = np.random.default_rng(n)
    M = draw_model(rng, dims, k, total=3.0, spread=0.3)
    keys = np.stack([rng.integers(0, d, n) for d in dims], axis=1).astype(np.int32)
    free = [cref.predict_keys(M, ks) for ks in keys.tolist()]
    lo, hi = (np.percentile(free, [30, 70]).tolist() if n > 1 else (free[0] + 1.0, free[0] + 2.0))
    h = capi.CPTFInstance(k, dims)
    h.set_model(M)
    assert same_bits_exact(h.predict(keys), free)
    assert same_bits_exact(h.predict(keys, True, lo, hi), [cref.clamp(p, lo, hi) for p in free])
    h.close()
    assert n == 1 or len({cref.clamp(p, lo, hi) == p for p in free}) == 2


# ---- the premises, without a GPU --------------------------------------------------------------------------------------------------
def test_the_cases_reach_what_they_are_meant_to():
    """staged words above 256 where meant, at least three batches with a short one, candidate order different from id order, the
    oracle's lists holding +Inf, a clamped infinity and no -Inf, the byte counts at the LDS budget's edge, the stale-pair share below
    a tenth, a model of both signs"""
    for k, n_dims in CELLS:
        shape_case_is_sound(k, n_dims)
    assert PAST_ONE_TRIP | FILLS_ONE_TRIP <= set(CELLS)
    dims, _, _, _, tr, te = batch_case()
    batch_case_is_sound(*plan_queries(dims, tr, te))
    catalogue_case_is_sound()
    nonfinite_case_is_sound()
    for dims, want in (([3, 4, 64], LDS_BUDGET), ([3, 4, 32, 32], LDS_BUDGET), ([3, 4, 65], LDS_BUDGET + 1024)):
        lds_case_is_sound(dims, want)
    long_stream_is_sound()
    for k in (5, 65):
        signed_model_is_sound(k)
