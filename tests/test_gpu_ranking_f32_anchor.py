"""The fp32 evalRankings kernels -- the split contraction on the f32 matrix cores (rank_gemm_mfma_f32), the tile-pruned selection
(rank_topn_split_pruned), the plain split selection, and the per-query form (rank_mask + rank_topn_stream / rank_topn) -- against
oracle/rank_oracle.py over an fp64 score table, with NO training in between: the model is injected with set_states, read back as
fp32, and the reference scores are computed in fp64 from exactly those values (tests/rank_anchor.py).  What stands between the
GPU's answer and the reference is then the ranking kernels alone.

Layer 1: states on a grid where every fp32 partial sum of a score is exact in any association.  The fp32 score EQUALS the fp64
score, so queries, lists (item for item, in order) and scores (bit for bit) must equal the oracle's; the 18 measures to 1e-12
(host arithmetic, the bar of test_f64_rankings_match_oracle).  Two value distributions: `spread` (many distinct scores: wrong data
shows) and `tied` (a handful of distinct scores and the threshold ON the most frequent one: tie order, `>` against `>=` at the
threshold and at the N-th best, exclusions inside skipped tiles show).

Layer 2: arbitrary fp32 states.  Every listed score within the forward bound B = gamma_n * sum |terms| of the fp64 score, the
list sorted and complete up to that bound, and for every query the reference alone decides (an `unambiguous` query: at least 80 %
of each case) the list equal to the oracle's item for item.  Nothing in B is measured.

The premises (exact sums in four orders; the unambiguous share) are host-only and are also checked without a device.
`python -m tests.test_gpu_ranking_f32_anchor` prints them per case.

Wall time on an MI355X box: 30 s for the module (96 tests), 24 s of it the 48 GPU tests (most of that the Python oracle)."""
import math
import time
import zlib

import numpy as np
import pytest

from carskit_amd import capi, synth
from oracle import rank_oracle
from tests import rank_anchor as ra
from tests import util

gpu = pytest.mark.gpu

DEFAULT = {"CMI_RANK_NO_SPLIT": None, "CMI_RANK_NO_PRUNE": None}
NO_PRUNE = {"CMI_RANK_NO_SPLIT": None, "CMI_RANK_NO_PRUNE": "1"}
NO_SPLIT = {"CMI_RANK_NO_SPLIT": "1", "CMI_RANK_NO_PRUNE": None}
ALL3 = (DEFAULT, NO_PRUNE, NO_SPLIT)


def _case(model, k, nc, n_users, n_conds=3, num_recs=10, batch=None, forms=(DEFAULT,), one_stream=False, num_ignore=0, strategy="ucu"):
    return dict(model=model, k=k, nc=nc, n_users=n_users, n_conds=n_conds, num_recs=num_recs, batch=batch, forms=forms,
                one_stream=one_stream, num_ignore=num_ignore, strategy=strategy)


# Which case covers which value (every case runs both distributions; cases are named model-k-candidates):
#   k, kp1 = ceil16(k), steps of the contraction's k loop (RG_BK = 16):
#     1 -> 1 step, padded: PMF-1-63            15 -> 1, padded: CAMF_C-15-64             16 -> 1, unpadded: CAMF_CI-16-65
#     17 -> 2, padded: CAMF_CUCI-17-127        33 -> 3 (odd), padded: BiasedMF-33-128    48 -> 3, unpadded: CAMF_CU-48-129
#     64 -> 4: CAMF_CI-64-4095, CAMF_CUCI-64-9000     100 -> 7, padded: PMF-100-4096     128 -> 8: CAMF_CI-128-9000, BiasedMF-128-4097,
#     CAMF_CI-128-4097     200 -> 13 (odd), padded: CAMF_C-200-4096     256 -> 16: CAMF_CUCI-256-9000, CAMF_CU-256-4097
#   candidates: 63, 64, 65 (the 64-candidate tile): PMF-1-63, CAMF_C-15-64, CAMF_CI-16-65; 127, 128, 129 (the 128-column block tile):
#     CAMF_CUCI-17-127, BiasedMF-33-128, CAMF_CU-48-129; 4095, 4096, 4097 (the selection's chunk of 64 tiles): CAMF_CI-64-4095,
#     PMF-100-4096 and CAMF_C-200-4096, BiasedMF-128-4097 / CAMF_CU-256-4097 / CAMF_CI-128-4097; 9000: CAMF_CI-128-9000,
#     CAMF_CUCI-256-9000, CAMF_CUCI-64-9000
#   128 x 128 block tiles of the S1 contraction: a multiple of 8 -- 32 (CAMF_C-200-4096: 4096 candidates x 100 users, one batch), 32 per
#     batch (PMF-100-4096: batches of 128 users); not -- 33 / 66 (the 4097 cases), 71 / 142 (the 9000 cases), 1 (the small ones)
#   user groups per batch (CMI_RANK_BATCH, with 3 x as many users: three batches of exactly that many rows, both slab parities reused
#     behind evsel[b - 2]): 1 -> PMF-1-63 (40 batches); 127 -> CAMF_CU-256-4097; 128 -> CAMF_CUCI-256-9000, PMF-100-4096; 129 ->
#     BiasedMF-128-4097; unset (one batch) -> the others; CMI_RANK_ONE_STREAM=1 with three batches -> CAMF_CI-64-4095.  (Under
#     CMI_RANK_NO_SPLIT the same variable counts queries: batches of 127 / 128 / 129 queries there.)
#   n_conds, kp2 = ceil16(n_conds), on the icBias models: 3 -> CAMF_CI-16-65, CAMF_CUCI-64-9000; 16 -> CAMF_CI-128-9000; 17 ->
#     CAMF_CUCI-17-127, CAMF_CI-128-4097; 40 -> CAMF_CUCI-256-9000, CAMF_CI-64-4095.  Every problem has 12 distinct contexts with 0, 1, 2
#     and up to 6 conditions, and users with queries in two contexts (the S2 slab and q_dctx)
#   models: all six, each at least twice; CAMF_C with the serial flag
#   num_recs on the split form: 1 -> CAMF_C-15-64; 5 -> PMF-1-63, CAMF_C-200-4096; 10 -> most; 64 -> CAMF_CI-16-65, CAMF_CUCI-64-9000;
#     70 (the per-query extraction form, rank_topn) -> CAMF_CU-48-129, CAMF_CI-128-4097
#   num_ignore = 5 -> CAMF_CUCI-17-127; strategy uc -> BiasedMF-33-128 (the others ucu)
#   forms: default + CMI_RANK_NO_PRUNE + CMI_RANK_NO_SPLIT (ALL3) on the corners (k = 128, 256) x (9000, 4097) and on the 64 / 65 / 127
#     candidate cases; default + NO_SPLIT on PMF-1-63; default + NO_PRUNE on PMF-100-4096 and CAMF_CUCI-64-9000
#   every problem: users with >= 20 rated items in their query's context, and one query whose eligible candidates above the threshold
#     number fewer than num_recs (its user rated all the others: an exclusion list of hundreds to thousands of entries)
L1_CASES = [
    _case("CAMF_CI", 128, 9000, 150, n_conds=16, forms=ALL3),
    _case("CAMF_CUCI", 256, 9000, 384, n_conds=40, batch="128", forms=ALL3),
    _case("BiasedMF", 128, 4097, 387, batch="129", forms=ALL3),
    _case("CAMF_CU", 256, 4097, 381, n_conds=17, batch="127", forms=ALL3),
    _case("PMF", 1, 63, 40, num_recs=5, batch="1", forms=(DEFAULT, NO_SPLIT)),
    _case("CAMF_C", 15, 64, 60, num_recs=1, forms=ALL3),
    _case("CAMF_CI", 16, 65, 60, n_conds=3, num_recs=64, forms=ALL3),
    _case("CAMF_CUCI", 17, 127, 60, n_conds=17, num_ignore=5, forms=ALL3),
    _case("BiasedMF", 33, 128, 60, strategy="uc"),
    _case("CAMF_CU", 48, 129, 60, n_conds=16, num_recs=70),
    _case("CAMF_CI", 64, 4095, 384, n_conds=40, batch="128", one_stream=True),
    _case("PMF", 100, 4096, 384, batch="128", forms=(DEFAULT, NO_PRUNE)),
    _case("CAMF_C", 200, 4096, 100, n_conds=16, num_recs=5),
    _case("CAMF_CI", 128, 4097, 100, n_conds=17, num_recs=70),
    _case("CAMF_CUCI", 64, 9000, 100, n_conds=3, num_recs=64, forms=(DEFAULT, NO_PRUNE)),
]

# layer 2: all six models x k in {64, 128, 256}, every (k, candidates) pair of {64, 128, 256} x {4097, 9000}; both forms on each
L2_CASES = [(m, k, (4097, 9000)[(i + j) % 2]) for i, m in enumerate(util.MODELS) for j, k in enumerate((64, 128, 256))]
L2_NUM_RECS, L2_THOLD, L2_USERS = 10, 2.5, 150


def _id(c):
    return "%s-k%d-nc%d" % (c["model"], c["k"], c["nc"])


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


# ---- host-only parts ------------------------------------------------------------------------------------------------------------

def l1_problem(case, dist):
    prob = ra.make_problem(case["model"], case["nc"], case["n_users"], case["n_conds"], _seed(_id(case), dist))
    st, gm = ra.exact_state(case["model"], prob, case["k"], dist, _seed(_id(case), dist, "state"))
    return prob, st, gm


def l1_reference(case, dist, prob, st, gm):
    """From the (read-back) fp32 state: the fp64 score table, the threshold, the short-list query (appended to prob.train) and the
    premise of layer 1; returns (F, thold)."""
    model = case["model"]
    F = ra.score_table(model, st, gm, prob, prob.queries)
    if dist == "tied":                    # ON the value most scores take: `score > thold` is strict, all of those must stay out
        thold, n_at = ra.modal_score(F)
        assert n_at >= 0.05 * F.size and -7.0 < thold < 5.0, (thold, n_at)
    else:
        thold = 2.5
    ra.check_exact_premise(model, st, gm, prob, F, prob.queries, _seed(_id(case), dist, "premise"))
    short = ra.add_short_query(prob, F, prob.queries, thold, case["num_recs"], _seed(_id(case), "short"))
    E = ra.eligible_mask(prob, prob.queries)
    n_pass = ((F > thold) & E).sum(axis=1)
    assert n_pass[prob.queries.index(short)] < case["num_recs"]                       # a short list (-1 / NaN padding) ...
    assert case["num_recs"] == 1 or 0 < n_pass[prob.queries.index(short)]             # ... that is not empty
    assert max(len(x) for x in ra.excluded_columns(prob).values()) >= 20              # long exclusion lists are in play
    assert np.mean(n_pass > 0) >= 0.5                                                 # most queries have a list (the rest: no list at all)
    if dist == "tied":
        # ties at the N-th-best boundary (wherever the candidates outnumber the list by far): queries whose N-th and (N + 1)-th best
        # eligible scores are equal
        n = case["num_recs"]
        srt = -np.sort(-np.where(E & (F > thold), F, -np.inf), axis=1)
        if case["nc"] >= 20 * n:
            assert np.sum((srt[:, n - 1] == srt[:, n]) & np.isfinite(srt[:, n])) >= 0.25 * len(prob.queries)
    return F, thold


def l2_problem(model, k, nc):
    prob = ra.make_problem(model, nc, L2_USERS, 16, _seed("l2", model, k, nc))
    st = synth.init_state(model, prob, k, seed=_seed("l2state", model, k, nc), dtype=np.float32)
    return prob, st, (0.0 if model == "PMF" else 3.0)


def l2_thold(model):
    return 0.0 if model == "PMF" else L2_THOLD      # PMF scores are bare dot products around zero


def l2_reference(model, k, prob, st, gm):
    """F, B, eligibility, the unambiguous queries and their expected lists -- from the reference alone; asserts the 80 % cap."""
    F = ra.score_table(model, st, gm, prob, prob.queries)
    B = ra.error_bound(model, st, gm, prob, prob.queries, k)
    E = ra.eligible_mask(prob, prob.queries)
    ok, tops = ra.unambiguous(F, B, E, l2_thold(model), L2_NUM_RECS)
    share = float(ok.mean())
    print("layer 2 %s k=%d nc=%d: %d queries, mean B %.2e, unambiguous share %.3f" % (model, k, len(prob.cand), len(ok), B.mean(), share))
    assert share >= 0.80, share
    return F, B, E, ok, tops


@pytest.mark.parametrize("dist", ["spread", "tied"])
@pytest.mark.parametrize("case", L1_CASES, ids=_id)
def test_layer1_premise_holds_on_the_host(case, dist):
    prob, st, gm = l1_problem(case, dist)
    l1_reference(case, dist, prob, st, gm)


@pytest.mark.parametrize("model,k,nc", L2_CASES)
def test_layer2_inputs_are_mostly_unambiguous(model, k, nc):
    prob, st, gm = l2_problem(model, k, nc)
    l2_reference(model, k, prob, st, gm)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

def _instance(model, k, prob, st, gm):
    """The injected model: set_ratings only gives the contextual models their context table (no epoch is ever run); returns the
    instance and the state as the device holds it."""
    inst = capi.Instance(model, k, prob.n_users, prob.n_items, prob.n_conds, flags=capi.FLAG_SCHED_SERIAL if model == "CAMF_C" else 0)
    inst.set_hparams(util.REG, util.REG, util.REG, util.REGC, gm)
    if model not in util.TWO_D:
        u, j, c, r = ra.arrays(prob.train)
        inst.set_ratings(u, j, c, r, prob.ctx_ptr, prob.ctx_conds)
    inst.set_states(st)
    back = inst.get_states(np.float32)
    for name, a in st.items():
        assert back[name].dtype == np.float32 and np.array_equal(back[name], a), name
    return inst, back


def _n_queries(prob, num_ignore):
    """(user, context) pairs with a correct item among the candidates that are left once the num_ignore most popular are dropped"""
    deg = {}
    for t in prob.train:
        deg[t[1]] = deg.get(t[1], 0) + 1
    alive = set(sorted(prob.cand, key=lambda j: -deg[j])[num_ignore:])
    return len({(t[0], t[2]) for t in prob.test if t[3] == ra.R_POS and t[1] in alive})


def _env(case, form):
    env = dict(form)
    env["CMI_RANK_BATCH"] = case["batch"]
    env["CMI_RANK_ONE_STREAM"] = "1" if case["one_stream"] else None
    return env


@gpu
@pytest.mark.parametrize("dist", ["spread", "tied"])
@pytest.mark.parametrize("case", L1_CASES, ids=_id)
def test_exact_models_equal_the_fp64_oracle_bit_for_bit(case, dist):
    model = case["model"]
    prob, st, gm = l1_problem(case, dist)
    inst, back = _instance(model, case["k"], prob, st, gm)
    F, thold = l1_reference(case, dist, prob, back, gm)
    kw = dict(bin_thold=thold, num_recs=case["num_recs"], num_ignore=case["num_ignore"], strategy=case["strategy"])
    ref, ref_lists = rank_oracle.eval_rankings(ra.TablePredict(F, prob.queries, prob.pos), prob.train, prob.test, **kw)
    assert case["num_recs"] == 1 or any(len(l) < case["num_recs"] for l in ref_lists.values())
    train, test = ra.arrays(prob.train), ra.arrays(prob.test)
    for form in case["forms"]:
        res, lists = ra.with_env(_env(case, form), lambda: inst.eval_rankings(train, test, with_lists=True, **kw))
        assert res["n_queries"] == _n_queries(prob, case["num_ignore"]), form
        assert set(lists) == set(ref_lists), form
        for key, ref_l in ref_lists.items():
            assert lists[key] == ref_l, (form, key, lists[key], ref_l)             # (item, score) pairs: == on ints and doubles, in order
        for m in rank_oracle.MEASURES:
            a, b = res[m], ref[m]
            assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12, (form, m, a, b)
        assert res["D5"] == res["D10"] == res["DN"] == 0.0
    inst.close()


@gpu
@pytest.mark.parametrize("model,k,nc", L2_CASES)
def test_arbitrary_models_within_the_forward_bound(model, k, nc):
    prob, st, gm = l2_problem(model, k, nc)
    inst, back = _instance(model, k, prob, st, gm)
    F, B, E, ok, tops = l2_reference(model, k, prob, back, gm)
    thold, n = l2_thold(model), L2_NUM_RECS
    ref, ref_lists = rank_oracle.eval_rankings(ra.TablePredict(F, prob.queries, prob.pos), prob.train, prob.test, bin_thold=thold, num_recs=n)
    train, test = ra.arrays(prob.train), ra.arrays(prob.test)
    for form in (DEFAULT, NO_SPLIT):
        env = dict(form, CMI_RANK_BATCH=None, CMI_RANK_ONE_STREAM=None)
        res, lists = ra.with_env(env, lambda: inst.eval_rankings(train, test, bin_thold=thold, num_recs=n, with_lists=True))
        assert res["n_queries"] == len(prob.queries)
        worst = 0.0
        for qi, q in enumerate(prob.queries):
            got = lists.get(q, [])
            cols = np.array([prob.pos.get(j, -1) for j, _ in got], np.intp)
            g = np.array([s for _, s in got], np.float64)
            # 1. candidates, not excluded, not twice, every score within the bound
            assert np.all(cols >= 0) and len(set(cols.tolist())) == len(cols) and bool(np.all(E[qi, cols])), (form, q)
            err = np.abs(g - F[qi, cols])
            assert np.all(err <= B[qi, cols]), (form, q, err.tolist(), B[qi, cols].tolist())
            worst = max(worst, float(np.max(err / B[qi, cols], initial=0.0)))
            # 2. descending, equal scores in ascending candidate position, strictly above the threshold
            assert all(g[i] > g[i + 1] or (g[i] == g[i + 1] and cols[i] < cols[i + 1]) for i in range(len(g) - 1)), (form, q)
            assert np.all(g > thold), (form, q)
            # 3. complete: no eligible candidate left out that beats the list's end (or, behind a short list, the threshold) by its bound
            rest = E[qi].copy()
            rest[cols] = False
            limit = g[-1] if len(g) == n else thold
            assert np.all(F[qi, rest] <= limit + B[qi, rest]), (form, q)
            # 4. where the reference alone decides, the oracle's list item for item
            if ok[qi]:
                want = [j for j, _ in ref_lists.get(q, [])]
                assert want == [prob.cand[c] for c in tops[qi]]
                assert [j for j, _ in got] == want, (form, q)
        print("  %s: worst |g - f| / B = %.3f" % ("per-query form" if form is NO_SPLIT else "split form", worst))
    inst.close()


if __name__ == "__main__":
    t0 = time.time()
    for case_ in L1_CASES:
        for dist_ in ("spread", "tied"):
            prob_, st_, gm_ = l1_problem(case_, dist_)
            F_, thold_ = l1_reference(case_, dist_, prob_, st_, gm_)
            print("layer 1 %s %s: %d queries, threshold %.6f, %d scores on it, exact sums hold" % (_id(case_), dist_, len(prob_.queries), thold_, int((F_ == thold_).sum())))
    for m_, k_, nc_ in L2_CASES:
        l2_reference(m_, k_, *l2_problem(m_, k_, nc_))
    print("%.1f s" % (time.time() - t0))
