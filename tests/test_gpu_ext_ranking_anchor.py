"""Top-N evaluation of SVD++, CAMF_ICS, CAMF_LCS and CAMF_MCS -- the operand builders ext_rank_items / ext_rank_queries
(ext_kernels.hip) in front of the per-query contraction (rank_gemm_mfma_f32 for fp32 state, rank_gemm<double> for fp64), rank_mask and
rank_topn_stream / rank_topn -- against oracle/rank_oracle.py over the score table of tests/ext_rank_anchor.py, with NO training in
between: the model is injected with set_states, read back, and the reference scores are computed from exactly those values.  The two
layers, their premises and the four checks of layer 2 are those of tests/test_gpu_ranking_f32_anchor.py; the derivation of the bound
per model is in the docstring of tests/ext_rank_anchor.py.

Layer 1: exact-grid states, both value distributions, fp32 and fp64 state: queries, lists and scores equal the oracle's with ==, the
18 measures within 1e-12; the default environment and CMI_RANK_NO_SPLIT=1 give the identical answer (these models have no split form).
Layer 2: arbitrary states, all four models at (k, candidates) in {(17, 129), (64, 513), (128, 513), (130, 513)}, fp32 and fp64 state.

The premises (exact sums in four orders; the unambiguous share of at least 80 %; the restatement against oracle_c.SimOracle.predict)
are host-only tests of this module and run without a device."""
import math
import zlib

import numpy as np
import pytest

from carskit_amd import capi
from oracle import oracle_c, rank_oracle
from tests import ext_rank_anchor as xa
from tests import rank_anchor as ra
from tests import util

gpu = pytest.mark.gpu


def _case(model, k, nc, n_users=60, n_dims=3, cpd=4, num_f=0, num_recs=10, batch=None, num_ignore=0, strategy="ucu", degrees=(0, 1, 4, 16)):
    return dict(model=model, k=k, nc=nc, n_users=n_users, n_dims=n_dims, cpd=cpd, num_f=num_f, num_recs=num_recs, batch=batch,
                num_ignore=num_ignore, strategy=strategy, degrees=degrees)


# what a case reaches (kp = ceil16 of the operand length: k, and k + 1 for SVD++ whose last column is [1 | itemBias]):
#   SVD++-15: k + 1 = 16, the bias column is the last of the only k step    SVD++-16: it opens a second k step, 15 padded columns behind it
#   SVD++-17: the odd count    SVD++-128: 129 columns, the builders' 128-thread stride loops take a second pass for the bias column alone;
#   degrees up to 64; num_recs 70 is rank_topn       every SVD++ case: user 4 has no training tuple (the `ie > ib` branch)
#   CAMF_ICS-1: one factor, one dimension    CAMF_ICS-17: 16 dimensions of 2 conditions, the longest context the models allow; num_ignore 5
#   CAMF_ICS-128: 4097 candidates (the selection's chunk of 64 tiles plus one), three query batches of 127
#   CAMF_LCS: num_f 1, 130 (strategy uc), 65 (num_recs 70); 7 in layer 2      CAMF_MCS-130: k past 128 in the query builder's stride loop,
#   two dimensions: every context that differs in both is a (3, 4, 5) / 8 pair
#   candidates 63, 64, 65 / 127, 128, 129 (twice) / 513 / 4097; num_recs 1, 5, 10, 64, 70
L1_CASES = [
    _case("SVD++", 15, 63, num_recs=5),
    _case("SVD++", 16, 65, num_recs=64),
    _case("SVD++", 17, 127),
    _case("SVD++", 128, 129, num_recs=70, degrees=(0, 1, 4, 16, 64)),
    _case("CAMF_ICS", 1, 64, n_dims=1, num_recs=1),
    _case("CAMF_ICS", 17, 127, n_dims=16, cpd=2, num_ignore=5),
    _case("CAMF_ICS", 128, 4097, n_users=254, batch="127"),
    _case("CAMF_LCS", 64, 65, num_f=1),
    _case("CAMF_LCS", 33, 128, num_f=130, strategy="uc"),
    _case("CAMF_LCS", 16, 129, num_f=65, num_recs=70),
    _case("CAMF_MCS", 48, 129),
    _case("CAMF_MCS", 130, 513, n_dims=2, num_recs=64),
]

L2_SHAPES = ((17, 129), (64, 513), (128, 513), (130, 513))
L2_CASES = [(m, k, nc, (65 if (m, k) == ("CAMF_LCS", 64) else 7 if m == "CAMF_LCS" else 0)) for m in xa.MODELS for k, nc in L2_SHAPES]
L2_NUM_RECS, L2_USERS, L2_DEGREES = 10, 60, (0, 1, 3, 4, 17, 64)


def _id(c):
    return "%s-k%d-nc%d" % (c["model"], c["k"], c["nc"])


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


# ---- host-only parts ------------------------------------------------------------------------------------------------------------
def l1_problem(case, dist):
    prob = xa.make_problem(case["model"], case["nc"], case["n_users"], case["n_dims"], case["cpd"], _seed(_id(case), dist), degrees=case["degrees"])
    st, gm = xa.exact_state(case["model"], prob, case["k"], dist, _seed(_id(case), dist, "state"), case["num_f"])
    return prob, st, gm


def l1_reference(case, dist, prob, st, gm):
    """From the (read-back) state: the score table, the threshold, the short-list query (appended to prob.train) and the premise of
    layer 1; returns (F, thold)."""
    model = case["model"]
    Fx = xa.score_table(model, st, gm, prob, prob.queries)
    F = Fx.astype(np.float64)
    assert np.array_equal(F.astype(xa.LD), Fx)                                        # every score is a double: nothing was rounded
    thold, n_at = ra.modal_score(F)
    if dist == "tied":                    # ON the value most scores take: `score > thold` is strict, all of those must stay out
        assert n_at >= 0.05 * F.size and -7.0 < thold < 5.0, (thold, n_at)
    else:
        thold = 2.5 if model == "SVD++" else float(np.median(F))
    xa.check_exact_premise(model, st, gm, prob, F, prob.queries, _seed(_id(case), dist, "premise"))
    short = ra.add_short_query(prob, F, prob.queries, thold, case["num_recs"], _seed(_id(case), "short"))
    E = ra.eligible_mask(prob, prob.queries)
    n_pass = ((F > thold) & E).sum(axis=1)
    assert n_pass[prob.queries.index(short)] < case["num_recs"]
    assert case["num_recs"] == 1 or 0 < n_pass[prob.queries.index(short)]
    assert max(len(x) for x in ra.excluded_columns(prob).values()) >= min(20, case["nc"] // 4)
    assert np.mean(n_pass > 0) >= 0.5
    return F, thold


def l2_problem(model, k, nc, num_f, f64):
    prob = xa.make_problem(model, nc, L2_USERS, 3, 4, _seed("l2", model, k, nc), degrees=L2_DEGREES)
    st, gm = xa.loud_state(model, prob, k, _seed("l2state", model, k, nc), num_f)
    return prob, {n: a.astype(np.float64 if f64 else np.float32) for n, a in st.items()}, gm


def l2_reference(model, k, num_f, f64, prob, st, gm):
    """F (extended precision), B, eligibility, the threshold, the unambiguous queries and their expected lists -- from the reference
    alone; asserts the 80 % cap."""
    Fx = xa.score_table(model, st, gm, prob, prob.queries)
    F = Fx.astype(np.float64)
    B = xa.error_bound(model, st, gm, prob, prob.queries, k, xa.U64 if f64 else ra.U32, num_f)
    E = ra.eligible_mask(prob, prob.queries)
    thold = 2.5 if model == "SVD++" else float(np.median(F))
    ok, tops = ra.unambiguous(F, B, E, thold, L2_NUM_RECS)
    share = float(ok.mean())
    print("layer 2 %s k=%d nc=%d %s: %d queries, threshold %.4f, mean B %.2e, unambiguous share %.3f"
          % (model, k, len(prob.cand), "f64" if f64 else "f32", len(ok), thold, B.mean(), share))
    assert share >= 0.80, share
    return Fx, F, B, E, thold, ok, tops


@pytest.mark.parametrize("dist", ["spread", "tied"])
@pytest.mark.parametrize("case", L1_CASES, ids=_id)
def test_layer1_premise_holds_on_the_host(case, dist):
    prob, st, gm = l1_problem(case, dist)
    l1_reference(case, dist, prob, st, gm)
    if case["model"] == "SVD++":
        deg = {len(r) for r in prob.rated}
        assert deg <= set(case["degrees"]) and 0 in deg and max(deg) == max(case["degrees"])
    else:
        # the reference's contexts: one condition per dimension; the all-empty context; contexts empty in some dimensions only
        assert all(len(c) == case["n_dims"] and all(i * case["cpd"] <= x < (i + 1) * case["cpd"] for i, x in enumerate(c)) for c in prob.ctxs)
        assert prob.ctxs[0] == prob.empty.tolist()
        if case["n_dims"] > 1:
            assert sum(0 < sum(x == e for x, e in zip(c, prob.empty.tolist())) < case["n_dims"] for c in prob.ctxs) >= 3


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("model,k,nc,num_f", L2_CASES)
def test_layer2_inputs_are_mostly_unambiguous(model, k, nc, num_f, f64):
    prob, st, gm = l2_problem(model, k, nc, num_f, f64)
    l2_reference(model, k, num_f, f64, prob, st, gm)
    if model == "SVD++":
        assert {len(r) for r in prob.rated} == set(L2_DEGREES)


def _sim_oracle(model, k, prob, st, gm):
    u, j, c, r = ra.arrays(prob.model_train)
    return oracle_c.SimOracle(model, k, prob.n_users, prob.n_items, prob.n_conds, u, j, c, r, prob.ctx_ptr, prob.ctx_conds, prob.empty,
                              {n: np.asarray(a, np.float64) for n, a in st.items()}, gm, util.REG, util.REG, util.REG, util.REGC,
                              n_ctx_dims=prob.n_dims)


@pytest.mark.parametrize("model", xa.MODELS)
def test_restatement_is_the_oracle_predict(model):
    """score_seq and the table against oracle_c.SimOracle.predict on 200 (user, item, context) triples: bit for bit on an exact-grid state;
    on an arbitrary one within 2 gamma_n(2^-53) A (tests/ext_rank_anchor.py; the worst observed difference is printed)"""
    num_f = 7 if model == "CAMF_LCS" else 0
    case = _case(model, 17, 127, num_f=num_f)
    prob, st, gm = l1_problem(case, "spread")
    rng = np.random.default_rng(5)
    orc = _sim_oracle(model, 17, prob, st, gm)
    F = xa.score_table(model, st, gm, prob, prob.queries)
    for _ in range(200):
        qi, ci = int(rng.integers(len(prob.queries))), int(rng.integers(len(prob.cand)))
        (u, c), j = prob.queries[qi], prob.cand[ci]
        assert orc.predict(u, j, c) == xa.score_seq(model, st, gm, prob, u, j, c) == float(F[qi, ci])
    prob, st, gm = l2_problem(model, 17, 129, num_f, True)
    orc = _sim_oracle(model, 17, prob, st, gm)
    F = xa.score_table(model, st, gm, prob, prob.queries)
    A = xa.score_table(model, st, gm, prob, prob.queries, absolute=True).astype(np.float64)
    n = xa.n_roundings(model, prob, 17, prob.queries, num_f)
    worst = 0.0
    for _ in range(200):
        qi, ci = int(rng.integers(len(prob.queries))), int(rng.integers(len(prob.cand)))
        (u, c), j = prob.queries[qi], prob.cand[ci]
        a, b = orc.predict(u, j, c), xa.score_seq(model, st, gm, prob, u, j, c)
        bar = 2.0 * n[qi] * xa.U64 * A[qi, ci]
        assert abs(a - b) <= bar and abs(xa.LD(b) - F[qi, ci]) <= bar, (a, b, F[qi, ci], bar)
        worst = max(worst, abs(a - b) / bar)
    print("%s: worst |oracle - restatement| / bar = %.3f" % (model, worst))


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
def _instance(model, k, prob, st, gm, num_f, f64):
    """The injected model: set_ratings gives SVD++ its users' item lists and the others their context table (no epoch is ever run);
    returns the instance and the state as the device holds it."""
    inst = capi.Instance(model, k, prob.n_users, prob.n_items, prob.n_conds, flags=capi.FLAG_SCHED_SERIAL | (capi.FLAG_STATE_F64 if f64 else 0))
    inst.set_hparams(util.REG, util.REG, util.REG, util.REGC, gm)
    u, j, c, r = ra.arrays(prob.model_train)
    if model == "SVD++":
        inst.set_ratings(u, j, None, r)
    else:
        inst.set_sim_params(max(num_f, 1), prob.n_dims, prob.empty)
        inst.set_ratings(u, j, c, r, prob.ctx_ptr, prob.ctx_conds)
    inst.set_states(st)
    back = inst.get_states(np.float64 if f64 else np.float32)
    for name, a in st.items():
        assert back[name].dtype == a.dtype and np.array_equal(back[name], a), name
    return inst, back


def _n_queries(prob, num_ignore):
    """(user, context) pairs with a correct item among the candidates that are left once the num_ignore most popular are dropped"""
    deg = {}
    for t in prob.train:
        deg[t[1]] = deg.get(t[1], 0) + 1
    alive = set(sorted(prob.cand, key=lambda j: -deg[j])[num_ignore:])
    return len({(t[0], t[2]) for t in prob.test if t[3] == ra.R_POS and t[1] in alive})


@gpu
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("dist", ["spread", "tied"])
@pytest.mark.parametrize("case", L1_CASES, ids=_id)
def test_exact_models_equal_the_oracle_bit_for_bit(case, dist, f64):
    model = case["model"]
    prob, st, gm = l1_problem(case, dist)
    if f64:
        st = {n: a.astype(np.float64) for n, a in st.items()}
    inst, back = _instance(model, case["k"], prob, st, gm, case["num_f"], f64)
    F, thold = l1_reference(case, dist, prob, {n: a.astype(np.float32) for n, a in back.items()}, gm)
    kw = dict(bin_thold=thold, num_recs=case["num_recs"], num_ignore=case["num_ignore"], strategy=case["strategy"])
    ref, ref_lists = rank_oracle.eval_rankings(ra.TablePredict(F, prob.queries, prob.pos), prob.train, prob.test, **kw)
    assert case["num_recs"] == 1 or any(len(l) < case["num_recs"] for l in ref_lists.values())
    train, test = ra.arrays(prob.train), ra.arrays(prob.test)
    answers = []
    for no_split in (None, "1"):
        env = {"CMI_RANK_NO_SPLIT": no_split, "CMI_RANK_NO_PRUNE": None, "CMI_RANK_BATCH": case["batch"], "CMI_RANK_ONE_STREAM": None}
        res, lists = ra.with_env(env, lambda: inst.eval_rankings(train, test, with_lists=True, **kw))
        assert res["n_queries"] == _n_queries(prob, case["num_ignore"]), no_split
        assert set(lists) == set(ref_lists), no_split
        for key, ref_l in ref_lists.items():
            assert lists[key] == ref_l, (no_split, key, lists[key], ref_l)         # (item, score) pairs: == on ints and doubles, in order
        for m in rank_oracle.MEASURES:
            a, b = res[m], ref[m]
            assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12, (no_split, m, a, b)
        answers.append((res, lists))
    util.assert_same_rankings(answers[1], answers[0], "CMI_RANK_NO_SPLIT")       # these models have no split form: the variable changes nothing
    inst.close()


@gpu
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("model,k,nc,num_f", L2_CASES)
def test_arbitrary_models_within_the_forward_bound(model, k, nc, num_f, f64):
    prob, st, gm = l2_problem(model, k, nc, num_f, f64)
    inst, back = _instance(model, k, prob, st, gm, num_f, f64)
    Fx, F, B, E, thold, ok, tops = l2_reference(model, k, num_f, f64, prob, back, gm)
    n = L2_NUM_RECS
    ref, ref_lists = rank_oracle.eval_rankings(ra.TablePredict(F, prob.queries, prob.pos), prob.train, prob.test, bin_thold=thold, num_recs=n)
    train, test = ra.arrays(prob.train), ra.arrays(prob.test)
    env = {"CMI_RANK_NO_SPLIT": None, "CMI_RANK_NO_PRUNE": None, "CMI_RANK_BATCH": None, "CMI_RANK_ONE_STREAM": None}
    res, lists = ra.with_env(env, lambda: inst.eval_rankings(train, test, bin_thold=thold, num_recs=n, with_lists=True))
    assert res["n_queries"] == len(prob.queries)
    worst = 0.0
    for qi, q in enumerate(prob.queries):
        got = lists.get(q, [])
        cols = np.array([prob.pos.get(j, -1) for j, _ in got], np.intp)
        g = np.array([s for _, s in got], np.float64)
        # 1. candidates, not excluded, not twice, every score within the bound (of the extended-precision score)
        assert np.all(cols >= 0) and len(set(cols.tolist())) == len(cols) and bool(np.all(E[qi, cols])), q
        err = np.abs(g.astype(xa.LD) - Fx[qi, cols]).astype(np.float64)
        assert np.all(err <= B[qi, cols]), (q, err.tolist(), B[qi, cols].tolist())
        worst = max(worst, float(np.max(err / B[qi, cols], initial=0.0)))
        # 2. descending, equal scores in ascending candidate position, strictly above the threshold
        assert all(g[i] > g[i + 1] or (g[i] == g[i + 1] and cols[i] < cols[i + 1]) for i in range(len(g) - 1)), q
        assert np.all(g > thold), q
        # 3. complete: no eligible candidate left out that beats the list's end (or, behind a short list, the threshold) by its bound
        rest = E[qi].copy()
        rest[cols] = False
        limit = g[-1] if len(g) == n else thold
        assert np.all(F[qi, rest] <= limit + B[qi, rest]), q
        # 4. where the reference alone decides, the oracle's list item for item
        if ok[qi]:
            want = [j for j, _ in ref_lists.get(q, [])]
            assert want == [prob.cand[c] for c in tops[qi]]
            assert [j for j, _ in got] == want, q
    print("  worst |g - f| / B = %.3f" % worst)
    inst.close()
