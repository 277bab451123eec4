"""NaN, +Inf and -Inf scores through every top-N selection path, against oracle/rank_oracle.py on the models of
tests/nonfinite_scores.py (whose scores every device form computes exactly; tests/test_nonfinite_scores.py shows on the CPU that these
cases tell a selector that breaks the rule from one that keeps it).  The rule (Recommender.java:808-812 and the stable descending
sort behind it): a NaN score never enters a list, a score enters only if it is > the threshold (so -Inf never does), equal scores --
+Inf ties among them -- keep candidate order.  Lists are compared entry for entry: items, score bits, counts; the measures within the
1e-12 the fp64 ranking tests use.

Which kernels a case reaches (rank_kernels.hip unless noted):
  slab form, fp64 (RankALS, BPR: rankals_score_kernel; SLIM: its own score kernel), rank_mask<double>, then
      num_recs 10 -> rank_topn_stream<double>          num_recs 70 -> rank_topn<double>
  fp64 contraction (BiasedMF, CAMF_CUCI with FLAG_STATE_F64): rank_gemm<double>, rank_mask<double>, then as above
  fp32, default: rank_gemm_mfma_f32 (S1 and S2 with their tile maxima; on S2 rank_fix_onehot and rank_fix_tile_max),
      rank_topn_split_pruned<float>
  fp32, CMI_RANK_NO_PRUNE=1: the same slabs without maxima, rank_topn_split<float>
  fp32, CMI_RANK_NO_SPLIT=1 or num_recs 70: the per-query contraction rank_gemm_mfma_f32 (and rank_fix_onehot where the model has icBias),
      rank_mask<float>, then rank_topn_stream<float> (num_recs <= 64) or rank_topn<float> (70)
  rank_gemm<double> is followed by rank_fix_onehot too.  Contexts 2 and 3 of the CAMF models do not hold the condition whose icBias
  entries are planted: a contraction that multiplies them by the one-hot row's zeros makes NaN of scores the reference leaves alone.
  SVD++, CAMF_ICS / LCS / MCS (fp32 and fp64 state; always the per-query contraction): ext_rank_items and ext_rank_queries
      (ext_kernels.hip) build the operands, rank_gemm_mfma_f32 or rank_gemm<double> contracts them, then
      SVD++: rank_list_nonfinite_rows lists the candidates whose Q row is no number, ext_rank_mend_svdpp forms their scores again
      then rank_mask -- which, for CAMF_ICS / LCS / MCS, first multiplies the rows whose context's scale is an infinity or a NaN
          (ext_rank_queries left P_u unscaled there and recorded the scale); contexts 0, 4 and 5 have finite scales (1, 0, -1) and take
          the folded operand as before -- and rank_topn_stream (num_recs 10) or rank_topn (70), as above
  rank_tile_max, the VALU fallback of the contraction's tile maxima, is not reached: no supported configuration takes it (every
  operand length is rounded up to the matrix kernel's k step of 16).
"""
import functools
import math

import numpy as np
import pytest

from carskit_amd import capi
from oracle import rank_oracle
from tests import nonfinite_scores as nf
from tests import slim_ref as sref
from tests.util import REG, REGC, same_bits_exact, with_env

pytestmark = pytest.mark.gpu

THOLDS = (-1.0, "mode", -1e300)


def thold_of(model, t):
    return nf.mode_threshold(model) if t == "mode" else t


def check(h, model, thold, num_recs, oracle=nf.oracle, **env):
    """one evaluation against the oracle's lists and measures of the same setting; returns the lists.  (The similarity models: a zero
    score of either sign counts as +0, see nf.plus_zero; every other model's scores bit for bit, as ever.)"""
    train, test = nf.tuples_of(model)
    res, lists = with_env(lambda: h.eval_rankings(train, test, bin_thold=thold, num_recs=num_recs, with_lists=True), **env)
    ref, want = oracle(model, thold, num_recs)
    label = (model, thold, num_recs, env)
    canon = nf.plus_zero if model in nf.SIM_MODELS else (lambda x: x)
    assert set(lists) == set(want) and len(want) > 20, (label, sorted(set(lists) ^ set(want))[:5])
    for key, ref_l in want.items():
        got = lists[key]
        assert len(got) == len(ref_l), (label, key, len(got), len(ref_l))
        assert [i for i, _ in got] == [i for i, _ in ref_l], (label, key, got[:12], ref_l[:12])
        assert same_bits_exact(canon([s for _, s in got]), canon([s for _, s in ref_l])), (label, key)
    for m, b in ref.items():
        a = res[m]
        assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12, (label, m, a, b)
    return lists


# ---- the slab form: fp64 scores filled by a model's own kernel ------------------------------------------------------------------------
def cells_2d():
    train, _ = nf.tuples()
    return sorted(set(zip(train[0].tolist(), train[1].tolist())))


@functools.lru_cache(maxsize=None)
def factor_handle(name):
    cls, flags = {"rankals": (capi.RankALSInstance, 0), "bpr": (capi.BPRInstance, capi.BPR_FLAG_STRICT)}[name]
    P, Q = nf.factors()
    h = cls(nf.K, nf.NU, nf.N_ITEMS, flags=flags)
    cells = cells_2d()
    h.set_ratings([c[0] for c in cells], [c[1] for c in cells], [3.0] * len(cells))
    h.set_model(P, Q)
    return h


@pytest.mark.parametrize("num_recs", [10, 70])
@pytest.mark.parametrize("name", ["rankals", "bpr"])
def test_slab_form_of_the_factor_models(name, num_recs):
    h = factor_handle(name)
    for t in THOLDS:
        lists = check(h, "PQ", thold_of("PQ", t), num_recs)
        assert check(h, "PQ", thold_of("PQ", t), num_recs, CMI_RANK_BATCH=3) == lists


# the items that have a column, none of them a candidate: every neighbour list is these, one per factor
SLIM_ANCHORS = tuple([j for j in range(2000, nf.N_ITEMS) if j not in set(nf.items()[0])][:nf.K])


@functools.lru_cache(maxsize=None)
def slim_model():
    """SLIM with the non-finites in W: item j's weights from the anchors are Q[j]; user u's cells on the anchors are P[u] (users 9 and
    12, whose P[u][0] is no number, take +1/2 and -1/2; a zero is no cell, so a 0 * Inf of the factor models is no term here)"""
    P, Q = nf.factors()
    P = P.copy()
    P[nf.U_NAN, 0], P[nf.U_NINF, 0] = 0.5, -0.5
    assert not set(SLIM_ANCHORS) & set(nf.items()[0]) and np.isfinite(P).all()
    cells = [(u, SLIM_ANCHORS[f], float(P[u, f])) for u in range(nf.NU) for f in range(nf.K) if P[u, f] != 0.0]
    cand, _ = nf.items()
    ref = sref.Slim(nf.NU, nf.N_ITEMS, cells)                      # (the restatement: which cells of a row Ru.contains finds is its business)
    nbr = ref.neighbors(0)
    assert nbr[0] == list(SLIM_ANCHORS)
    with np.errstate(invalid="ignore"):
        s = np.array([[ref.predict(nbr, Q, u, j) for j in cand] for u in range(nf.NU)])
    return cells, Q, s


@functools.lru_cache(maxsize=None)
def slim_oracle(model, thold, num_recs):
    _, _, s = slim_model()
    _, pos = nf.items()
    train, test = nf.tuples()
    return rank_oracle.eval_rankings(lambda u, j, c: float(s[u, pos[j]]), nf.as_lists(train), nf.as_lists(test), bin_thold=thold,
                                     num_recs=num_recs)


@pytest.mark.parametrize("num_recs", [10, 70])
def test_slab_form_of_slim_with_non_finite_weights(num_recs):
    cells, Q, s = slim_model()
    assert np.sum(s == np.inf) > 100 and np.sum(s == -np.inf) > 100 and np.isnan(s).sum() > 20
    h = capi.SLIMInstance(nf.NU, nf.N_ITEMS)
    h.set_ratings([c[0] for c in cells], [c[1] for c in cells], [c[2] for c in cells])
    h.build_neighbors(0)
    ptr, idx = h.neighbors()
    assert all(idx[ptr[j]:ptr[j + 1]].tolist() == list(SLIM_ANCHORS) for j in (0, nf.items()[0][0], nf.N_ITEMS - 1))
    h.set_weights(np.ascontiguousarray(Q).reshape(-1))
    for t in (-1.0, 0.0, -1e300):
        lists = check(h, "SLIM", t, num_recs, slim_oracle)
        assert check(h, "SLIM", t, num_recs, slim_oracle, CMI_RANK_BATCH=3) == lists
    h.close()


# ---- the MF family ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mf_handle(model, flags):
    train, _ = nf.tuples()
    h = capi.Instance(model, nf.K, nf.NU, nf.N_ITEMS, nf.N_CONDS, flags=flags)
    h.set_hparams(REG, REG, REG, REGC, nf.GM)
    if model != "BiasedMF":
        h.set_ratings(*train, nf.CTX_PTR, nf.CTX_CONDS)
    h.set_states(nf.state(model))
    return h


@pytest.mark.parametrize("num_recs", [10, 70])
@pytest.mark.parametrize("model", ["BiasedMF", "CAMF_CUCI"])
def test_fp64_contraction_form(model, num_recs):
    h = mf_handle(model, capi.FLAG_STATE_F64)
    for t in THOLDS:
        lists = check(h, model, thold_of(model, t), num_recs)
        assert check(h, model, thold_of(model, t), num_recs, CMI_RANK_BATCH=23) == lists


FORMS = {"pruned": {}, "plain": {"CMI_RANK_NO_PRUNE": 1}, "per_query": {"CMI_RANK_NO_SPLIT": 1}}


@pytest.mark.parametrize("num_recs", [10, 64, 70])
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("model", ["BiasedMF", "CAMF_CI", "CAMF_CUCI"])
def test_fp32_forms(model, form, num_recs):
    """(num_recs 70 takes the per-query form whatever the environment says: the split selection keeps its list in 64 lanes)"""
    h = mf_handle(model, 0)
    for t in THOLDS:
        lists = check(h, model, thold_of(model, t), num_recs, **FORMS[form])
        assert check(h, model, thold_of(model, t), num_recs, CMI_RANK_BATCH=23, **FORMS[form]) == lists


@pytest.mark.parametrize("model", ["BiasedMF", "CAMF_CI", "CAMF_CUCI"])
def test_pruned_and_plain_split_forms_agree_entry_for_entry(model):
    h = mf_handle(model, 0)
    train, test = nf.tuples()
    for t in THOLDS:
        for num_recs in (10, 64):
            run = lambda: h.eval_rankings(train, test, bin_thold=thold_of(model, t), num_recs=num_recs, with_lists=True)  # noqa: E731
            pruned, plain = run(), with_env(run, CMI_RANK_NO_PRUNE=1)
            assert pruned[1] == plain[1] and len(plain[1]) > 20
            for m, v in plain[0].items():
                assert np.float64(v).tobytes() == np.float64(pruned[0][m]).tobytes() or (math.isnan(v) and math.isnan(pruned[0][m])), m


# ---- SVD++ and the similarity models: operand builders of their own, always the per-query contraction ----------------------------------
@functools.lru_cache(maxsize=None)
def ext_handle(model, flags):
    """the injected model (never trained): set_ratings gives SVD++ its users' item lists and the others their context table"""
    train, _ = nf.tuples_of(model)
    h = capi.Instance(model, nf.K, nf.NU, nf.N_ITEMS, nf.SIM_CONDS if model in nf.SIM_MODELS else nf.N_CONDS, flags=flags | capi.FLAG_SCHED_SERIAL)
    h.set_hparams(REG, REG, REG, REGC, nf.GM)
    if model == "SVD++":
        h.set_ratings(train[0], train[1], None, train[3])
    else:
        h.set_sim_params(nf.SIM_NUM_F, nf.SIM_DIMS, nf.SIM_EMPTY)
        h.set_ratings(*train, nf.SIM_CTX_PTR, nf.SIM_CTX_CONDS)
    st = nf.ext_state(model)
    h.set_states(st)
    back = h.get_states()
    for name, a in st.items():
        assert np.array_equal(back[name], a, equal_nan=True), name           # every entry is an fp32 number, an infinity or a NaN
    return h


@pytest.mark.parametrize("num_recs", [10, 70])
@pytest.mark.parametrize("state", ["f32", "f64"])
@pytest.mark.parametrize("model", nf.EXT_MODELS)
def test_ext_operand_forms(model, state, num_recs):
    """scales of +Inf, -Inf, NaN, 0, -1 and 1 (CAMF_MCS: no +Inf) against dot products that are positive, negative, exactly 0, +Inf, -Inf
    and NaN; SVD++ with planted Y rows, biases, a row constant of -Inf, the user without a rated item, and Q rows that are no numbers"""
    h = ext_handle(model, capi.FLAG_STATE_F64 if state == "f64" else 0)
    for t in THOLDS:
        lists = check(h, model, thold_of(model, t), num_recs)
        assert check(h, model, thold_of(model, t), num_recs, CMI_RANK_BATCH=23) == lists
        assert check(h, model, thold_of(model, t), num_recs, CMI_RANK_NO_SPLIT=1) == lists      # (no split form: the variable changes nothing)
