"""The construction of tests/nonfinite_scores.py, checked without a GPU: its finite scores are exact in fp32 and fp64 in every
association, every planted class and list situation occurs, and each deliberately wrong selector changes at least one list -- so the
GPU cases of tests/test_gpu_rank_nonfinite.py can tell a kernel that breaks the reference's rule from one that keeps it."""
import math

import numpy as np
import pytest

from carskit_amd import capi
from oracle import rank_oracle
from tests import nonfinite_scores as nf
from tests.util import same_bits

MODELS = ("PQ",) + nf.MF_MODELS
THOLDS = (-1.0, "mode", -1e300)
RECS = (10, 64, 70)


def thold_of(model, t):
    return nf.mode_threshold(model) if t == "mode" else t


def plan(thold):
    train, test = nf.tuples()
    return capi.rank_plan(nf.NU, nf.N_ITEMS, train, test, thold, 0)


def test_the_candidates_sit_where_the_construction_puts_them():
    cand, queries = plan(-1.0)
    train, _ = nf.tuples()
    assert cand == nf.items()[0] == rank_oracle.java_int_hashset_order(train[1].tolist())
    assert len(cand) == nf.NC == 64 * 9 + 5 and cand != sorted(cand)
    assert {u for u, _, _, _ in queries} == set(range(nf.NU))
    assert len(set(nf.A) & set(nf.B)) == 4 and set(nf.TILE) <= set(nf.A) and nf.TILE[0] % 64 == 0 and len(nf.TILE) == 64
    assert set(nf.SPECIAL) == {0, 63, 64, 511, 512, nf.NC - 1, (nf.NC // 64) * 64 - 1} <= set(nf.A)
    assert not (set(nf.SURVIVORS) | set(nf.IB_PINF) | set(nf.IB_NINF) | set(nf.IC_PINF)) & (set(nf.A) | set(nf.B))
    assert set(nf.IC_NINF) & set(nf.A)


@pytest.mark.parametrize("model", MODELS)
def test_finite_entries_are_eighths_and_the_scores_are_exact_in_fp32_and_fp64(model):
    for name, a in nf.state(model).items():
        fin = a[np.isfinite(a)]
        assert np.all(fin * 8 == np.rint(fin * 8)) and np.all(np.abs(fin) <= 0.5), name
    assert nf.K <= 16 and (nf.GM * 8).is_integer()
    ref = nf.scores(model)
    assert np.isfinite(ref).sum() > ref.size // 2
    for dtype in (np.float64, np.float32):
        for form in ("chain", "reversed", "split"):
            got = nf.score_slab(model, dtype, form)
            assert got.dtype == dtype
            assert same_bits(got.astype(np.float64), ref), (dtype, form)   # (every number and infinity bit for bit, NaN where NaN)
    fin = ref[np.isfinite(ref)]
    # few distinct values (sixteenths inside +-2.25: at most 73) over 581 candidates: ties at the cut are common
    assert len(np.unique(fin)) <= 73 and np.all(fin * 16 == np.rint(fin * 16)) and np.abs(fin).max() <= 2.25


def classes(row):
    return int(np.sum(row == np.inf)), int(np.sum(row == -np.inf)), int(np.isnan(row).sum())


def test_planted_classes_per_user_in_the_factor_models():
    s = nf.scores("PQ")
    a_only, b_only, both = len(set(nf.A) - set(nf.B)), len(set(nf.B) - set(nf.A)), len(set(nf.A) & set(nf.B))
    assert (a_only, b_only, both) == (67, 3, 4)
    P, Q = nf.factors()
    assert [tuple(P[u, :2]) for u in range(9)] == nf.SIGNS
    want = {nf.U_PP: (a_only, b_only, both), nf.U_PM: (a_only + b_only + both, 0, 0), nf.U_P0: (a_only, 0, b_only + both),
            nf.U_MP: (0, a_only + b_only + both, 0), nf.U_MM: (b_only, a_only, both), nf.U_M0: (0, a_only, b_only + both),
            nf.U_0P: (0, b_only, a_only + both), nf.U_0M: (b_only, 0, a_only + both), nf.U_00: (0, 0, a_only + b_only + both),
            nf.U_NAN: (0, 0, nf.NC), nf.U_LOW: (b_only, a_only, both)}
    for c in range(4):
        for u, w in want.items():
            assert classes(s[c, u]) == w, (u, c)
        pinf, ninf, nan = classes(s[c, nf.U_NINF])
        assert pinf == 0 and ninf + nan == nf.NC and ninf > 100 and nan > 100
        # position 0: NaN for one user and +Inf for another; a whole tile NaN for one user and +Inf for another
        assert math.isnan(s[c, nf.U_PP, 0]) and s[c, nf.U_PM, 0] == np.inf
        assert np.isnan(s[c, nf.U_0P, 192:256]).all() and np.all(s[c, nf.U_PM, 192:256] == np.inf)
        low = s[c, nf.U_LOW]
        fin = np.isfinite(low)
        assert sorted(np.nonzero(fin & (low > -1.0))[0].tolist()) == list(nf.SURVIVORS)


@pytest.mark.parametrize("model", nf.MF_MODELS)
def test_planted_classes_in_the_mf_family(model):
    s = nf.scores(model)
    s1, s2, rc = nf.split_parts(model)
    assert np.isinf(rc[:, nf.U_RC]).all() and np.all(rc[:, nf.U_RC] < 0)           # a row constant of -Inf: nothing of that user passes
    assert not np.any(s[:, nf.U_RC] > -np.inf)
    if s2 is None:
        assert np.all(s1[nf.U_00, list(nf.IB_PINF)] == np.inf) and np.all(s1[nf.U_00, list(nf.IB_NINF)] == -np.inf)
        return
    # the S2 slab holds both infinities in the contexts with condition 0 and none in the others
    for c in range(4):
        holds = 0 in nf.CTX[c]
        assert bool(np.any(s2[c] == np.inf)) == holds and bool(np.any(s2[c] == -np.inf)) == holds and not np.isnan(s2[c]).any()
    # +Inf in S1 and -Inf in S2 at one candidate: a NaN that is in neither slab
    hit = [(u, c, p) for u in (nf.U_PP, nf.U_PM) for c in (0, 1) for p in nf.IC_NINF
           if s1[u, p] == np.inf and s2[c, p] == -np.inf and math.isnan(s[c, u, p])]
    assert hit
    # in the contexts without condition 0 the reference never reads the planted icBias entries: those scores are finite
    for c in (2, 3):
        assert np.isfinite(s[c, nf.U_00][list(nf.IC_NINF[2:] + nf.IC_PINF)]).all()
    for c in (0, 1):
        assert np.all(s[c, nf.U_00][list(nf.IC_PINF)] == np.inf) and s[c, nf.U_00, nf.IC_NINF[2]] == -np.inf


def test_a_one_hot_contraction_left_alone_would_be_told_apart():
    """the zeros of a context's one-hot row against the planted icBias entries: NaN where the reference's score is a number or +Inf"""
    ref, raw = nf.scores("CAMF_CI"), nf.score_slab("CAMF_CI", np.float32, "onehot").astype(np.float64)
    for c in (0, 1):
        assert same_bits(raw[c], ref[c])
    for c in (2, 3):
        spoiled = np.isnan(raw[c]) & ~np.isnan(ref[c])
        assert spoiled[:, list(nf.IC_NINF + nf.IC_PINF)].any(axis=0).all() and not spoiled[:, 10].any()
        assert np.isfinite(ref[c][spoiled]).any() and np.any(ref[c][spoiled] == np.inf)
        assert same_bits(raw[c][~spoiled], ref[c][~spoiled])


def situations(model, thold, num_recs):
    """which of the list situations occur among the oracle's lists of one setting"""
    cand, pos = nf.items()
    _, queries = plan(thold)
    s = nf.scores(model)
    _, lists = nf.oracle(model, thold, num_recs)
    seen = set()
    for u, c, correct, excl in queries:
        keep = np.array([p not in set(excl) for p in range(nf.NC)])
        row = s[c, u]
        n_pinf = int(np.sum((row == np.inf) & keep))
        n_pass = int(np.sum((row > thold) & keep))
        got = lists.get((u, c))
        if got is None:
            assert n_pass == 0
            if not np.any(np.isfinite(row[keep])) and n_pinf == 0:
                seen.add("none: only NaN and -Inf")
            continue
        assert len(got) == min(n_pass, num_recs) and not any(math.isnan(v) for _, v in got)
        first_pinf = [cand[p] for p in range(nf.NC) if keep[p] and row[p] == np.inf][:num_recs]
        assert [j for j, v in got if v == np.inf] == first_pinf          # +Inf ties keep candidate order, in front of everything else
        if n_pinf > num_recs:
            seen.add("more +Inf than num_recs")
        if 0 < n_pinf < num_recs and len(got) == num_recs and got[-1][1] < np.inf:
            seen.add("fewer +Inf than num_recs, then finite")
        if len(got) < num_recs:
            seen.add("short list")
        if any(row[p] == np.inf for p in excl):
            assert not {cand[p] for p in excl} & {j for j, _ in got}
            seen.add("+Inf item excluded")
        if any(row[pos[j]] == np.inf and j in [i for i, _ in got] for j in correct):
            seen.add("+Inf item correct")
    return seen


@pytest.mark.parametrize("model", MODELS)
def test_every_list_situation_occurs(model):
    all_seen = set()
    for num_recs in RECS:
        seen = situations(model, -1.0, num_recs)
        print(model, num_recs, sorted(seen))
        assert {"more +Inf than num_recs", "fewer +Inf than num_recs, then finite", "none: only NaN and -Inf", "+Inf item excluded",
                "+Inf item correct"} <= seen, (num_recs, seen)
        all_seen |= seen
    assert "short list" in situations(model, -1.0, 10)
    # the +Inf item that is a correct item moves the measures: without it user 1's first context has no hit at the top
    res, lists = nf.oracle(model, -1.0, 10)
    cand, _ = nf.items()
    if model == "PQ":
        assert lists[(nf.U_PM, 0)][0] == (cand[0], np.inf) and cand[63] not in [j for j, _ in lists[(nf.U_PM, 0)]]
        assert lists[(nf.U_PM, 1)][:2] == [(cand[0], np.inf), (cand[63], np.inf)]
        assert res["MRR10"] > 0.0
    # a threshold exactly on the most frequent finite score: > and >= give different lists
    t = nf.mode_threshold(model)
    _, queries = plan(t)
    s = nf.scores(model)
    assert np.sum(s == t) >= 0.05 * np.isfinite(s).sum()
    _, strict = nf.oracle(model, t, 70)
    loose = nf.lists_by(model, queries, np.nextafter(t, -np.inf), 70)
    assert not nf.same_lists(strict, loose)


RULES = ("nan_passes", "nan_is_pinf", "ninf_admitted", "pinf_descending", "full_accepts_pinf", "nan_bound")


@pytest.mark.parametrize("model", MODELS)
def test_the_reference_selector_is_the_oracle_and_every_wrong_selector_is_caught(model):
    caught = {r: 0 for r in RULES}
    for t in THOLDS:
        thold = thold_of(model, t)
        _, queries = plan(thold)
        bounds = nf.pruning_bounds(model, queries, propagate_nan=True)
        for num_recs in RECS:
            _, want = nf.oracle(model, thold, num_recs)
            assert nf.same_lists(nf.lists_by(model, queries, thold, num_recs), want)
            for rule in RULES:
                got = nf.lists_by(model, queries, thold, num_recs, rule, bounds)
                caught[rule] += not nf.same_lists(got, want)
    print(model, caught)
    assert all(n >= 1 for n in caught.values()), caught


@pytest.mark.parametrize("model", MODELS)
def test_the_real_tile_bound_is_nan_only_over_tiles_that_hold_no_passing_score(model):
    """The pruned selection skips a tile when !(ub > thr), also when ub = (M1 + M2) + rc is NaN.  M1 and M2 ignore NaN entries, so ub is
    NaN only if M1 and M2 are opposite infinities, or rc is NaN, or rc is an infinity opposite to M1 + M2.  M = -Inf means every entry
    of the tile is -Inf or NaN in that slab, so every sum is -Inf or NaN; M = +Inf against rc = -Inf (or the other way round) makes
    every sum -Inf or NaN again.  Checked here on every (query, tile) of the construction: wherever the bound is NaN, or not above a
    score of the tile, no score of that tile is above -Inf."""
    _, queries = plan(-1.0)
    s1, s2, rc = nf.split_parts(model)
    bounds = nf.pruning_bounds(model, queries)
    n_nan = 0
    for (u, c, _, _), ub in zip(queries, bounds):
        with np.errstate(invalid="ignore"):
            v = ((s1[u] + s2[c]) if s2 is not None else s1[u]) + rc[c, u]
        assert same_bits(v.astype(np.float64), nf.scores(model)[c, u])
        for t in range(len(ub)):
            tile = v[64 * t:64 * t + 64]
            top = np.max(tile[~np.isnan(tile)], initial=-np.inf)
            if math.isnan(ub[t]):
                n_nan += 1
                assert top == -np.inf, (u, c, t)
            else:
                assert ub[t] >= top, (u, c, t)
    assert n_nan >= 1 or model == "PQ", model


# ---- SVD++ and the similarity models CAMF_ICS / CAMF_LCS / CAMF_MCS -------------------------------------------------------------------
def ext_plan(model, thold):
    train, test = nf.tuples_of(model)
    return capi.rank_plan(nf.NU, nf.N_ITEMS, train, test, thold, 0)


@pytest.mark.parametrize("model", nf.EXT_MODELS)
def test_ext_candidates_and_queries_are_the_constructions(model):
    cand, queries = ext_plan(model, -1.0)
    assert cand == nf.items()[0]
    n_ctx = nf.SIM_NCTX if model in nf.SIM_MODELS else 4
    assert {(u, c) for u, c, _, _ in queries} >= {(u, c) for u in range(13) for c in range(n_ctx)}
    if model == "SVD++":
        (tu, tj, _, _), _ = nf.tuples_of(model)
        assert len(set(zip(tu.tolist(), tj.tolist()))) == len(tu)                      # unique pairs: |N(u)| is unambiguous
        deg = [len(n) for n in nf.rated_items()]
        assert deg[nf.U_DEG0] == 0 and set(deg) == {0, 16, 64}
        assert not [q for q in queries if q[0] == nf.U_DEG0 and q[3]]                   # no training tuple: nothing excluded
        N, cand_at = nf.rated_items(), nf.items()[0]
        assert {cand_at[28], cand_at[55]} <= set(N[nf.U_Y_SAME]) and {cand_at[29], cand_at[56]} <= set(N[nf.U_Y_TWO]) and cand_at[30] in N[nf.U_Y_ONE]
    else:
        # the reference's contexts: one condition per dimension, the i-th from dimension i; one context of the ':na' conditions alone
        assert all(len(c) == nf.SIM_DIMS and all(4 * i <= x < 4 * i + 4 for i, x in enumerate(c)) for c in nf.SIM_CTX)
        assert tuple(nf.SIM_EMPTY) == nf.SIM_CTX[0] and nf.ext_state(model)["P"].shape[1] == nf.K
        assert all(np.any(nf.ext_state(model)["P"][u] == 0.0) for u in range(nf.NU))     # every P row has zeros


@pytest.mark.parametrize("model", nf.EXT_MODELS)
def test_ext_finite_entries_are_dyadic_and_the_chain_is_exact_in_fp32_and_fp64(model):
    for name, a in nf.ext_state(model).items():
        fin = a[np.isfinite(a)]
        assert np.all(fin * 8 == np.rint(fin * 8)) and np.all(np.abs(fin) <= 2.5), name
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a, equal_nan=True), name
    ref = nf.scores(model)
    assert same_bits(nf.ext_score_slab(model, np.float32, "chain").astype(np.float64), ref)
    assert (np.isfinite(ref).sum(), np.sum(ref == np.inf), np.sum(ref == -np.inf), np.isnan(ref).sum()) > (ref.size // 8, 1000, 1000, 1000)


@pytest.mark.parametrize("model", nf.SIM_MODELS)
def test_sim_contexts_carry_the_planted_scales_against_every_class_of_dot_product(model):
    chain = nf.sim_chain(model, nf.ext_state(model))
    with np.errstate(invalid="ignore"):
        scales = [float(np.prod(np.array(c))) if len(c) == 1 else float(c[0] * c[1]) for c in chain]
    assert same_bits(scales, nf.SIM_SCALES[model])
    if model != "CAMF_MCS":
        assert chain[6][0] == np.inf and chain[6][1] == 0.0 and chain[7][0] == np.inf and chain[7][1] == -np.inf
        assert chain[0] == [2.0, 0.5]                                  # the ':na' pairs are not 1 each: a skipped dimension shows
    dot = nf.scores("PQ")[0]                                           # <P_u, Q_j>, the same factors
    ref = nf.scores(model)
    _, queries = ext_plan(model, -1.0)
    for c, s in enumerate(nf.SIM_SCALES[model]):
        users = sorted({u for u, qc, _, _ in queries if qc == c})
        d = dot[users]
        fin = np.isfinite(d)
        assert np.any(d[fin] > 0) and np.any(d[fin] < 0) and np.any(d == 0.0) and np.any(d == np.inf) and np.any(d == -np.inf) and np.isnan(d).any()
        if abs(s) == np.inf:      # the reference: an infinity by the sign of the dot product, a NaN only on an exact zero (or a NaN)
            r = ref[c][users]
            assert np.array_equal(r[fin & (d != 0)], np.sign(d[fin & (d != 0)]) * s) and np.isnan(r[d == 0.0]).all()
            assert np.array_equal(r[np.isinf(d)], np.sign(d[np.isinf(d)]) * s)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("model", nf.SIM_MODELS)
def test_a_scale_folded_into_the_query_operand_would_be_told_apart(model, dtype):
    """a_q = s * P_u first, then the contraction: NaN where the reference's chain has an infinity (Inf - Inf over terms of both signs,
    0 * Inf on the zeros of P_u); bit for bit the chain on the finite contexts; and a selector fed those scores loses lists.
    (Bit for bit but for the sign of a zero: the chain's dot * s is -0 where one of the two is negative and the other an exact zero, a
    sum of products that starts from +0 is +0.  Nothing orders or thresholds the two apart, so the comparisons here and on the device
    take a zero of either sign for +0: nf.plus_zero.)"""
    ref, raw = nf.scores(model), nf.ext_score_slab(model, dtype, "operand").astype(np.float64)
    for c, s in enumerate(nf.SIM_SCALES[model]):
        if c in nf.SIM_FINITE_CTX:
            assert np.isfinite(s) and same_bits(nf.plus_zero(raw[c]), nf.plus_zero(ref[c]))
            odd = raw[c].view(np.int64) != ref[c].view(np.int64)
            assert np.all(raw[c][odd & ~np.isnan(ref[c])] == 0.0) and np.all(ref[c][odd & ~np.isnan(ref[c])] == 0.0)
        elif abs(s) == np.inf:
            spoiled = np.isnan(raw[c]) & np.isinf(ref[c])
            assert spoiled.sum() > 1000 and spoiled[nf.U_LOW].any() and spoiled[nf.U_PP].any(), (c, spoiled.sum())
            assert np.isnan(raw[c][np.isnan(ref[c])]).all()
        else:
            assert math.isnan(s) and np.isnan(ref[c]).all() and np.isnan(raw[c]).all()
    differ = 0
    for thold in (-1.0, nf.mode_threshold(model), -1e300):
        _, queries = ext_plan(model, thold)
        for num_recs in (10, 70):
            _, want = nf.oracle(model, thold, num_recs)
            assert nf.same_lists(nf.lists_by(model, queries, thold, num_recs), want)
            got = nf.lists_by(model, queries, thold, num_recs, s=raw)
            differ += not nf.same_lists(got, want)
            fin = lambda d: {k: [(j, v + 0.0) for j, v in l] for k, l in d.items() if k[1] in nf.SIM_FINITE_CTX}  # noqa: E731
            assert fin(got) == fin(want)
    assert differ == 6


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_svdpp_operand_form_is_the_chain_but_on_the_candidates_whose_q_row_is_no_number(dtype):
    """[P_u + ysum / w | 1] against [Q_j | itemBias_j]: the same NaN and infinite terms as the reference's chain wherever Q_j is finite --
    planted Y rows, biases, P rows included.  Against a Q_j[f] that is an infinity the operand has ONE term, (P_u + ysum / w)[f] * Inf,
    an infinity by the sign of the sum; the chain has P_u[f] * Inf and every Y_k[f] * Inf / w as terms of their own, a NaN as soon as two
    differ in sign or one factor is 0: there the contraction alone is not the reference, and a selector fed its scores is told apart"""
    ref, raw = nf.scores("SVD++"), nf.ext_score_slab("SVD++", dtype, "operand").astype(np.float64)
    q_bad = np.zeros(nf.NC, bool)
    q_bad[list(set(nf.A) | set(nf.B))] = True
    assert same_bits(raw[:, :, ~q_bad], ref[:, :, ~q_bad])
    assert not np.isfinite(ref[:, :, q_bad]).any() and not np.isfinite(raw[:, :, q_bad]).any()
    spoiled = np.isinf(raw) & np.isnan(ref)
    assert spoiled.sum() > 1000 and not (np.isnan(raw) & ~np.isnan(ref)).any()
    differ = 0
    for thold in (-1.0, -1e300):
        _, queries = ext_plan("SVD++", thold)
        for num_recs in (10, 70):
            differ += not nf.same_lists(nf.lists_by("SVD++", queries, thold, num_recs, s=raw), nf.oracle("SVD++", thold, num_recs)[1])
    assert differ == 4
    s = ref[0]
    assert np.isnan(s[nf.U_Y_SAME]).all()                                            # +Inf and -Inf in one factor: Inf - Inf whatever Q_j
    assert np.any(s[nf.U_Y_TWO] == np.inf) and np.any(s[nf.U_Y_TWO] == -np.inf) and np.isnan(s[nf.U_Y_TWO]).any()
    assert np.any(s[nf.U_Y_ONE] == np.inf) and np.any(s[nf.U_Y_ONE] == -np.inf) and np.isnan(s[nf.U_Y_ONE]).any()
    assert not np.any(s[nf.U_RC] > -np.inf) and np.isfinite(s[nf.U_DEG0]).any()
    assert np.all(s[nf.U_Y_ONE][list(nf.IB_PINF)] != -np.inf) and s[17, nf.IB_PINF[0]] == np.inf and s[17, nf.IB_NINF[0]] == -np.inf
    for thold in (-1.0, nf.mode_threshold("SVD++"), -1e300):
        _, queries = ext_plan("SVD++", thold)
        for num_recs in (10, 70):
            assert nf.same_lists(nf.lists_by("SVD++", queries, thold, num_recs), nf.oracle("SVD++", thold, num_recs)[1])
