"""The reference side of tests/test_gpu_fm_eval_anchor.py, on the host alone (tests/fm_anchor.py): the restatement of FM.predict against
the C oracle, the extended-precision table against the restatement, and the premises the device tests rest on -- each shown on the
reference before any device is asked.  A premise says that a particular WRONG evaluation moves the scores by more than 4 B (B the
forward bound of a device score) or, on the exact grid, moves them at all: the device tests, which hold every score within B (or
bit for bit), then fail for a kernel that evaluates that way."""
import math

import numpy as np
import pytest

from oracle import oracle_c
from tests import fm_anchor as fa


def _oracle(m):
    z = np.zeros(1, np.int32)
    return oracle_c.FMOracle(m.k, m.n_users, m.n_items, m.n_conds, m.n_dims, z, z, z, np.ones(1), m.w0, m.w, m.V, 0.1, 0.1)


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("n_dims", [1, 2, 3])
@pytest.mark.parametrize("kind", ["real", "loud", "grid"])
def test_restatement_is_the_oracle_predict_bit_for_bit(kind, n_dims):
    """predict_seq (the dense walk) == oracle_c.FMOracle.predict (the active rows, in the same order) == seq_table on finite models, with
    contexts n_conds - 1, n_conds, FAR and below"""
    m, tuples = fa.predict_case(kind, 17, n_dims if kind != "grid" else (1, 2, 4)[n_dims - 1])
    orc = _oracle(m)
    u, j, c = tuples[257]
    assert {m.n_conds - 1, m.n_conds, fa.FAR} <= set(c.tolist()) and (c < m.n_conds).sum() > 50 and (c >= m.n_conds).sum() > 50
    F = fa._eval(m, u, j, c, np.float64)
    for t in range(len(u)):
        a = fa.predict_seq(m, int(u[t]), int(j[t]), int(c[t]))
        assert a == orc.predict(int(u[t]), int(j[t]), int(c[t])) == F[t], t


@pytest.mark.parametrize("case", fa.NF_CASES, ids=fa.nf_id)
def test_restatement_is_the_oracle_predict_on_non_finite_models(case):
    """the oracle follows FM.java:97-98, 103-105 too: one entry of w or V that is no number makes NaN of every prediction that does not
    hold its coordinate (and, in V, of those that do)"""
    prob, m = fa.nonfinite_case(case)
    orc = _oracle(m)
    T = fa.nonfinite_table(m, prob)
    for qi in range(0, len(prob.queries), 3):
        u, c = prob.queries[qi]
        for ci in (0, 5, 6, len(prob.cand) - 1):
            assert _same(orc.predict(u, prob.cand[ci], c), float(T[qi, ci])), (qi, ci)
    field, coord, touched, value = case
    if field == "w0":
        assert np.array_equal(T, np.full(T.shape, value), equal_nan=True)
    elif not touched or field == "V":
        assert np.isnan(T).all()
    else:                                       # a weight of a coordinate some tuples hold: theirs is the infinity, every other is NaN
        own = np.zeros(T.shape, bool)
        if coord == "user":
            own[prob.q_users == 0, :] = True
        elif coord == "item":
            own[:, 5] = True
        else:
            own[prob.q_ctx == fa.N_CONDS - 1, :] = True
        assert own.any() and not own.all() and np.isnan(T[~own]).all()
        assert np.array_equal(T[own], np.full(int(own.sum()), value), equal_nan=True)


@pytest.mark.parametrize("kind", ["real", "loud"])
def test_extended_precision_table_is_within_the_bound_of_the_restatement(kind):
    worst = 0.0
    for k in (1, 17, 130):
        for n_dims in (1, 3):
            m, tuples = fa.predict_case(kind, k, n_dims)
            u, j, c = tuples[257]
            Fx, B = fa.tuple_scores(m, u, j, c)
            for t in range(len(u)):
                err = abs(fa.LD(fa.predict_seq(m, int(u[t]), int(j[t]), int(c[t]))) - Fx[t])
                assert err <= B[t], (k, n_dims, t, float(err), B[t])
                assert fa.bound(m, int(u[t]), int(j[t]), int(c[t])) == B[t]
                worst = max(worst, float(err) / B[t])
    print("%s: worst |predict_seq - table| / B = %.4f" % (kind, worst))


def _wrong_tables(m, users, items, ctx, seed):
    """name -> (the table of a wrong evaluation, the entries it must move)"""
    has = np.broadcast_to((np.asarray(ctx) < m.n_conds)[:, None], (len(users), len(items)))
    every = np.ones(has.shape, bool)
    wrong = {"w_j left out": (fa.score_table(m, users, items, ctx, drop_wj=True), every),
             "context term dropped": (fa.score_table(m, users, items, ctx, drop_ctx=True), has),
             "c == n_conds holds a feature": (fa.score_table(fa.with_one_more_condition(m, seed), users, items, ctx),
                                              np.broadcast_to((np.asarray(ctx) == m.n_conds)[:, None], has.shape))}
    if m.n_dims > 1:
        wrong["xc taken as 1"] = (fa.score_table(m, users, items, ctx, xc=1.0), has)
    if m.k > 64:
        wrong["factors >= 64 dropped"] = (fa.score_table(m, users, items, ctx, k_cut=64), every)
    return wrong


@pytest.mark.parametrize("nc", fa.TOPN_NC)
@pytest.mark.parametrize("k", fa.TOPN_K)
@pytest.mark.parametrize("kind", fa.KINDS)
def test_top_n_premises(kind, k, nc):
    """On the reference alone, for every top-N case of the device tests: the wrong evaluations move every score they touch by more than
    4 B (grid: they move scores in most of the queries they touch); every gap among a query's first num_recs + 1 reference candidates exceeds
    4 B, in EVERY query, planted ties excepted; no eligible score lies within 4 B of the threshold; the planted pairs tie exactly."""
    prob, m, pairs = fa.topn_case(kind, k, nc)
    users, items, ctx = prob.q_users, prob.items, prob.q_ctx
    assert len(prob.queries) > 64 and len(prob.cand) == nc and {m.n_conds - 1, m.n_conds, fa.FAR} <= set(ctx.tolist())
    F = fa.check_grid(m, users, items, ctx, fa.seed_of("grid", kind, k, nc)) if kind == "grid" else fa.score_table(m, users, items, ctx)
    for a, b in pairs:
        assert a < b and np.array_equal(F[:, a], F[:, b])
    B = fa.bound_table(m, users, items, ctx)
    for name, (W, where) in _wrong_tables(m, users, items, ctx, fa.seed_of("one more", kind, k, nc)).items():
        assert where.any(axis=1).sum() >= 3, name
        if kind == "grid":
            assert np.mean((W != F)[where.any(axis=1)].any(axis=1)) > 0.5, name   # (a grid entry may be 0: a factor can drop out of a row)
        else:
            assert np.all(np.abs(W - F)[where] > 4.0 * B[where]), (name, float((np.abs(W - F) / B)[where].min()))
        assert np.array_equal(W[~where], F[~where]), name
    if kind != "grid":
        E = fa.eligible(prob)
        assert np.all(np.abs(F - fa.THOLD)[E] > 4.0 * B[E])
        for num_recs in fa.NUM_RECS:
            r = fa.min_gap_ratio(F, B, E, pairs, num_recs)
            assert len(r) == len(prob.queries) and np.all(r > 1.0), (num_recs, float(r.min()))


@pytest.mark.parametrize("k", fa.PREDICT_K)
@pytest.mark.parametrize("kind", fa.KINDS)
def test_predict_premises(kind, k):
    """the same wrong evaluations on the tuples of the predict cases (257 tuples, every dims)"""
    for n_dims in fa.PREDICT_DIMS[kind]:
        m, tuples = fa.predict_case(kind, k, n_dims)
        u, j, c = tuples[257]
        has = c < m.n_conds
        F = fa._eval(m, u, j, c, fa.LD).astype(np.float64)
        if kind == "grid":
            assert np.array_equal(F, fa._eval(m, u, j, c, np.float64))
            assert all(fa.predict_seq(m, int(u[t]), int(j[t]), int(c[t])) == F[t] for t in range(0, 257, 16))
        B = fa.tuple_scores(m, u, j, c)[1]
        wrong = {"w_j left out": (dict(drop_wj=True), np.ones(257, bool)), "context term dropped": (dict(drop_ctx=True), has)}
        if n_dims > 1:
            wrong["xc taken as 1"] = (dict(xc=1.0), has)
        if k > 64:
            wrong["factors >= 64 dropped"] = (dict(k_cut=64), np.ones(257, bool))
        for name, (kw, where) in wrong.items():
            W = fa._eval(m, u, j, c, fa.LD, **kw).astype(np.float64)
            if kind == "grid":
                assert (W != F)[where].mean() > 0.5, name
            else:
                assert np.all(np.abs(W - F)[where] > 4.0 * B[where]), (name, n_dims)
        W = fa._eval(fa.with_one_more_condition(m, 1), u, j, c, fa.LD).astype(np.float64)
        at = c == m.n_conds
        assert at.sum() >= 1 and np.all(W[at] != F[at]) and np.array_equal(W[~at], F[~at])
