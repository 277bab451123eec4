"""tests/rank_anchor.py for the four models behind ext_operands (rank_api.cpp): SVD++, CAMF_ICS, CAMF_LCS, CAMF_MCS.  Inputs and the
fp64 reference for tests/test_gpu_ext_ranking_anchor.py: ranking problems in the reference's context form, model states whose scores
are EXACT in the device's form and in the reference's, the score table of a state, and the forward error bound of a device score.
Everything here is numpy on the host; nothing imports the GPU library.

Contexts are those of the reference's data (DataDAO.java:213-214): exactly n_dims conditions per context, the i-th from dimension i
(condition ids i * cpd .. i * cpd + cpd - 1), and empty_conds[i] = dimension i's last condition plays its ':na' condition.

predict(), restated in the reference's order (score_seq; the table is the same sum vectorised in extended precision):
  CAMF_ICS (CAMF_ICS.java:53-57)   pred = rowMult(P, u, Q, j); per dimension i: pred = pred * ccMatrix[c_i][e_i]
  CAMF_LCS (CAMF_LCS.java:43-61)   the same with rowMult(cfMatrix, c_i, cfMatrix, e_i)
  CAMF_MCS (CAMF_MCS.java:53-67)   dist = sum_i (cVector[c_i] - cVector[e_i])^2; pred = rowMult(P, u, Q, j) * (1 - sqrt(dist))
  SVD++ (SVDPlusPlus.java:138-146) pred = gm + bu + bj + rowMult(P, u, Q, j); per rated item k, ascending: pred += rowMult(Y, k, Q, j) / w,
                                   w = sqrt|N(u)|
The device (ext_kernels.hip) contracts a_q = fl(s * P_u) with b_j = Q_j, s the product of the similarities formed in fp64 (or
1 - sqrt(dist)); for SVD++ a_q = [fl(P_u + ysum_u / w) | 1] with b_j = [Q_j | itemBias_j], plus the row constant fl(gm + bu).

The forward bound B = gamma_n * A, gamma_n = n u / (1 - n u), u the unit roundoff of the state's type (2^-24 / 2^-53); derived here, nothing
in it is measured.  Every rounding the device makes is counted with u, also those it makes in fp64 while the state is fp32 (that only
makes n larger than it need be).
  similarity models   A = S * sum_f |p_f q_f| with S the magnitude the scale is formed from:
                        ICS  S = prod_i |cc_i|                     n_s = d          (d - 1 products, and the first against 1)
                        LCS  S = prod_i sum_f |cf[c_i][f] cf[e_i][f]|   n_s = d (num_f + 1)   (a dot product of num_f terms per dimension, d products)
                        MCS  S = 1 + sqrt(dist)                      n_s = 2 d + 3    (per dimension a difference and a squared addend, each relative
                             to dist; sqrt halves the relative error of dist and adds its own; the subtraction from 1 adds one relative to
                             1 + sqrt(dist) -- the cancellation in 1 - sqrt(dist) is why S is not |1 - sqrt(dist)|)
                      n = k (the contraction: a dot product of k terms in any association, fused or not) + 1 (s * p_f rounded to the state's
                          type) + n_s
  SVD++               A = sum_f (|p_f| + sum_k |y_kf| / w) |q_f| + |bj| + |gm| + |bu|
                      n = (k + 1) (the contraction over [a | 1] . [q | bj]) + 1 (the row constant added) + 1 (gm + bu rounded) + 1 (a_f
                          rounded) + (deg + 2) (the deg additions of ysum, the division by w, the addition to p_f) = k + deg + 6
The reference side is computed in extended precision (np.longdouble, 2^-64 on x86: its own error is 2^-11 of an fp64 B and less of an
fp32 one) and rounded once to fp64 where the oracle needs doubles.

score_seq against oracle_c.SimOracle.predict (test_restatement_is_the_oracle_predict in tests/test_gpu_ext_ranking_anchor.py, host-only):
bit for bit on exact-grid states.  On arbitrary states both are fp64 evaluations of the same n operations, possibly associated or fused
differently: each is within n 2^-53 A of the exact value, so the two are within 2 n 2^-53 A of each other -- for CAMF_ICS at k = 17 and
three dimensions n = 21, that is 42 units of 2^-53 A; the test prints the worst difference it saw (0: the C oracle keeps the order)."""
import math
from types import SimpleNamespace

import numpy as np

from oracle import rank_oracle
from tests import rank_anchor as ra

SIM_MODELS = ("CAMF_ICS", "CAMF_LCS", "CAMF_MCS")
MODELS = ("SVD++",) + SIM_MODELS
U64 = 2.0 ** -53
R_POS, R_NEG = ra.R_POS, ra.R_NEG
LD = np.longdouble


# ---- problems ---------------------------------------------------------------------------------------------------------------
def _contexts(model, rng, n_dims, cpd, n_ctx):
    """context 0 = the ':na' conditions alone; contexts 1..3 are empty in some dimensions only; CAMF_MCS (exact_state) needs at most two
    dimensions that differ from their partner, one even and one odd (a (3, 4, 5) / 8 pair)"""
    empty = [i * cpd + cpd - 1 for i in range(n_dims)]
    ctxs = [list(empty)]
    while len(ctxs) < n_ctx:
        c = [i * cpd + int(rng.integers(cpd)) for i in range(n_dims)]
        if len(ctxs) <= 3 and n_dims > 1:
            c[len(ctxs) % n_dims] = empty[len(ctxs) % n_dims]
            c[(len(ctxs) + 1) % n_dims] = ((len(ctxs) + 1) % n_dims) * cpd                       # ... and not empty in another
        if model == "CAMF_MCS":
            keep = {int(rng.integers(0, n_dims, 1)[0])} if n_dims == 1 or rng.random() < 0.4 else \
                {2 * int(rng.integers((n_dims + 1) // 2)), 2 * int(rng.integers(n_dims // 2)) + 1}
            c = [x if i in keep else empty[i] for i, x in enumerate(c)]
        ctxs.append(c)
    return empty, ctxs


def make_problem(model, nc, n_users, n_dims, cpd, seed, n_ctx=12, degrees=(0, 1, 4, 16)):
    """rank_anchor.make_problem in the reference's context form: exactly `nc` candidates with sparse ids (the HashSet order is not
    ascending), users with queries in one or two contexts, every 7th user with a long exclusion list in its first query's context, correct
    items that are no candidates, one (user, context) that is no query.  SVD++: the training set holds unique (user, item) pairs, every
    user's degree is drawn from `degrees` (user 4: none at all), the long lists are as long as the degree allows."""
    rng = np.random.default_rng(seed)
    id_space = 3 * nc + 500
    ids = rng.choice(id_space, size=nc + 8, replace=False).astype(np.int64)
    items, strangers = ids[:nc], ids[nc:]
    empty, ctxs = _contexts(model, rng, n_dims, cpd, n_ctx)
    ctx_ptr = np.arange(0, n_dims * n_ctx + 1, n_dims, dtype=np.int32)
    ctx_conds = np.array([x for c in ctxs for x in c], np.int32)
    q_ctx = {}
    for u in range(n_users):
        q_ctx[u] = [int(c) for c in rng.choice(n_ctx, size=1 + int(rng.integers(2)), replace=False)]
        if u < 3:
            q_ctx[u][0] = u
            q_ctx[u] = list(dict.fromkeys(q_ctx[u]))
    tr = []
    if model == "SVD++":
        deg = [int(d) for d in rng.choice([d for d in degrees if d <= nc], size=n_users)]
        deg[0], deg[3], deg[4] = max(d for d in degrees if d <= nc), max(d for d in degrees if d <= nc), 0
        slots = [u for u in range(n_users) for _ in range(deg[u])]
        assert len(slots) >= nc
        slots = [slots[i] for i in rng.permutation(len(slots))]
        have = {u: set() for u in range(n_users)}
        for u, j in zip(slots[:nc], rng.permutation(items)):                       # every candidate once
            have[u].add(int(j))
        for u in slots[nc:]:
            have[u].add(int(rng.choice([j for j in items if int(j) not in have[u]])))
        for u in range(n_users):
            assert len(have[u]) == deg[u]
            for j in sorted(have[u]):
                tr.append((u, j, q_ctx[u][0] if u % 7 == 3 else int(rng.integers(n_ctx)), float(rng.integers(1, 6))))
        tr = [tr[i] for i in rng.permutation(len(tr))]
    else:
        for j in rng.permutation(items):
            tr.append((int(rng.integers(n_users)), int(j), int(rng.integers(n_ctx)), float(rng.integers(1, 6))))
        for _ in range(2 * n_users):
            tr.append((int(rng.integers(n_users)), int(items[int(rng.integers(min(nc, 40)))]), int(rng.integers(n_ctx)), float(rng.integers(1, 6))))
        for u in range(3, n_users, 7):
            for j in rng.choice(items, size=min(nc // 2, int(rng.integers(20, 41))), replace=False):
                tr.append((u, int(j), q_ctx[u][0], float(rng.integers(1, 6))))
    seen, train = set(), []
    for t in tr:
        if t[:3] not in seen:
            seen.add(t[:3])
            train.append(t)
    te = []
    for u in range(n_users):
        for c in q_ctx[u]:
            for j in rng.choice(items, size=1 + int(rng.integers(3)), replace=False):
                te.append((u, int(j), c, R_POS))
            if u % 5 == 1:
                te.append((u, int(strangers[u % len(strangers)]), c, R_POS))
            te.append((u, int(items[int(rng.integers(nc))]), c, R_NEG))
    lone_c = next(c for c in range(n_ctx) if c not in q_ctx[n_users - 1])
    te.append((n_users - 1, int(strangers[0]), lone_c, R_POS))
    cand = rank_oracle.java_int_hashset_order([t[1] for t in train])
    assert len(cand) == nc and cand != sorted(cand)
    pos = {j: i for i, j in enumerate(cand)}
    queries = list(dict.fromkeys((t[0], t[2]) for t in te if t[3] == R_POS and t[1] in pos))
    rated = [sorted({t[1] for t in train if t[0] == u}) for u in range(n_users)]     # N(u): fixed here, before add_short_query
    if model == "SVD++":
        assert len({t[:2] for t in train}) == len(train) and not rated[4] and any(q[0] == 4 for q in queries)
    return SimpleNamespace(model=model, n_users=n_users, n_items=id_space, n_conds=n_dims * cpd, n_dims=n_dims, cpd=cpd, n_ctx=n_ctx, ctxs=ctxs,
                           empty=np.array(empty, np.int32), ctx_ptr=ctx_ptr, ctx_conds=ctx_conds, train=train, model_train=list(train), test=te,
                           cand=cand, pos=pos, queries=queries, rated=rated)


# ---- states -----------------------------------------------------------------------------------------------------------------
def _lcs_support(num_f):
    return sorted({0, num_f // 2, num_f - 1})


def exact_state(model, prob, k, dist, seed, num_f=0):
    """An fp32 state on a grid where the device's form AND the reference's are exact (check_exact_premise is the gate).  P and Q as
    rank_anchor.exact_state has them: multiples of 2^-3 with |x| <= 4 (spread) or sparse from {-1/2, 0, 1/2} (tied).
      CAMF_ICS  similarities from {-1, -1/2, 1/2, 1, 2}, ccMatrix symmetric; the ':na' conditions' own entries are not 1
      CAMF_LCS  cfMatrix rows are +-1/2 on the columns {0, num_f / 2, num_f - 1} and 0 elsewhere: a pair's similarity is an odd multiple of 1/4
                of magnitude <= 3/4 (never 0), a product over three dimensions has at most 5 significant bits
      CAMF_MCS  the ':na' positions are multiples of 1/8, a condition of an even dimension lies 3/8 from its partner, of an odd one 4/8: one
                differing dimension gives sqrt(dist) = 3/8 or 4/8, an even and an odd one 5/8
      SVD++     Y multiples of 2^-3 with |y| <= 1 (tied: sparse from {-1/2, 0, 1/2}), biases and the mean multiples of 2^-6 as in the MF family;
                the degrees are 0, 1, 4, 16 or 64, so w is a power of two"""
    rng = np.random.default_rng(seed)
    grid = lambda shape: rng.integers(-32, 33, shape) / 8.0  # noqa: E731
    sparse = lambda shape, p: np.where(rng.random(shape) < p, rng.choice([-0.5, 0.5], size=shape), 0.0)  # noqa: E731
    pk = min(1.0, 1.0 / math.sqrt(k))
    st = {"P": grid((prob.n_users, k)) if dist == "spread" else sparse((prob.n_users, k), pk),
          "Q": grid((prob.n_items, k)) if dist == "spread" else sparse((prob.n_items, k), pk)}
    gm = 0.0
    n = prob.n_conds
    if model == "SVD++":
        if dist == "spread":
            st["userBias"], st["itemBias"] = rng.integers(-256, 257, prob.n_users) / 64.0, rng.integers(-256, 257, prob.n_items) / 64.0
            st["Y"], gm = rng.integers(-8, 9, (prob.n_items, k)) / 8.0, 3.015625
        else:
            st["userBias"], st["itemBias"] = sparse((prob.n_users,), 0.5), sparse((prob.n_items,), 0.5)
            st["Y"], gm = sparse((prob.n_items, k), pk / 4), 3.0
    elif model == "CAMF_ICS":
        c = rng.choice([-1.0, -0.5, 0.5, 1.0, 2.0], size=(n, n))
        st["ccMatrix"] = np.triu(c) + np.triu(c, 1).T
    elif model == "CAMF_LCS":
        st["cfMatrix"] = np.zeros((n, num_f))
        st["cfMatrix"][:, _lcs_support(num_f)] = rng.choice([-0.5, 0.5], size=(n, len(_lcs_support(num_f))))
    else:
        cv = np.zeros(n)
        for i in range(prob.n_dims):
            e = int(prob.empty[i])
            cv[e] = int(rng.integers(0, 5)) / 8.0
            for x in range(i * prob.cpd, e):
                cv[x] = cv[e] + float(rng.choice([-1.0, 1.0])) * (3 if i % 2 == 0 else 4) / 8.0
        st["cVector"] = cv
    return {name: a.astype(np.float32) for name, a in st.items()}, gm


def loud_state(model, prob, k, seed, num_f=0):
    """the draws of tests/eval_anchor.loud_state at this problem's shapes, fp64: SVD++ factors N(0, 0.3), Y N(0, 0.1), biases at their own
    scales (gm = 3 puts the scores on the rating scale); the similarity models have no mean, theirs are positive and sized so that the dot
    product lands on the 0.5 .. 5 scale, every user's row scaled from 0.05 to 1.95 of that"""
    rng = np.random.default_rng(seed)
    if model == "SVD++":
        return {"P": 0.3 * rng.standard_normal((prob.n_users, k)), "Q": 0.3 * rng.standard_normal((prob.n_items, k)),
                "userBias": 0.5 * rng.standard_normal(prob.n_users), "itemBias": 0.3 * rng.standard_normal(prob.n_items),
                "Y": 0.1 * rng.standard_normal((prob.n_items, k))}, 3.0
    a = math.sqrt(4.0 * (0.5 + 0.6 * 4.5) / k)
    st = {"P": a * rng.random((prob.n_users, k)) * np.linspace(0.05, 1.95, prob.n_users)[:, None], "Q": a * rng.random((prob.n_items, k))}
    if model == "CAMF_ICS":
        c = 1.0 + 0.1 * rng.standard_normal((prob.n_conds, prob.n_conds))
        st["ccMatrix"] = (c + c.T) / 2
    elif model == "CAMF_LCS":
        st["cfMatrix"] = (0.8 + 0.4 * rng.random((prob.n_conds, num_f))) / math.sqrt(num_f)
    else:
        st["cVector"] = (0.2 + 0.6 * rng.random(prob.n_conds)) / math.sqrt(prob.n_dims)
    return st, 0.0


# ---- the reference ----------------------------------------------------------------------------------------------------------
def score_seq(model, st, gm, prob, u, j, c):
    """predict(u, j, c) in fp64, every operation in the reference's order (module docstring)"""
    f64 = lambda x: np.asarray(x, np.float64).tolist()  # noqa: E731
    qj = f64(st["Q"][j])

    def row_mult(a, b):
        s = 0.0
        for x, y in zip(a, b):
            s += x * y
        return s
    if model == "SVD++":
        pred = gm + float(st["userBias"][u]) + float(st["itemBias"][j]) + row_mult(f64(st["P"][u]), qj)
        w = math.sqrt(len(prob.rated[u]))
        for k in prob.rated[u]:
            pred += row_mult(f64(st["Y"][k]), qj) / w
        return pred
    pred = row_mult(f64(st["P"][u]), qj)
    dist = 0.0
    for c1, c2 in zip(prob.ctxs[c], prob.empty.tolist()):
        if model == "CAMF_ICS":
            pred = pred * float(st["ccMatrix"][c1][c2])
        elif model == "CAMF_LCS":
            pred = pred * row_mult(f64(st["cfMatrix"][c1]), f64(st["cfMatrix"][c2]))
        else:
            d = float(st["cVector"][c1]) - float(st["cVector"][c2])
            dist += d * d
    return pred * (1.0 - math.sqrt(dist)) if model == "CAMF_MCS" else pred


def context_scales(model, st, prob):
    """per context (chain, S): the factors the reference multiplies by, in its order, in extended precision, and the magnitude S of the
    bound (module docstring)"""
    out = []
    for ctx in prob.ctxs:
        chain, mag, dist = [], LD(1.0), LD(0.0)
        for c1, c2 in zip(ctx, prob.empty.tolist()):
            if model == "CAMF_ICS":
                s = LD(st["ccMatrix"][c1][c2])
                chain.append(s)
                mag = mag * abs(s)
            elif model == "CAMF_LCS":
                a, b = st["cfMatrix"][c1].astype(LD), st["cfMatrix"][c2].astype(LD)
                s = LD(0.0)
                for x in (a * b).tolist():
                    s = s + LD(x)
                chain.append(s)
                mag = mag * np.abs(a * b).sum()
            else:
                d = LD(st["cVector"][c1]) - LD(st["cVector"][c2])
                dist = dist + d * d
        if model == "CAMF_MCS":
            chain, mag = [LD(1.0) - np.sqrt(dist)], LD(1.0) + np.sqrt(dist)
        out.append((chain, mag))
    return out


def _dots(A, Qc, absolute):
    """sum_f A[q][f] Qc[i][f], ascending f, in extended precision"""
    A, Qc = A.astype(LD), Qc.astype(LD)
    if absolute:
        A, Qc = np.abs(A), np.abs(Qc)
    s = np.zeros((A.shape[0], Qc.shape[0]), LD)
    for f in range(A.shape[1]):
        s = s + A[:, f][:, None] * Qc[:, f][None, :]
    return s


def score_table(model, st, gm, prob, queries, absolute=False):
    """F[q][i] = predict(user, candidate i, context) of query q from the state `st`, in extended precision (np.longdouble), candidates in
    the reference's HashSet order.  absolute=True: the factor A of the forward bound (module docstring)"""
    cand = np.array(prob.cand)
    qu = np.array([q[0] for q in queries])
    Qc = st["Q"][cand]
    if model == "SVD++":
        bu, bj = st["userBias"].astype(LD)[qu][:, None], st["itemBias"].astype(LD)[cand][None, :]
        if absolute:
            F = (abs(LD(gm)) + np.abs(bu)) + np.abs(bj) + _dots(st["P"][qu], Qc, True)
        else:
            F = ((LD(gm) + bu) + bj) + _dots(st["P"][qu], Qc, False)
        rows = {}
        for u in sorted(set(qu.tolist())):
            if prob.rated[u]:
                rows[u] = _dots(st["Y"][prob.rated[u]], Qc, absolute) / LD(math.sqrt(len(prob.rated[u])))
        for i, u in enumerate(qu.tolist()):
            if u in rows:
                for r in rows[u]:                                  # per rated item, ascending, as the reference adds them
                    F[i] = F[i] + r
        return F
    F = _dots(st["P"][qu], Qc, absolute)
    scales = context_scales(model, st, prob)
    for i, (_, c) in enumerate(queries):
        chain, mag = scales[c]
        if absolute:
            F[i] = F[i] * mag
        else:
            for s in chain:
                F[i] = F[i] * s
    return F


def n_roundings(model, prob, k, queries, num_f=0):
    """n of gamma_n per query (module docstring)"""
    d = prob.n_dims
    if model == "SVD++":
        return np.array([k + len(prob.rated[u]) + 6 for u, _ in queries], np.float64)
    n_s = {"CAMF_ICS": d, "CAMF_LCS": d * (num_f + 1), "CAMF_MCS": 2 * d + 3}[model]
    return np.full(len(queries), k + 1 + n_s, np.float64)


def error_bound(model, st, gm, prob, queries, k, u, num_f=0):
    A = score_table(model, st, gm, prob, queries, absolute=True).astype(np.float64)
    n = n_roundings(model, prob, k, queries, num_f)
    return A * (n * u / (1.0 - n * u))[:, None]


# ---- premises ---------------------------------------------------------------------------------------------------------------
def device_terms(model, st, gm, prob, u, j, c):
    """the terms of the device's form of predict(u, j, c) as fp64 numbers computed from the fp32 state, and the operand entries whose
    rounding to fp32 must be exact: k products fl(s p_f) q_f; SVD++: k products fl(p_f + ysum_f / w) q_f, then itemBias and gm + userBias"""
    P, q = np.asarray(st["P"][u], np.float64), np.asarray(st["Q"][j], np.float64)
    if model == "SVD++":
        a = P.copy()
        if prob.rated[u]:
            a = a + np.asarray(st["Y"][prob.rated[u]], np.float64).sum(axis=0) / math.sqrt(len(prob.rated[u]))
        return (a * q).tolist() + [float(st["itemBias"][j]), gm + float(st["userBias"][u])], a
    s = 1.0
    for x in context_scales(model, st, prob)[c][0]:
        s = s * float(x)
    return (P * s * q).tolist(), P * s


def check_exact_premise(model, st, gm, prob, F, queries, seed, n_sample=48):
    """Layer 1's premise, proven on the host: for a sample of (query, candidate) pairs the reference's chain in fp64 (score_seq) equals
    the table; the device's operand entries are fp32 numbers; every term of the device's form is an fp32 number; and the fp32 sum of
    those terms -- accumulated term by term in forward, reverse and two shuffled orders -- equals the table's score."""
    for name, a in st.items():
        assert a.dtype == np.float32 and np.all(np.abs(a) <= 4.0), name
        unit = 8.0 if name in ("P", "Q", "Y", "cVector", "cfMatrix", "ccMatrix") else 64.0
        assert np.all(a.astype(np.float64) * unit == np.rint(a.astype(np.float64) * unit)), name
    rng = np.random.default_rng(seed)
    for _ in range(n_sample):
        qi, ci = int(rng.integers(len(queries))), int(rng.integers(len(prob.cand)))
        (u, c), j = queries[qi], prob.cand[ci]
        exact = float(F[qi, ci])
        assert LD(exact) == F[qi, ci] and score_seq(model, st, gm, prob, u, j, c) == exact, (qi, ci)
        terms, operand = device_terms(model, st, gm, prob, u, j, c)
        terms = np.array(terms, np.float64)
        t32 = terms.astype(np.float32)
        assert np.array_equal(operand.astype(np.float32).astype(np.float64), operand)
        assert np.array_equal(t32.astype(np.float64), terms)
        assert math.fsum(terms.tolist()) == exact, (qi, ci)
        for order in (np.arange(len(t32)), np.arange(len(t32))[::-1], rng.permutation(len(t32)), rng.permutation(len(t32))):
            s = np.add.accumulate(t32[order], dtype=np.float32)[-1]
            assert float(s) == exact, (qi, ci, float(s), exact)
