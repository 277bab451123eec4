"""Inputs and the fp64 reference for tests/test_gpu_ranking_f32_anchor.py: ranking problems with the edges the fp32 evalRankings
kernels have (candidate counts around the 64 / 128 tiles, sparse item ids, empty and long contexts, long exclusion lists, a query
with a short list), model states whose fp32 scores are EXACT, the fp64 score table of a state, and the forward error bound of an
fp32 score.  Everything here is numpy on the host: the premises of the GPU tests (exact sums; enough unambiguous queries) are
checked by plain functions that need no device."""
import math
import os
from types import SimpleNamespace

import numpy as np

from oracle import rank_oracle

TWO_D = ("BiasedMF", "PMF")
U32 = 2.0 ** -24                      # unit roundoff of fp32
R_POS, R_NEG = 5.0, -7.0              # test ratings: a positive is `r > bin_thold`; every threshold used here lies in (-7, 5)


def with_env(env, fn):
    """fn() with the environment variables of `env` set (None = unset), restored afterwards."""
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---- problems ---------------------------------------------------------------------------------------------------------------

def make_problem(model, nc, n_users, n_conds, seed, n_ctx=12):
    """A ranking problem with exactly `nc` candidates (= distinct training items) whose ids are sparse in a larger id space, so the
    candidates' HashSet order is not ascending.  Context 0 has no condition, context 1 one, context 2 the first and the last
    condition id, the others 1..6.  Every user has a query in one or two contexts; every 7th user rated 20..40 items in the context of
    its first query (a long exclusion list).  Some queries also name a correct item that is no candidate; one (user, context) names only
    such items and is therefore no query."""
    rng = np.random.default_rng(seed)
    id_space = 3 * nc + 500
    ids = rng.choice(id_space, size=nc + 8, replace=False).astype(np.int64)
    items, strangers = ids[:nc], ids[nc:]
    ctxs = [[], [int(rng.integers(n_conds))], sorted({0, n_conds - 1})]
    while len(ctxs) < n_ctx:
        d = int(rng.integers(1, min(n_conds, 6) + 1))
        ctxs.append(sorted(rng.choice(n_conds, size=d, replace=False).tolist()))
    ctx_ptr = np.zeros(n_ctx + 1, np.int32)
    ctx_ptr[1:] = np.cumsum([len(c) for c in ctxs])
    ctx_conds = np.array([x for c in ctxs for x in c], np.int32)

    tr = []                                                             # (u, j, c, r)
    for j in rng.permutation(items):                                    # every candidate once: the first-seen order is random
        tr.append((int(rng.integers(n_users)), int(j), int(rng.integers(n_ctx)), float(rng.integers(1, 6))))
    for _ in range(2 * n_users):                                        # uneven training degrees (num_ignore drops the most popular)
        tr.append((int(rng.integers(n_users)), int(items[int(rng.integers(min(nc, 40)))]), int(rng.integers(n_ctx)), float(rng.integers(1, 6))))
    q_ctx = {}
    for u in range(n_users):
        n = 1 + int(rng.integers(2))
        q_ctx[u] = [int(c) for c in rng.choice(n_ctx, size=n, replace=False)]
        if u < 3:
            q_ctx[u][0] = u                                             # contexts 0 (no condition), 1 and 2 are certainly queried
            q_ctx[u] = list(dict.fromkeys(q_ctx[u]))
        if u % 7 == 3:
            h = min(nc // 2, int(rng.integers(20, 41)))
            for j in rng.choice(items, size=h, replace=False):
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
    te.append((n_users - 1, int(strangers[0]), lone_c, R_POS))          # only a non-candidate is correct: not a query
    cand = rank_oracle.java_int_hashset_order([t[1] for t in train])
    assert len(cand) == nc and cand != sorted(cand)
    pos = {j: i for i, j in enumerate(cand)}
    queries = list(dict.fromkeys((t[0], t[2]) for t in te if t[3] == R_POS and t[1] in pos))    # the order is of no consequence
    return SimpleNamespace(model=model, n_users=n_users, n_items=id_space, n_conds=n_conds, n_ctx=n_ctx, ctxs=ctxs, ctx_ptr=ctx_ptr,
                           ctx_conds=ctx_conds, train=train, test=te, cand=cand, pos=pos, queries=queries)


def arrays(tuples):
    u, j, c, r = zip(*tuples)
    return np.array(u, np.int32), np.array(j, np.int32), np.array(c, np.int32), np.array(r, np.float64)


def excluded_columns(prob):
    """{(user, context): ascending candidate positions of the items the user rated in that context in the training set}"""
    out = {}
    for (u, j, c, _) in prob.train:
        out.setdefault((u, c), set()).add(prob.pos[j])
    return {q: sorted(s) for q, s in out.items()}


# ---- states -----------------------------------------------------------------------------------------------------------------

def _shapes(model, prob, k):
    s = {"P": (prob.n_users, k), "Q": (prob.n_items, k)}
    if model in ("BiasedMF", "CAMF_C", "CAMF_CI"):
        s["userBias"] = (prob.n_users,)
    if model in ("BiasedMF", "CAMF_C", "CAMF_CU"):
        s["itemBias"] = (prob.n_items,)
    if model == "CAMF_C":
        s["condBias"] = (prob.n_conds,)
    if model in ("CAMF_CU", "CAMF_CUCI"):
        s["ucBias"] = (prob.n_users, prob.n_conds)
    if model in ("CAMF_CI", "CAMF_CUCI"):
        s["icBias"] = (prob.n_items, prob.n_conds)
    return s


def exact_state(model, prob, k, dist, seed):
    """An fp32 state on the exact grid: factors multiples of 2^-3 with |x| <= 4, biases and the global mean multiples of 2^-6 with
    |x| <= 4.  A product is then a multiple of 2^-6 of magnitude <= 16, and a sum of k <= 256 products and <= 34 bias terms stays below
    2^13 at granularity 2^-6 -- 19 significant bits: every fp32 partial sum is exact in any association.
      spread: dense over the whole grid (many distinct scores);
      tied:   sparse factors from {-1/2, 0, 1/2}, biases from {-1/2, 0, 1/2} (a handful of distinct scores, thousands of exact ties)."""
    rng = np.random.default_rng(seed)
    st = {}
    for name, shape in _shapes(model, prob, k).items():
        factor = name in ("P", "Q")
        if dist == "spread":
            a = rng.integers(-32, 33, shape) / 8.0 if factor else rng.integers(-256, 257, shape) / 64.0
        else:
            p = min(1.0, 1.0 / math.sqrt(k)) if factor else 0.5
            a = np.where(rng.random(shape) < p, rng.choice([-0.5, 0.5], size=shape), 0.0)
        st[name] = a.astype(np.float32)
    gm = 0.0 if model == "PMF" else (3.015625 if dist == "spread" else 3.0)
    return st, gm


# ---- the fp64 reference -------------------------------------------------------------------------------------------------------

def score_terms(model, st, gm, prob, u, j, c):
    """The terms of predict(u, j, c) as fp64 numbers, from the fp32 state: k products, then the bias / constant terms."""
    f64 = lambda x: np.asarray(x, np.float64)
    terms = (f64(st["P"][u]) * f64(st["Q"][j])).tolist()
    conds = prob.ctxs[c] if model not in TWO_D else []
    if model != "PMF":
        terms.append(float(gm))
    if model in ("BiasedMF", "CAMF_C", "CAMF_CI"):
        terms.append(float(st["userBias"][u]))
    if model in ("BiasedMF", "CAMF_C", "CAMF_CU"):
        terms.append(float(st["itemBias"][j]))
    for cond in conds:
        if model == "CAMF_C":
            terms.append(float(st["condBias"][cond]))
        if model in ("CAMF_CI", "CAMF_CUCI"):
            terms.append(float(st["icBias"][j][cond]))
        if model in ("CAMF_CU", "CAMF_CUCI"):
            terms.append(float(st["ucBias"][u][cond]))
    return terms


def n_bias_terms(model, prob, c):
    """How many bias / constant terms predict() adds to the k products for a query in context c."""
    d = len(prob.ctxs[c]) if model not in TWO_D else 0
    return {"PMF": 0, "BiasedMF": 3, "CAMF_C": 3 + d, "CAMF_CI": 2 + d, "CAMF_CU": 2 + d, "CAMF_CUCI": 1 + 2 * d}[model]


def score_table(model, st, gm, prob, queries, absolute=False):
    """F[q][i] = predict(user, candidate i, context) of query q in fp64 from the fp32 state `st` (candidates in the reference's
    HashSet order).  absolute=True: the same sum over the terms' magnitudes (the factor of the forward error bound)."""
    f = (lambda x: np.abs(np.asarray(x, np.float64))) if absolute else (lambda x: np.asarray(x, np.float64))
    cand = np.array(prob.cand)
    qu = np.array([q[0] for q in queries])
    F = f(st["P"])[qu] @ f(st["Q"])[cand].T
    if model != "PMF":
        F += abs(gm) if absolute else gm
    if "userBias" in st:
        F += f(st["userBias"])[qu][:, None]
    if "itemBias" in st:
        F += f(st["itemBias"])[cand][None, :]
    if model not in TWO_D:
        for i, (u, c) in enumerate(queries):
            for cond in prob.ctxs[c]:
                if model == "CAMF_C":
                    F[i] += f(st["condBias"][cond])
                if "icBias" in st:
                    F[i] += f(st["icBias"])[cand, cond]
                if "ucBias" in st:
                    F[i] += f(st["ucBias"][u][cond])
    return F


def error_bound(model, st, gm, prob, queries, k):
    """B[q][i] = gamma_n * (sum_f |p_f q_f| + sum |bias terms| + |gm|), gamma_n = n u / (1 - n u), u = 2^-24,
    n = k + (bias / constant terms) + 2: the forward bound of a length-n fp32 sum in any order."""
    A = score_table(model, st, gm, prob, queries, absolute=True)
    n = np.array([k + n_bias_terms(model, prob, c) + 2 for (_, c) in queries], np.float64)
    return A * (n * U32 / (1.0 - n * U32))[:, None]


class TablePredict:
    """predict(u, j, c) for rank_oracle.eval_rankings from a precomputed score table (one row per query, read as a Python list)."""

    def __init__(self, F, queries, pos):
        self.F, self.row_of, self.pos, self.key, self.row = F, {q: i for i, q in enumerate(queries)}, pos, None, None

    def __call__(self, u, j, c):
        if self.key != (u, c):
            self.key, self.row = (u, c), self.F[self.row_of[(u, c)]].tolist()
        return self.row[self.pos[j]]


def modal_score(F):
    v, n = np.unique(F, return_counts=True)
    return float(v[np.argmax(n)]), int(n.max())


def add_short_query(prob, F, queries, thold, num_recs, seed):
    """Make the last user's first query a SHORT list: the user rates (in the query's context, appended to the training set, so the
    candidates' order stays) every candidate that scores above the threshold except min(3, num_recs - 1) of them.  Also a very long
    exclusion list.  Returns the query."""
    rng = np.random.default_rng(seed)
    q = next(x for x in queries if x[0] == prob.n_users - 1)
    have = {t[1] for t in prob.train if (t[0], t[2]) == q}
    passing = [prob.cand[i] for i in np.flatnonzero(F[queries.index(q)] > thold) if prob.cand[i] not in have]
    keep = set(rng.choice(len(passing), size=min(3, num_recs - 1, len(passing)), replace=False).tolist())
    prob.train += [(q[0], j, q[1], 3.0) for i, j in enumerate(passing) if i not in keep]
    return q


def eligible_mask(prob, queries):
    """E[q][i]: candidate i is not among the items the query's user rated in the query's context."""
    E = np.ones((len(queries), len(prob.cand)), bool)
    excl = excluded_columns(prob)
    for i, q in enumerate(queries):
        E[i, excl.get(q, [])] = False
    return E


# ---- premises ---------------------------------------------------------------------------------------------------------------

def check_exact_premise(model, st, gm, prob, F, queries, seed, n_sample=48):
    """Layer 1's premise, proven on the host: the state lies on the exact grid, and for a sample of (query, candidate) pairs the fp32
    sum of the score's terms -- accumulated term by term in forward, reverse and two shuffled orders -- equals the fp64 score."""
    for name, a in st.items():
        a64 = np.asarray(a, np.float64)
        unit = 8.0 if name in ("P", "Q") else 64.0
        assert a.dtype == np.float32 and np.all(np.abs(a64) <= 4.0) and np.all(a64 * unit == np.rint(a64 * unit)), name
    assert abs(gm) <= 4.0 and gm * 64.0 == round(gm * 64.0)
    rng = np.random.default_rng(seed)
    for _ in range(n_sample):
        qi, ci = int(rng.integers(len(queries))), int(rng.integers(len(prob.cand)))
        (u, c), j = queries[qi], prob.cand[ci]
        terms = np.array(score_terms(model, st, gm, prob, u, j, c), np.float64)
        t32 = terms.astype(np.float32)
        assert np.array_equal(t32.astype(np.float64), terms)                      # every product is itself an fp32 number
        assert len(terms) - st["P"].shape[1] <= 34
        exact = math.fsum(terms.tolist())
        assert exact == F[qi, ci], (qi, ci)
        for order in (np.arange(len(t32)), np.arange(len(t32))[::-1], rng.permutation(len(t32)), rng.permutation(len(t32))):
            s = np.add.accumulate(t32[order], dtype=np.float32)[-1]               # sequential fp32 accumulation
            assert float(s) == exact, (qi, ci, float(s), exact)


def unambiguous(F, B, E, thold, num_recs):
    """Per query, from the reference alone: (mask, expected top list as candidate positions).  A query is unambiguous when the top
    num_recs + 1 eligible fp64 scores are pairwise more than 2 B apart (B = the larger of the pair's bounds), none of them is within its
    B of the threshold, and no candidate behind them can reach into the list or over the threshold within its own bound: then every
    fp32 evaluation that honours the bound produces the same list."""
    ok, tops = [], []
    for f, b, e in zip(F, B, E):
        idx = np.flatnonzero(e)
        order = idx[np.argsort(-f[idx], kind="stable")]
        top, tail = order[:num_recs + 1], order[num_recs + 1:]
        ft, bt = f[top], b[top]
        good = bool(np.all(ft[:-1] - ft[1:] > 2.0 * np.maximum(bt[:-1], bt[1:]))) and bool(np.all(np.abs(ft - thold) > bt))
        lst = [int(i) for i in top[:num_recs] if f[i] > thold]
        if len(tail):
            if len(lst) == num_recs:
                last = top[num_recs - 1]
                good = good and bool(np.max(f[tail] + b[tail]) < f[last] - b[last])
            else:
                good = good and bool(np.all(f[tail] + b[tail] < thold))
        ok.append(good)
        tops.append(lst)
    return np.array(ok), tops
