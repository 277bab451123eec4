"""tests/ext_rank_anchor.py for FM, the one model whose evaluation code is its own: fm_predict_kernel (fm_kernels.hip) and the operand
builders rank_fm_items / rank_fm_queries (rank_kernels.hip) in front of the fp64 contraction.  Inputs and the fp64 reference for
tests/test_fm_anchor_ref.py (host) and tests/test_gpu_fm_eval_anchor.py: FM.predict restated, its score table in extended precision, the
forward error bound of a device score, model makers, ranking problems in FM's context form.  Everything here is numpy on the host;
nothing imports the GPU library.

FM.predict (FM.java:93-113) over the feature vector of FM.java:76-91 -- p = numUsers + numItems + numConditions entries, 1 at u and at
numUsers + j, xc = 1 / numContextDims at indexc = numUsers + numItems + c where c is the id of the context COMBINATION, and 0 elsewhere; an
indexc >= p matches no entry (the index quirk: a context whose id is >= numConditions has no feature):
    pred = w0;  for l < p: pred += w[l] * fs[l]
    for f < k:  sum1 = sum2 = 0;  for l < p: dot = V[l][f] * fs[l]; sum1 += dot; sum2 += dot^2;     sum += sum1^2 - sum2
    pred += 0.5 * sum
predict_seq is that, every operation in fp64 and in Java's order, the zero features included: an entry of w or V that is an infinity or
a NaN at a coordinate the tuple does not hold adds 0 * Inf = NaN.  On a finite model the zero features add exact zeros, and with
d0 = v_u,f, d1 = v_j,f, d2 = fl(v_c,f xc) (0 without a context feature) the sum is
    pred = ((w0 + w_u) + w_j) + fl(w_c xc) + 0.5 * sum_f [ ((d0 + d1) + d2)^2 - ((d0^2 + d1^2) + d2^2) ]
seq_table is this in fp64 and in that order (what predict_seq returns, for a whole table at once); score_table the same sum in
np.longdouble (2^-64 on x86: its own error is 2^-11 of the bound below) rounded once to fp64.  Both are valid for FINITE models only
and refuse others.

The device has two forms.  fm_predict_kernel: the sum above, lanes striding over f (a lane adds its ceil(k / 64) terms, six shuffle
additions join the lanes).  The rankings: a_f = fl(v_u,f + fl(xc v_c,f)), b = [V_j | w_j] against [a | 1], padded with zeros to
kp = 16 ceil((k + 1) / 16) columns, plus the row constant w0 + w_u + (fl(xc w_c) + fl(xc s)), s = <v_u, v_c> summed through a
64-entry LDS array (a lane adds its ceil(kp / 64) products, one thread adds the 64 entries in order).

The forward bound B = gamma_n * A, gamma_n = n u / (1 - n u), u = 2^-53; derived here, nothing in it is measured.
  A = |w0| + |w_u| + |w_j| + |xc w_c| + 1/2 sum_f [ (|d0| + |d1| + |d2|)^2 + d0^2 + d1^2 + d2^2 ]
      the magnitudes of the sum above.  The pairwise form's are |d0 d1| + |d2 d1| + |d0 d2| per factor -- that is
      1/2 [ (|d0| + |d1| + |d2|)^2 - d0^2 - d1^2 - d2^2 ], less than A's share -- and the same linear terms.
  n = the roundings on the longest chain from an input to the result, over the three evaluations (a fused multiply-add only removes one):
      Java's order      d2 (1), the two additions of sum1 that follow (2), all three counted twice by the square and the square itself
                        (2 * 3 + 1 = 7; the sum2 side has fewer), the subtraction (8), k additions of `sum +=`, `pred +=`:       k + 9
      predict kernel    the same 8, then ceil(k / 64) additions in the lane, 6 across lanes, `pred +=`:              15 + ceil(k / 64)
      pairwise, a_f b_f a_f (2), the product (1), at most kp additions in the contraction, the row constant added (1):          kp + 4
      pairwise, v_u v_c the product (1), ceil(kp / 64) in the lane, 64 through the LDS array, xc s (1), the sum with xc w_c (1),
                        added to w0 + w_u (1), the contraction added (1):                                           69 + ceil(kp / 64)
      The linear terms pass through 5 roundings at most.  n is the largest of the four: 70 at k = 1, 148 at k = 130.
Two evaluations that each honour B are within 2 B of each other; a gap of more than 4 B between two reference scores therefore keeps
their order in every evaluation that honours B, with 2 B to spare."""
import math
import zlib
from types import SimpleNamespace

import numpy as np

from tests import rank_anchor as ra

LD = np.longdouble
U64 = 2.0 ** -53
FAR = 100003                            # a context id far above every numConditions used here
R_POS, R_NEG = ra.R_POS, ra.R_NEG


# ---- models -----------------------------------------------------------------------------------------------------------------
def _model(k, n_users, n_items, n_conds, n_dims, w0, w, V):
    p = n_users + n_items + n_conds
    assert w.shape == (p,) and V.shape == (p, k)
    return SimpleNamespace(k=k, n_users=n_users, n_items=n_items, n_conds=n_conds, n_dims=n_dims, p=p, w0=float(w0),
                           w=np.ascontiguousarray(w, np.float64), V=np.ascontiguousarray(V, np.float64))


def real_model(k, n_users, n_items, n_conds, n_dims, seed):
    """the scale of a trained model on 1..5 ratings: w0 = 3.5, w ~ N(0, 0.5), V ~ N(0, 0.3)"""
    rng = np.random.default_rng(seed)
    p = n_users + n_items + n_conds
    return _model(k, n_users, n_items, n_conds, n_dims, 3.5, 0.5 * rng.standard_normal(p), 0.3 * rng.standard_normal((p, k)))


def loud_model(k, n_users, n_items, n_conds, n_dims, seed):
    """V ~ N(0, 30): sum1^2 - sum2 cancels (both are thousands, their difference 2 (d0 d1 + d0 d2 + d1 d2)); the pairwise form does not"""
    rng = np.random.default_rng(seed)
    p = n_users + n_items + n_conds
    return _model(k, n_users, n_items, n_conds, n_dims, 3.5, 0.5 * rng.standard_normal(p), 30.0 * rng.standard_normal((p, k)))


def grid_model(k, n_users, n_items, n_conds, n_dims, seed):
    """The exact grid: w and V multiples of 2^-4 with |x| <= 1, w0 = 3.5, numContextDims a power of two <= 4 (xc = 1, 1/2, 1/4).  Then d2
    and a_f are multiples of 2^-6, every product of either form (d^2, sum1^2, a_f b_f, xc v_u v_c, xc w_c) a multiple of 2^-12, and every
    partial sum of either form is bounded by A <= 6.5 + 6 k < 2^11 for k <= 256: 23 significant bits, exact in fp64 in ANY order.
    check_grid compares the three evaluations of this module bit for bit."""
    assert n_dims in (1, 2, 4) and k <= 256
    rng = np.random.default_rng(seed)
    p = n_users + n_items + n_conds
    return _model(k, n_users, n_items, n_conds, n_dims, 3.5, rng.integers(-16, 17, p) / 16.0, rng.integers(-16, 17, (p, k)) / 16.0)


MAKERS = {"grid": grid_model, "real": real_model, "loud": loud_model}


def with_one_more_condition(m, seed):
    """the model with numConditions + 1: a context id equal to m.n_conds holds a feature in it (what a `c <= n_conds` would read, if the
    row past the end of V held numbers of the model's own scale)"""
    rng = np.random.default_rng(seed)
    scale = float(np.abs(m.V).mean())
    return _model(m.k, m.n_users, m.n_items, m.n_conds + 1, m.n_dims, m.w0, np.append(m.w, 0.5),
                  np.vstack([m.V, scale * (1.0 + rng.random((1, m.k)))]))


# ---- the reference ----------------------------------------------------------------------------------------------------------
def predict_seq(m, u, j, c):
    """FM.predict(u, j, c) (FM.java:76-113) in fp64, the dense walk over all p entries in Java's order: np.add.accumulate is the running
    sum `s += x` (each output is the previous one plus the next input), taken along l; the sum over f is a loop over Python floats."""
    indexu, indexj, indexc = u, m.n_users + j, m.n_users + m.n_items + c
    i = np.arange(m.p)
    fs = np.where((i == indexu) | (i == indexj), 1.0, np.where(i == indexc, 1.0 / m.n_dims, 0.0))            # FM.java:82-89
    with np.errstate(invalid="ignore", over="ignore"):
        pred = float(np.add.accumulate(np.concatenate(([m.w0], m.w * fs)))[-1])                              # FM.java:96-98
        dot = m.V * fs[:, None]                                                                               # FM.java:104
        sum1 = np.add.accumulate(dot, axis=0)[-1].tolist()                                                    # FM.java:105
        sum2 = np.add.accumulate(dot * dot, axis=0)[-1].tolist()                                              # FM.java:106
    total = 0.0
    for f in range(m.k):
        total += sum1[f] * sum1[f] - sum2[f]                                                                  # FM.java:108
    return pred + 0.5 * total                                                                                 # FM.java:111


def clip(x, lo, hi):
    """Recommender.predict(u, j, c, bound) (Recommender.java:306-317): two comparisons, both false on a NaN"""
    x = np.array(x, np.float64)
    x[x > hi] = hi
    x[x < lo] = lo
    return x


def _eval(m, U, J, C, T, absolute=False, k_cut=None, xc=None, drop_ctx=False, drop_wj=False):
    """the sum of the module docstring for index arrays U, J, C that broadcast against each other, in the number type T and in Java's
    order; absolute=True: A.  The keywords make the WRONG sums the premises of tests/test_fm_anchor_ref.py are about."""
    assert np.isfinite(m.w0) and np.isfinite(m.w).all() and np.isfinite(m.V).all(), "valid for finite models only: use predict_seq"
    U, J, C = np.asarray(U), np.asarray(J), np.asarray(C)
    has = (C < m.n_conds) & (not drop_ctx)
    ic = np.where(has, m.n_users + m.n_items + C, 0)
    x = T(np.float64(1.0 / m.n_dims if xc is None else xc))                        # the reference's xc is the double, also in extended precision
    k = m.k if k_cut is None else min(m.k, k_cut)
    w, V = m.w.astype(T), m.V.astype(T)
    zero = T(0.0)
    wc = np.where(has, w[ic] * x, zero)
    Vu, Vj, Vc = V[U], V[m.n_users + J], np.where(has[..., None], V[ic] * x, zero)
    if absolute:
        out = ((abs(T(m.w0)) + np.abs(w[U])) + np.abs(w[m.n_users + J])) + np.abs(wc)
        for f in range(k):
            d0, d1, d2 = np.abs(Vu[..., f]), np.abs(Vj[..., f]), np.abs(Vc[..., f])
            s1 = (d0 + d1) + d2
            out = out + T(0.5) * (s1 * s1 + ((d0 * d0 + d1 * d1) + d2 * d2))
        return out
    pred = (T(m.w0) + w[U]) + (zero if drop_wj else w[m.n_users + J])
    pred = pred + wc
    total = np.zeros(np.broadcast(U, J, C).shape, T)
    for f in range(k):
        d0, d1, d2 = Vu[..., f], Vj[..., f], Vc[..., f]
        s1 = (d0 + d1) + d2
        total = total + (s1 * s1 - ((d0 * d0 + d1 * d1) + d2 * d2))
    return pred + T(0.5) * total


def _grid(users, items, ctx):
    return np.asarray(users)[:, None], np.asarray(items)[None, :], np.asarray(ctx)[:, None]


def seq_table(m, users, items, ctx, **wrong):
    """F[q][i] = predict_seq(m, users[q], items[i], ctx[q]) for a FINITE model: fp64, Java's order, the zero features left out"""
    return _eval(m, *_grid(users, items, ctx), np.float64, **wrong)


def score_table_ld(m, users, items, ctx, **wrong):
    """the same sum in extended precision, not yet rounded (FINITE models only)"""
    return _eval(m, *_grid(users, items, ctx), LD, **wrong)


def score_table(m, users, items, ctx, **wrong):
    """... rounded once to fp64 (FINITE models only)"""
    return score_table_ld(m, users, items, ctx, **wrong).astype(np.float64)


def n_roundings(k):
    """n of gamma_n (module docstring)"""
    kp = 16 * ((k + 1 + 15) // 16)
    return max(k + 9, 15 + -(-k // 64), kp + 4, 69 + -(-kp // 64))


def gamma(k):
    n = n_roundings(k)
    return n * U64 / (1.0 - n * U64)


def bound_table(m, users, items, ctx):
    """B[q][i] (module docstring); FINITE models only"""
    return _eval(m, *_grid(users, items, ctx), LD, absolute=True).astype(np.float64) * gamma(m.k)


def bound(m, u, j, c):
    return float(_eval(m, np.array([u]), np.array([j]), np.array([c]), LD, absolute=True)[0]) * gamma(m.k)


def tuple_scores(m, u, j, c):
    """(extended-precision scores, bounds) of the tuples (u[t], j[t], c[t]); FINITE models only"""
    return _eval(m, u, j, c, LD), _eval(m, u, j, c, LD, absolute=True).astype(np.float64) * gamma(m.k)


def check_grid(m, users, items, ctx, seed, n_sample=24):
    """The exact-grid premise: the model lies on the grid; the table in fp64 and Java's order equals the extended-precision one bit for
    bit in every entry (nothing was rounded in either); and predict_seq, the dense walk, equals both on a sample.  Returns the table."""
    for a in (m.w, m.V):
        assert np.all(np.abs(a) <= 1.0) and np.array_equal(a * 16.0, np.rint(a * 16.0))
    assert m.w0 * 16.0 == round(m.w0 * 16.0) and abs(m.w0) <= 4.0 and m.n_dims in (1, 2, 4) and m.k <= 256
    F, Fx = seq_table(m, users, items, ctx), score_table_ld(m, users, items, ctx)
    assert np.array_equal(F.astype(LD), Fx)
    rng = np.random.default_rng(seed)
    for _ in range(n_sample):
        q, i = int(rng.integers(len(users))), int(rng.integers(len(items)))
        assert predict_seq(m, int(users[q]), int(items[i]), int(ctx[q])) == F[q, i], (q, i)
    return F


# ---- problems ---------------------------------------------------------------------------------------------------------------
def make_problem(nc, n_users, n_conds, seed):
    """rank_anchor.make_problem (exactly nc candidates with sparse ids, so the HashSet order is not ascending; long exclusion lists;
    correct items that are no candidates) with FM's contexts: a context is its combination's id.  The twelve ids are renamed so that
    users 0, 1 and 2 have a query in the contexts n_conds - 1 (the last id that holds a feature), n_conds (the first that does not) and
    FAR; condition n_conds - 2 is held by no context at all.  One more user than the problem has tuples for: user n_users - 1 has no
    query and no rating.  free_item is no candidate and in no tuple."""
    assert 5 <= n_conds <= 10
    prob = ra.make_problem("FM", nc, n_users - 1, n_conds, seed)
    name = {c: c for c in range(prob.n_ctx)}
    name.update({0: n_conds - 1, n_conds - 1: 0, 1: n_conds, n_conds: 1, 2: FAR, n_conds - 2: FAR + 1})
    assert len(set(name.values())) == prob.n_ctx
    re = lambda ts: [(t[0], t[1], name[t[2]], t[3]) for t in ts]  # noqa: E731
    train, test = re(prob.train), re(prob.test)
    queries = [(u, name[c]) for u, c in prob.queries]
    assert {(0, n_conds - 1), (1, n_conds), (2, FAR)} <= set(queries) and len(set(queries)) == len(queries)
    assert all(t[2] != n_conds - 2 for t in train + test)
    used = {t[1] for t in train + test}
    free_item = next(j for j in range(prob.n_items) if j not in used)
    return SimpleNamespace(n_users=n_users, n_items=prob.n_items, n_conds=n_conds, train=train, test=test, cand=prob.cand, pos=prob.pos,
                           queries=queries, q_users=np.array([q[0] for q in queries]), q_ctx=np.array([q[1] for q in queries]),
                           items=np.array(prob.cand), free_user=n_users - 1, free_item=free_item, free_cond=n_conds - 2)


def plant_ties(m, prob):
    """two pairs of candidates with identical V rows and w: exact ties in every query, in every evaluation.  Returns the pairs as
    candidate positions (first < second)."""
    nc = len(prob.cand)
    pairs = [(1, nc // 2), (7, nc - 1)]
    for a, b in pairs:
        la, lb = m.n_users + prob.cand[a], m.n_users + prob.cand[b]
        m.V[lb], m.w[lb] = m.V[la], m.w[la]
    return pairs


def eligible(prob):
    """E[q][i]: candidate i is not among the items the query's user rated in the query's context"""
    return ra.eligible_mask(prob, prob.queries)


def min_gap_ratio(F, B, E, pairs, num_recs):
    """Per query: the smallest (gap / 4 B) between adjacent scores among the first num_recs + 1 eligible candidates in the reference's
    order (stable, descending), B the largest bound of the query's row; the gap inside a planted pair (exactly 0) is left out.  A ratio
    above 1 for every query means every evaluation that honours B gives the reference's list (module docstring; whatever lies behind
    the first num_recs + 1 is below the last listed score by more than 4 B as well)."""
    tied = {x: i for i, pair in enumerate(pairs) for x in pair}
    out = []
    for f, b, e in zip(F, B, E):
        idx = np.flatnonzero(e)
        top = idx[np.argsort(-f[idx], kind="stable")][:num_recs + 1]
        r = math.inf
        for x, y in zip(top[:-1], top[1:]):
            if tied.get(int(x), -1) == tied.get(int(y), -2):
                assert f[x] == f[y] and x < y
                continue
            r = min(r, float(f[x] - f[y]) / (4.0 * float(b.max())))
        out.append(r)
    return np.array(out)


def predict_tuples(m, n, seed):
    """n tuples for predict: any user, any item of the id space; contexts n_conds - 1, n_conds, FAR, 0 in turn, then any id below
    2 n_conds"""
    rng = np.random.default_rng(seed)
    u = rng.integers(0, m.n_users, n).astype(np.int32)
    j = rng.integers(0, m.n_items, n).astype(np.int32)
    c = rng.integers(0, 2 * m.n_conds, n).astype(np.int32)
    head = [m.n_conds - 1, m.n_conds, FAR, 0]
    c[:min(n, 4)] = head[:min(n, 4)]
    return u, j, c


# ---- the cases of tests/test_fm_anchor_ref.py and tests/test_gpu_fm_eval_anchor.py ---------------------------------------------
KINDS = ("grid", "real", "loud")
PREDICT_K = (1, 15, 16, 17, 63, 64, 65, 128, 130)      # the 64-lane stride of fm_predict_kernel: below, at, above, twice, twice and two
PREDICT_N = (1, 4, 5, 257)                             # a block's four waves: one, all, one over, many blocks
PREDICT_DIMS = {"grid": (1, 2, 4), "real": (1, 2, 3), "loud": (1, 2, 3)}
TOPN_K = (14, 15, 16, 31, 63, 64, 65, 128)             # kp = 16, 16, 32, 32, 64, 80, 80, 144
TOPN_NC = (63, 64, 65, 257)                            # the contraction's 64-wide tile
TOPN_DIMS = {"grid": 4, "real": 3, "loud": 2}
NUM_RECS = (10, 64, 70)
TOPN_USERS, N_CONDS, THOLD = 70, 5, 2.5                # 69 users with one or two queries each: the 64-row query tile is crossed
RESEED = {}                                            # (kind, k, nc) -> salt, where the first draw misses the gap premise (none does)


def seed_of(*parts):
    return zlib.crc32(repr(parts).encode())


def predict_case(kind, k, n_dims):
    """(model, {n: (u, j, c)}) of a predict case: 40 users, 90 items"""
    m = MAKERS[kind](k, 40, 90, N_CONDS, n_dims, seed_of("predict", kind, k, n_dims))
    return m, {n: predict_tuples(m, n, seed_of("tuples", kind, k, n_dims, n)) for n in PREDICT_N}


def topn_case(kind, k, nc):
    """(problem, model with its planted ties, the pairs) of a top-N case"""
    prob = make_problem(nc, TOPN_USERS, N_CONDS, seed_of("problem", nc))
    m = MAKERS[kind](k, prob.n_users, prob.n_items, N_CONDS, TOPN_DIMS[kind], seed_of("model", kind, k, nc, RESEED.get((kind, k, nc), 0)))
    return prob, m, plant_ties(m, prob)


NF_K, NF_NC, NF_USERS = 5, 80, 21
NF_VALUES = (math.inf, -math.inf, math.nan)
# (field, coordinate, touched): a coordinate no query or tuple holds -- the user without queries, the item that is no candidate, the
# condition no context holds -- and one that some do: user 0, candidate 5, condition n_conds - 1 (user 0's first query)
NF_CASES = [("w0", None, True, v) for v in NF_VALUES] + \
           [(fld, co, t, v) for fld in ("w", "V") for co in ("user", "item", "cond") for t in (False, True) for v in NF_VALUES]


def nf_id(case):
    return "%s-%s-%s-%s" % (case[0], case[1], "touched" if case[2] else "untouched", case[3])


def nonfinite_case(case):
    """(problem, model) with the one planted entry; every other entry is finite, at the real scale"""
    field, coord, touched, value = case
    prob = make_problem(NF_NC, NF_USERS, N_CONDS, seed_of("nf problem"))
    m = real_model(NF_K, prob.n_users, prob.n_items, N_CONDS, 2, seed_of("nf model"))
    if field == "w0":
        m.w0 = value
        return prob, m
    l = {"user": 0 if touched else prob.free_user,
         "item": m.n_users + (prob.cand[5] if touched else prob.free_item),
         "cond": m.n_users + m.n_items + (N_CONDS - 1 if touched else prob.free_cond)}[coord]
    if field == "w":
        m.w[l] = value
    else:
        m.V[l, NF_K // 2] = value
    return prob, m


def nonfinite_table(m, prob):
    """predict_seq for every (query, candidate): the dense walk, one call per score"""
    return np.array([[predict_seq(m, u, j, c) for j in prob.cand] for u, c in prob.queries])
