"""Models whose top-N scores are exact in every form the device computes them, with planted NaN, +Inf and -Inf scores.

Dyadic models: every finite entry of P, Q, the bias tables and the global mean is a multiple of 1/8 in [-1/2, 1/2] and k = 12, so every
product is a multiple of 1/64 and every partial sum is exact in fp32 in any association: the fp64 chain, the fp32 contraction, the split
sum (S1 + S2) + rc and the reference give the same finite scores bit for bit, and whether a sum is +Inf, -Inf or NaN depends only on
which terms it has (a NaN term or both infinities: NaN; else the infinity; 0 * Inf is a NaN term), not on their order.

Candidates sit at chosen POSITIONS of the reference's candidate order (a HashSet<Integer>): the 581 item ids have distinct hash buckets
in the final table of 1024, so the order is by bucket whatever the order of the training tuples, and it is not the order of the ids.

  set A (Q[j][0] = +Inf): positions 0, 63, 64, 511, 512, 575 (the last full tile's last slot), 580 (the last) and the whole tile 192..255
  set B (Q[j][1] = -Inf): positions 0, 64, 250, 580 (all in A) and 100, 300, 400
  a user's (P[u][0], P[u][1]) is drawn from {+1/2, -1/2, 0}^2: users 0..8 take the nine pairs in the order of SIGNS, so each of A \\ B,
  B \\ A and the intersection is +Inf, -Inf or NaN for that user (0 * Inf and Inf - Inf both occur)
  user 9: P[u][0] = NaN, every score NaN          user 12: P[u][0] = -Inf and Q[:, 0] >= 0, every score -Inf or NaN
  user 10: the pair (-, -) and P[u][2..5] = -1/2 against Q[:, 2..5] = 1/2: every finite score is <= -1 except on the four SURVIVORS
  user 11: the pair (+, -); in the MF family its row constant is -Inf (userBias, or ucBias of every condition where there is no userBias)
  MF family: itemBias = +Inf at IB_PINF and -Inf at IB_NINF; icBias of condition 0 = -Inf at IC_NINF (which meets A: +Inf in S1 and -Inf
  in S2 at one candidate) and +Inf at IC_PINF.  Contexts 0 and 1 hold condition 0, contexts 2 and 3 do not: there the reference never
  reads those entries and the scores stay finite.
"""
import functools
import math

import numpy as np

from oracle import rank_oracle

NC, NU, K, N_ITEMS, N_CONDS = 64 * 9 + 5, 40, 12, 3072, 4
CTX_PTR = np.array([0, 2, 4, 6, 8], np.int32)
CTX_CONDS = np.array([0, 2, 0, 3, 1, 2, 1, 3], np.int32)          # contexts 0, 1 hold condition 0; 2, 3 hold condition 1
CTX = [CTX_CONDS[CTX_PTR[c]:CTX_PTR[c + 1]].tolist() for c in range(4)]
GM = 0.125

SPECIAL = (0, 63, 64, 511, 512, 575, 580)
TILE = tuple(range(192, 256))
A = tuple(sorted(set(SPECIAL) | set(TILE)))
B = (0, 64, 100, 250, 300, 400, 580)
SURVIVORS = (5, 130, 333, 579)
IB_PINF, IB_NINF = (1, 513), (2, 320)
IC_NINF, IC_PINF = (63, 200, 450), (3, 451, 576)
SIGNS = [(a, b) for a in (0.5, -0.5, 0.0) for b in (0.5, -0.5, 0.0)]   # users 0..8
U_PP, U_PM, U_P0, U_MP, U_MM, U_M0, U_0P, U_0M, U_00, U_NAN, U_LOW, U_RC, U_NINF = range(13)

MF_MODELS = ("BiasedMF", "CAMF_CI", "CAMF_CUCI")


@functools.lru_cache(maxsize=None)
def items():
    """(cand, pos): the 581 item ids in candidate order and id -> position"""
    rng = np.random.default_rng(20261020)
    buckets = np.sort(rng.choice(1024, NC, replace=False))
    cand = (buckets + 1024 * rng.integers(0, 3, NC)).tolist()
    return cand, {j: p for p, j in enumerate(cand)}


@functools.lru_cache(maxsize=None)
def factors():
    """(P, Q) of every model, fp64; Q over all N_ITEMS ids (the rows of ids that are no candidates stay zero)"""
    rng = np.random.default_rng(20261021)
    cand, _ = items()
    Qc = np.zeros((NC, K))
    Qc[:, 0:2] = rng.choice([0.0, 0.125, 0.25, 0.5], (NC, 2))
    Qc[:, 2:6] = 0.5
    Qc[:, 6:] = rng.choice([-0.5, 0.0, 0.0, 0.5], (NC, K - 6))
    Qc[list(SURVIVORS), 0:6] = 0.0
    Qc[list(A), 0] = np.inf
    Qc[list(B), 1] = -np.inf
    P = np.zeros((NU, K))
    P[:, 6:] = rng.choice([-0.5, 0.0, 0.5], (NU, K - 6))
    pairs = SIGNS + [SIGNS[int(x)] for x in rng.integers(0, 9, NU - 9)]
    pairs[U_NAN], pairs[U_LOW], pairs[U_RC], pairs[U_NINF] = (np.nan, 0.5), (-0.5, -0.5), (0.5, -0.5), (-np.inf, 0.0)
    P[:, 0:2] = np.array(pairs)
    P[U_LOW, 2:6] = -0.5
    P[U_LOW, 6:] = 0.0
    Q = np.zeros((N_ITEMS, K))
    Q[cand] = Qc
    return P, Q


@functools.lru_cache(maxsize=None)
def state(model):
    """the state tables of `model` ("PQ": the factor models whose score is the row product; or one of MF_MODELS), fp64"""
    P, Q = factors()
    st = {"P": P, "Q": Q}
    if model == "PQ":
        return st
    rng = np.random.default_rng(20261022)
    cand, _ = items()
    at = lambda ps: [cand[p] for p in ps]  # noqa: E731
    if model in ("BiasedMF", "CAMF_CI"):
        st["userBias"] = rng.choice([-0.5, -0.25, 0.0, 0.25, 0.5], NU)
        st["userBias"][U_RC] = -np.inf
        st["userBias"][U_LOW] = -0.5
    if model == "BiasedMF":
        st["itemBias"] = np.zeros(N_ITEMS)
        st["itemBias"][cand] = rng.choice([-0.25, 0.0, 0.0, 0.25], NC)
        st["itemBias"][at(IB_PINF)] = np.inf
        st["itemBias"][at(IB_NINF)] = -np.inf
    if model in ("CAMF_CI", "CAMF_CUCI"):
        st["icBias"] = np.zeros((N_ITEMS, N_CONDS))
        st["icBias"][cand] = rng.choice([-0.125, 0.0, 0.0, 0.125], (NC, N_CONDS))
        st["icBias"][at(IC_NINF), 0] = -np.inf
        st["icBias"][at(IC_PINF), 0] = np.inf
    if model == "CAMF_CUCI":
        st["ucBias"] = rng.choice([-0.125, 0.0, 0.125], (NU, N_CONDS))
        st["ucBias"][U_RC, :] = -np.inf
        st["ucBias"][U_LOW, :] = -0.25
    return st


def score_slab(model, dtype=np.float64, form="chain"):
    """S[c, u, p]: the score of user u in context c for the candidate at position p, every operation in `dtype`.
    form "chain": the reference's predict(), terms in its order, the dot product ascending; "reversed": the dot product descending and
    the biases in front of it; "split": (S1 + S2) + rc with S1 = dot + itemBias, S2 = the sum of the context's icBias entries, rc = the
    terms that do not depend on the item -- the device's split form; "onehot": the chain with EVERY condition's icBias entry multiplied
    by the context's one-hot row, zeros included -- what a contraction over one-hot columns computes if nothing mends it, and NOT what
    the reference computes: 0 * Inf is a NaN"""
    cand, _ = items()
    st = {n: a.astype(dtype) for n, a in state(model).items()}
    P, Qc = st["P"], st["Q"][cand]
    gm = dtype(GM if model != "PQ" else 0.0)
    zero = lambda *shape: np.zeros(shape, dtype)  # noqa: E731
    with np.errstate(invalid="ignore"):
        dot = zero(NU, NC)
        for f in (range(K) if form != "reversed" else range(K - 1, -1, -1)):
            dot = dot + P[:, f][:, None] * Qc[:, f][None, :]
        ub = st["userBias"][:, None] if "userBias" in st else None
        ib = st["itemBias"][cand][None, :] if "itemBias" in st else None
        ic = st["icBias"][cand] if "icBias" in st else None
        uc = st.get("ucBias")
        out = zero(4, NU, NC)
        for c in range(4):
            if form == "split":
                s1 = dot + ib if ib is not None else dot
                rc = zero(NU, 1) + gm
                if ub is not None:
                    rc = rc + ub
                s2 = zero(1, NC)
                for cond in CTX[c]:
                    if uc is not None:
                        rc = rc + uc[:, cond][:, None]
                    if ic is not None:
                        s2 = s2 + ic[:, cond][None, :]
                out[c] = ((s1 + s2) if ic is not None else s1) + rc
                continue
            if model == "PQ":
                s = dot
            elif form == "reversed":
                s = zero(NU, NC)
                for cond in reversed(CTX[c]):
                    if ic is not None:
                        s = s + ic[:, cond][None, :]
                    if uc is not None:
                        s = s + uc[:, cond][:, None]
                for t in (ib, ub):
                    if t is not None:
                        s = s + t
                s = (s + gm) + dot
            else:
                s = zero(NU, NC) + gm                       # BiasedMF: gm + userBias + itemBias + dot; CAMF_CI: gm + userBias + dot + ...
                if ub is not None:
                    s = s + ub
                if ib is not None:
                    s = s + ib
                s = s + dot
                for cond in CTX[c]:                         # CAMF_CI: += icBias; CAMF_CUCI: += icBias + ucBias
                    if ic is not None and uc is not None:
                        s = s + (ic[:, cond][None, :] + uc[:, cond][:, None])
                    elif ic is not None and form != "onehot":
                        s = s + ic[:, cond][None, :]
                if form == "onehot" and ic is not None and uc is None:
                    for cond in range(N_CONDS):
                        s = s + dtype(cond in CTX[c]) * ic[:, cond][None, :]
            out[c] = s
    return out


@functools.lru_cache(maxsize=None)
def scores(model):
    """the reference's scores, fp64: S[c, u, p]"""
    s = ext_score_slab(model) if model in EXT_MODELS else score_slab(model)
    s.setflags(write=False)
    return s


# ---- SVD++ and the similarity models CAMF_ICS / CAMF_LCS / CAMF_MCS (the operand builders of ext_kernels.hip) ---------------------------
# The similarity models multiply the FINISHED dot product by the context's similarities, one per dimension (CAMF_ICS.java:53-57,
# CAMF_LCS.java:43-61), or once by 1 - sqrt(dist) (CAMF_MCS.java:53-67).  Contexts are the reference's: one condition per dimension,
# the i-th against dimension i's ':na' condition SIM_EMPTY[i].  Two dimensions of four conditions; per condition the similarity to its
# partner (CAMF_ICS: the ccMatrix entry; CAMF_LCS: the dot product of two cfMatrix rows, one entry of a row at an infinity; CAMF_MCS: the
# difference of two positions, where an infinite or NaN position makes the scale -Inf or NaN -- a scale of +Inf does not exist there):
#   dimension 0: condition 0 +Inf, 1 NaN, 2 zero, 3 (':na', with itself) 2        dimension 1: 4 -Inf, 5 -1/2, 6 zero, 7 (':na') 1/2
# and the contexts' scales, in the order of SIM_CTX (ICS and LCS | MCS):
#   0 all empty: 2 * 1/2 = 1 | 1      1: +Inf | -Inf      2: -Inf | -Inf      3: NaN | NaN      4: 0 | 0      5: 2 * -1/2 = -1 | -1
#   6: the pair (+Inf, 0), a NaN by the reference's sequential product | -Inf      7: +Inf * -Inf = -Inf | -Inf
# P and Q are those of factors(): against every scale stand users whose dot products are positive, negative, exactly 0, +Inf, -Inf and
# NaN over the candidates, and every user's P row has zeros.
SIM_MODELS = ("CAMF_ICS", "CAMF_LCS", "CAMF_MCS")
EXT_MODELS = ("SVD++",) + SIM_MODELS
SIM_DIMS, SIM_CONDS, SIM_NUM_F = 2, 8, 2
SIM_EMPTY = np.array([3, 7], np.int32)
SIM_CTX = [(3, 7), (0, 7), (3, 4), (1, 7), (2, 7), (3, 5), (0, 6), (0, 4)]
SIM_NCTX = len(SIM_CTX)
SIM_CTX_PTR = np.arange(0, 2 * SIM_NCTX + 1, 2, dtype=np.int32)
SIM_CTX_CONDS = np.array(SIM_CTX, np.int32).reshape(-1)
SIM_FINITE_CTX = (0, 4, 5)
SIM_SCALES = {"CAMF_ICS": (1.0, np.inf, -np.inf, np.nan, 0.0, -1.0, np.nan, -np.inf),
              "CAMF_MCS": (1.0, -np.inf, -np.inf, np.nan, 0.0, -1.0, -np.inf, -np.inf)}
SIM_SCALES["CAMF_LCS"] = SIM_SCALES["CAMF_ICS"]
# SVD++: the user without a training tuple (|N(u)| = 0); users whose rated items' Y rows hold +Inf and -Inf in ONE factor, in two
# different factors, and -Inf alone (the items are candidate positions the user rated in every construction of svdpp_tuples)
U_DEG0, U_Y_SAME, U_Y_TWO, U_Y_ONE = U_00, 14, 15, 16
Y_PLANTS = {28: (6, np.inf), 55: (6, -np.inf), 29: (6, np.inf), 56: (7, -np.inf), 30: (6, -np.inf)}     # position: (factor, value)


def plus_zero(a):
    """`a` with every zero +0 (-0 + 0 = +0; every other value, infinities and NaN included, unchanged).  The similarity models' chain
    dot * s gives -0 where one of the two is negative and the other an exact zero; the device's sum of products starts from +0 and
    gives +0.  No comparison of the ranking tells the two apart (-0 == +0 for the threshold and for the sort)."""
    return np.asarray(a, np.float64) + 0.0


def tuples_of(model):
    return svdpp_tuples() if model == "SVD++" else tuples(SIM_NCTX) if model in SIM_MODELS else tuples()


def ctx_table(model):
    return (SIM_CTX_PTR, SIM_CTX_CONDS) if model in SIM_MODELS else (CTX_PTR, CTX_CONDS)


@functools.lru_cache(maxsize=None)
def svdpp_tuples():
    """tuples() for SVD++: unique (user, item) pairs (userItemsCache has no duplicates), no training tuple of U_DEG0, and every other
    user's degree filled up to 16 (users 0..12) or 64 (the others) with further candidates, so sqrt|N(u)| is a power of two and every
    sum stays exact; the items of Y_PLANTS are rated by their own user alone"""
    rng = np.random.default_rng(20261024)
    cand, _ = items()
    tr, te = _tuple_sets(4)
    planted = {cand[p] for p in Y_PLANTS}
    pairs, out = set(), set()
    for t in sorted(tr):
        if t[0] != U_DEG0 and t[:2] not in pairs and (t[1] not in planted or t[0] >= 13):
            pairs.add(t[:2])
            out.add(t)
    for u in range(NU):
        have = {j for (x, j) in pairs if x == u}
        want = 0 if u == U_DEG0 else 16 if u < 13 else 64
        assert len(have) <= want, (u, len(have))
        free = [j for j in cand if j not in have and j not in planted]
        for j in rng.choice(free, want - len(have), replace=False).tolist():
            out.add((u, j, u % 4))
    assert all([u for (u, j, _) in out if j == cand[p]] == [13 + p % 27] for p in Y_PLANTS)
    return _tuple_arrays(out, te)


@functools.lru_cache(maxsize=None)
def rated_items(model="SVD++"):
    """N(u) of every user: the items of its training tuples, ascending"""
    (u, j, _, _), _ = tuples_of(model)
    out = [[] for _ in range(NU)]
    for x, y in sorted(set(zip(u.tolist(), j.tolist()))):
        out[x].append(y)
    return out


@functools.lru_cache(maxsize=None)
def ext_state(model):
    """the state tables of an EXT model, fp64: P and Q of factors(), and the planted similarity tables / SVD++ biases and Y"""
    P, Q = factors()
    st = {"P": P, "Q": Q}
    rng = np.random.default_rng(20261025)
    cand, _ = items()
    inf, nan = np.inf, np.nan
    if model == "SVD++":
        at = lambda ps: [cand[p] for p in ps]  # noqa: E731
        st["userBias"] = rng.choice([-0.5, -0.25, 0.0, 0.25, 0.5], NU)
        st["userBias"][U_RC] = -inf
        st["userBias"][U_LOW] = -0.5
        st["itemBias"] = np.zeros(N_ITEMS)
        st["itemBias"][cand] = rng.choice([-0.25, 0.0, 0.0, 0.25], NC)
        st["itemBias"][at(IB_PINF)] = inf
        st["itemBias"][at(IB_NINF)] = -inf
        st["Y"] = np.zeros((N_ITEMS, K))
        st["Y"][cand] = rng.choice([-0.5, -0.125, 0.0, 0.0, 0.125, 0.25], (NC, K))
        for p, (f, v) in Y_PLANTS.items():
            st["Y"][cand[p], f] = v
    elif model == "CAMF_ICS":
        cc = np.full((SIM_CONDS, SIM_CONDS), 0.25)                   # (an entry read at a wrong index gives a finite scale)
        for c, e, v in ((0, 3, inf), (1, 3, nan), (2, 3, 0.0), (3, 3, 2.0), (4, 7, -inf), (5, 7, -0.5), (6, 7, 0.0), (7, 7, 0.5)):
            cc[c, e] = cc[e, c] = v
        st["ccMatrix"] = cc
    elif model == "CAMF_LCS":
        st["cfMatrix"] = np.array([[inf, 1.0], [nan, 0.0], [1.0, -1.0], [1.0, 1.0], [-inf, 1.0], [-1.0, 0.0], [1.0, -1.0], [0.5, 0.5]])
    else:
        st["cVector"] = np.array([inf, nan, 1.25, 0.25, -inf, 2.5, 1.5, 0.5])
    return st


def sim_chain(model, st):
    """per context the factors the reference multiplies the dot product by, in its order, fp64 from the state `st`"""
    out = []
    with np.errstate(invalid="ignore"):
        for ctx in SIM_CTX:
            sims, dist = [], np.float64(0.0)
            for c, e in zip(ctx, SIM_EMPTY.tolist()):
                if model == "CAMF_ICS":
                    sims.append(np.float64(st["ccMatrix"][c, e]))
                elif model == "CAMF_LCS":
                    s = np.float64(0.0)
                    for f in range(SIM_NUM_F):
                        s = s + np.float64(st["cfMatrix"][c, f]) * np.float64(st["cfMatrix"][e, f])
                    sims.append(s)
                else:
                    d = np.float64(st["cVector"][c]) - np.float64(st["cVector"][e])
                    dist = dist + d * d
            out.append(sims if model != "CAMF_MCS" else [np.float64(1.0) - np.sqrt(dist)])
    return out


def ext_score_slab(model, dtype=np.float64, form="chain"):
    """S[c, u, p] of an EXT model from its state rounded to `dtype`, every operation of the score in `dtype`.
    form "chain": the reference's predict() in its order -- the dot product ascending, then one multiplication per similarity; SVD++:
    gm + bu + bj + dot, then + dot(Y_k, Q_j) / sqrt|N(u)| per rated item, ascending (SVDPlusPlus.java:138-146).
    form "operand": the contraction over the device's operands -- a_q = fl(s * P_u) with s the product of the similarities formed in fp64,
    which is NOT what the reference computes when s is an infinity (Inf - Inf, 0 * Inf); SVD++: a_q = [fl(P_u + ysum / w) | 1],
    b_j = [Q_j | itemBias_j], + (gm + bu)"""
    cand, _ = items()
    st = {n: a.astype(dtype) for n, a in ext_state(model).items()}
    P, Qc = st["P"], st["Q"][cand]
    n_ctx = 4 if model == "SVD++" else SIM_NCTX
    out = np.zeros((n_ctx, NU, NC), dtype)

    def contract(A):
        s = np.zeros((NU, NC), dtype)
        for f in range(K):
            s = s + A[:, f][:, None] * Qc[:, f][None, :]
        return s
    with np.errstate(invalid="ignore", over="ignore"):
        if model == "SVD++":
            gm, ub, ib, Y, N = dtype(GM), st["userBias"][:, None], st["itemBias"][cand][None, :], st["Y"], rated_items()
            if form == "chain":
                s = ((gm + ub) + ib) + contract(P)
                for u in range(NU):
                    w = dtype(math.sqrt(len(N[u])))
                    for k in N[u]:
                        yq = np.zeros(NC, dtype)
                        for f in range(K):
                            yq = yq + Y[k, f] * Qc[:, f]
                        s[u] = s[u] + yq / w
            else:
                A = np.zeros((NU, K), np.float64)
                for u in range(NU):
                    ys = np.zeros(K, np.float64)
                    for k in N[u]:
                        ys = ys + Y[k].astype(np.float64)
                    A[u] = P[u].astype(np.float64) + (ys / math.sqrt(len(N[u])) if N[u] else 0.0)
                s = (contract(A.astype(dtype)) + dtype(1.0) * ib) + (gm + ub).astype(dtype)
            out[:] = s[None]
            return out
        chain = sim_chain(model, st)
        dot = contract(P)
        for c in range(n_ctx):
            if form == "chain":
                s = dot
                for sim in chain[c]:
                    s = s * dtype(sim)
            else:
                scale = np.float64(1.0)
                for sim in chain[c]:
                    scale = scale * sim
                s = contract((P.astype(np.float64) * scale).astype(dtype))
            out[c] = s
    return out


def _tuple_sets(n_ctx):
    rng = np.random.default_rng(20261023)
    cand, _ = items()
    tr = {(13 + p % 27, cand[p], p % n_ctx) for p in range(NC)}
    tr |= {(U_PM, cand[63], 0), (U_MM, cand[100], 1)}
    te = {(U_PM, cand[0], 0), (U_PP, cand[64], 1), (U_MM, cand[300], 0)}
    for u in range(NU):
        for c in (range(n_ctx) if u < 13 else ((u % n_ctx), (u + 1) % n_ctx)):
            if u < 13:
                tr |= {(u, cand[int(p)], c) for p in rng.choice(NC, 3, replace=False)}
            te |= {(u, cand[int(p)], c) for p in rng.choice(NC, 2, replace=False)}
    return tr, te


def _tuple_arrays(tr, te):
    arr = lambda ts, r: (np.array([t[0] for t in ts], np.int32), np.array([t[1] for t in ts], np.int32),  # noqa: E731
                         np.array([t[2] for t in ts], np.int32), np.full(len(ts), r))
    return arr(sorted(tr), 3.0), arr(sorted(te - tr), 5.0)


@functools.lru_cache(maxsize=None)
def tuples(n_ctx=4):
    """(train, test) as (u, j, ctx, r) arrays, sorted by (user, item, context).  Every candidate is rated once by a user of 13..39;
    users 0..12 have a query in every context, with three excluded items each; user 1 (pair (+, -)) has rated position 63 (+Inf for it)
    in context 0 only and has position 0 (+Inf) as a correct item there; user 4 (pair (-, -)) has rated position 100 in context 1.
    n_ctx: the number of contexts (4: the MF family and the slab form; SIM_NCTX: the similarity models)"""
    return _tuple_arrays(*_tuple_sets(n_ctx))


def as_lists(d):
    return list(zip(*[np.asarray(a).tolist() for a in d]))


@functools.lru_cache(maxsize=None)
def oracle(model, bin_thold, num_recs):
    """(measures, lists) of oracle/rank_oracle.eval_rankings over the reference's scores"""
    _, pos = items()
    s = scores(model)
    train, test = tuples_of(model)
    return rank_oracle.eval_rankings(lambda u, j, c: float(s[c, u, pos[j]]), as_lists(train), as_lists(test), bin_thold=bin_thold,
                                     num_recs=num_recs)


def mode_threshold(model):
    """the most frequent finite score of the model over every (context, user, candidate): a threshold exactly on it tells > from >="""
    s = scores(model)
    vals, counts = np.unique(s[np.isfinite(s)], return_counts=True)
    return float(vals[np.argmax(counts)])


# ---- selectors: the reference's rule and deliberately wrong ones ------------------------------------------------------------------
def select(row, excl, thold, num_recs, rule="reference", tile_bound=None):
    """the list [(position, score)] of one query from its scores by candidate position.  rule:
    reference      not NaN and score > thold; stable descending sort; the first num_recs
    nan_passes     admits whatever is not <= thold (a NaN too) and ranks a NaN last
    nan_is_pinf    a NaN counts as +Inf
    ninf_admitted  a NaN counts as -Inf, and -Inf is admitted when thold is below every finite double's reach (thold < -1e300 / 2)
    pinf_descending  equal +Inf scores in descending position
    full_accepts_pinf  a list that is full still takes a later +Inf, in place of its last entry
    nan_bound      tiles of 64 whose bound tile_bound[t] is NaN are not looked at"""
    ex = set(excl)
    entries = []
    for p, s in enumerate(row.tolist()):
        if p in ex:
            continue
        if rule == "nan_bound" and math.isnan(tile_bound[p // 64]):
            continue
        if rule == "nan_passes":
            ok, key = not s <= thold, (-math.inf if math.isnan(s) else s)
        elif rule == "nan_is_pinf":
            key = math.inf if math.isnan(s) else s
            ok = key > thold
        elif rule == "ninf_admitted":
            key = -math.inf if math.isnan(s) else s
            ok = key > thold or (thold < -0.5e300 and not math.isnan(s))
        else:
            ok, key = (not math.isnan(s)) and s > thold, s
        if ok:
            entries.append((p, s, key))
    if rule == "full_accepts_pinf":
        out = []
        for p, s, key in entries:                             # streaming: insert behind every entry >= the score; a full list ...
            if len(out) == num_recs:
                if key == math.inf:                           # ... takes a +Inf in place of its last entry
                    out[-1] = (p, s, key)
                    out.sort(key=lambda e: -e[2])
                    continue
                if not key > out[-1][2]:
                    continue
            out.append((p, s, key))
            out.sort(key=lambda e: -e[2])
            del out[num_recs:]
        return [(p, s) for p, s, _ in out]
    if rule == "pinf_descending":
        entries.sort(key=lambda e: (-e[2], -e[0] if e[2] == math.inf else e[0]))
    else:
        entries.sort(key=lambda e: -e[2])
    return [(p, s) for p, s, _ in entries[:num_recs]]


def lists_by(model, queries, thold, num_recs, rule="reference", bounds=None, s=None):
    """{(u, c): [(item, score)]} of every query of `queries` (capi.rank_plan's) that has a list under `rule`; s: scores to select from in
    place of the reference's"""
    cand, _ = items()
    s = scores(model) if s is None else s
    out = {}
    for q, (u, c, correct, excl) in enumerate(queries):
        got = select(s[c, u], excl, thold, num_recs, rule, None if bounds is None else bounds[q])
        if correct and got:
            out[(u, c)] = [(cand[p], v) for p, v in got]
    return out


def same_lists(a, b):
    """two {(u, c): [(item, score)]}: the same queries, items and score bits (a NaN equals a NaN)"""
    if a.keys() != b.keys():
        return False
    for key in a:
        if [i for i, _ in a[key]] != [i for i, _ in b[key]]:
            return False
        x, y = np.array([v for _, v in a[key]]), np.array([v for _, v in b[key]])
        if not np.all((x.view(np.int64) == y.view(np.int64)) | (np.isnan(x) & np.isnan(y))):
            return False
    return True


# ---- the tile bound of the pruned selection, restated in fp32 ----------------------------------------------------------------------
def tile_max(row, propagate_nan=False):
    """per tile of 64 candidates the largest value, NaN entries ignored (a tile of nothing but NaN: -Inf) -- or, propagate_nan, NaN as
    soon as the tile holds one"""
    nt = (len(row) + 63) // 64
    out = np.full(nt, -np.inf, np.float32)
    for t in range(nt):
        v = row[64 * t:64 * t + 64]
        if propagate_nan and np.isnan(v).any():
            out[t] = np.nan
        elif not np.isnan(v).all():
            out[t] = np.nanmax(v)
    return out


def split_parts(model):
    """(S1[u, p], S2[c, p] or None, rc[c, u]) in fp32, as the split form holds them"""
    cand, _ = items()
    st = {n: a.astype(np.float32) for n, a in state(model).items()}
    f32 = np.float32
    with np.errstate(invalid="ignore"):
        s1 = np.zeros((NU, NC), f32)
        for f in range(K):
            s1 = s1 + st["P"][:, f][:, None] * st["Q"][cand][:, f][None, :]
        if "itemBias" in st:
            s1 = s1 + st["itemBias"][cand][None, :]
        rc = np.zeros((4, NU), f32) + f32(GM if model != "PQ" else 0.0)
        if "userBias" in st:
            rc = rc + st["userBias"][None, :]
        s2 = np.zeros((4, NC), f32) if "icBias" in st else None
        for c in range(4):
            for cond in CTX[c]:
                if "ucBias" in st:
                    rc[c] = rc[c] + st["ucBias"][:, cond]
                if s2 is not None:
                    s2[c] = s2[c] + st["icBias"][cand][:, cond]
    return s1, s2, rc


def pruning_bounds(model, queries, propagate_nan=False):
    """per query the fp32 bound (M1 + M2) + rc of every tile, as rank_topn_split_pruned forms it"""
    s1, s2, rc = split_parts(model)
    m1 = [tile_max(s1[u], propagate_nan) for u in range(NU)]
    m2 = [tile_max(s2[c], propagate_nan) for c in range(4)] if s2 is not None else None
    with np.errstate(invalid="ignore"):
        return [((m1[u] + m2[c]) if m2 is not None else m1[u]) + rc[c, u] for u, c, _, _ in queries]
