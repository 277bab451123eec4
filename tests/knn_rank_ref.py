"""CPU restatement of ItemKNN / UserKNN.predict under isRankingPred (test infrastructure; never imported by carskit_amd/ or tools/).

Recommender.ranking(u, j, c) is predict(u, j, c, false) (Recommender.java:1016-1018): unbounded.  With isRankingPred the KNN models keep
a neighbour on `rate > 0` alone (ItemKNN.java:92-95, UserKNN.java:94-97), so negative similarities enter the map, the knn cut and the
weighted sum.  The neighbours come from corrs.row(target).getIndex(), and librec's SymmMatrix.row() leaves out the entries equal to
zero (+0.0 and -0.0), so over the dense matrix with NaN = unset the rule is

    keep iff sim == sim and sim != 0.0 and rate > 0

Everything after the filter is tests/knn_ref.py's predict(): the java.util.HashMap growth and treeify refusal, Lists.sortMap descending
and stable over the map's order, clear() keeping the table, the first knn put back, the sum in the final iteration order,
`ws > 0 ? mean[target] + sum / ws : globalMean`, and globalMean for an empty map."""
import numpy as np

from tests import knn_ref
from tests.knn_ref import JavaIntHashMap, Treeified  # noqa: F401  (Treeified: what ranking() raises)


def keeps(sim, rate):
    """the ranking-mode keep rule over the dense similarity matrix (NaN = unset)"""
    return sim == sim and sim != 0.0 and rate > 0


def ranking(kind, S, means, lists, u, j, knn, global_mean):
    """ItemKNN.predict(u, j) (kind "item": lists[u] = the user's (item, rating) cells) or UserKNN.predict(u, j) (kind "user":
    lists[j] = the item's (user, rating) cells) with isRankingPred set; S dense with NaN unset.  Raises Treeified."""
    owner, target = (u, j) if kind == "item" else (j, u)
    nns = JavaIntHashMap()
    for e, rate in lists[owner]:
        sim = float(S[target, e])
        if keeps(sim, rate):
            nns.put(e, sim)
    if 0 < knn < len(nns):
        srt = sorted(nns.items(), key=lambda kv: -kv[1])  # Lists.sortMap(nns, true): stable, descending by value
        nns.clear()
        for k, v in srt[:knn]:
            nns.put(k, v)
    if len(nns) == 0:
        return global_mean
    rate_of = dict(lists[owner])
    s = ws = 0.0
    for e, sim in nns.items():
        s += sim * (rate_of[e] - float(means[e]))
        ws += abs(sim)
    return float(means[target]) + knn_ref._div(s, ws) if ws > 0 else global_mean


def ranking_fast(kind, S, means, lists, u, j, knn, global_mean):
    """ranking() with the same contract and bits, vectorised as knn_ref.predict_fast is (its table growth and iteration order)"""
    owner, target = (u, j) if kind == "item" else (j, u)
    cells = np.asarray(lists[owner], dtype=np.float64).reshape(-1, 2)
    ids = cells[:, 0].astype(np.int64)
    rates = cells[:, 1]
    sims = np.asarray(S[target], dtype=np.float64)[ids]
    keep = (sims == sims) & (sims != 0.0) & (rates > 0)
    keys, sims, rates = ids[keep], sims[keep], rates[keep]
    m = len(keys)
    if m == 0:
        return global_mean
    cap, thr = knn_ref.hashmap_grow(keys)
    order = knn_ref._iteration_order(keys, cap)
    if 0 < knn < m:
        srt = order[np.argsort(-sims[order], kind="stable")][:knn]
        cap, thr = knn_ref.hashmap_grow(keys[srt], cap, thr)  # clear() keeps the table
        order = srt[knn_ref._iteration_order(keys[srt], cap)]
    s = ws = 0.0
    for t in order.tolist():
        sim = float(sims[t])
        s += sim * (float(rates[t]) - float(means[int(keys[t])]))
        ws += abs(sim)
    return float(means[target]) + knn_ref._div(s, ws) if ws > 0 else global_mean


def ranking_matrix(kind, S, means, lists, n_users, n_items, knn, global_mean, fast=False):
    """ranking(u, j) for every (u, j) as an (n_users, n_items) array"""
    f = ranking_fast if fast else ranking
    return np.array([[f(kind, S, means, lists, u, j, knn, global_mean) for j in range(n_items)] for u in range(n_users)])
