#!/usr/bin/env python3
"""Mint tests/golden/reference_knn_rank.json.gz by EXECUTING the reference's ItemKNN / UserKNN with isRankingPred = true (no JVM:
oracle/jvm interprets the source, as tests/tools/mint_reference_knn.py does; its knn_matrix, run_knn pieces and JdkHashMap are imported).

Recommender.ranking(u, j, c) is predict(u, j, c, false) (Recommender.java:1016-1018).  Under isRankingPred the KNN models keep a
neighbour on `rate > 0` alone (ItemKNN.java:92-95, UserKNN.java:94-97): negative similarities enter the map, the knn cut and the sum,
and the neighbours are corrs.row(target).getIndex(), from which librec's SymmMatrix.row() leaves out the entries equal to zero.

* `models`: ItemKNN and UserKNN on the 26 x 42 knn_matrix of reference_knn.json.gz, PCC / shrinkage -1 and cos / shrinkage 30,
  predict(u, j, 0, false) for every (u, j) at knn in {0, 1, 5, 12, 1000}.
* `hand`: the same on a handmade 8 x 10 matrix (PCC / -1, knn in {0, 1, 2, 3}) in which, for either model, (a) a pair's similarity is
  exactly 0.0 while both vectors are non-empty, (b) a negative similarity survives a knn cut and (c) a negative similarity is cut; one
  witness of each is recorded, and so is a tuple whose score would differ had the zero similarity been kept.

Asserted here: (a)-(c) for both models; that the restatement (tests/knn_rank_ref.py) over the restated similarities reproduces every
handmade score bit for bit, so the witnesses are facts about the reference's run; that for either model on knn_matrix some (u, j)
differs, after the bound, from the rating-mode golden (the PCC runs do; cos of positive ratings is positive, so ranking mode keeps
what rating mode keeps and those runs pin the unbounded scores alone); and that no tuple treeifies a bin (JdkHashMap raises on one).

    python tests/tools/mint_reference_knn_rank.py /path/to/reference"""
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mint_reference_knn as base  # noqa: E402
from mint_reference_knn import JdkHashMap, hexd, knn_matrix  # noqa: E402
from oracle.jvm import interp, javasrc  # noqa: E402
from oracle.jvm.interp import VM  # noqa: E402
from tests import knn_rank_ref, knn_ref  # noqa: E402

KNNS = (0, 1, 5, 12, 1000)
HAND_KNNS = (0, 1, 2, 3)
RUNS = (("PCC", -1), ("cos", 30))


def hand_matrix():
    """8 users x 10 items, small integer ratings (PCC sums cancel exactly), user 7 and item 9 empty"""
    rng = np.random.default_rng(15)
    nu, ni = 8, 10
    cells = {}
    for u in range(nu - 1):
        for j in range(ni - 1):
            if rng.random() < 0.6:
                cells[(u, j)] = float(rng.integers(1, 6))
    return nu, ni, sorted((u, j, v) for (u, j), v in cells.items())


def run_knn_rank(ref, model, nu, ni, cells2, measure, shrinkage, knns, gm, with_corrs):
    """mint_reference_knn.run_knn with isRankingPred = true and the unbounded predict(u, j, 0, false)"""
    from oracle.mint_reference_src import CLASS_MAP, sparse
    javasrc.JHashMap = JdkHashMap   # `new HashMap<>()` in the interpreted predict(); raises on a bin it would treeify
    vm = VM([os.path.join(ref, "lib", "librec-v1.4-alpha.jar"), os.path.join(ref, "lib", "happy.coding.utils-1.2.6.jar")])
    src = [os.path.join(ref, "src", "carskit", "alg", "baseline", "cf", model + ".java"),
           os.path.join(ref, "src", "carskit", "generic", "Recommender.java")]
    this = javasrc.This(vm, src, dict(CLASS_MAP, Sims="happy/coding/math/Sims", Lists="happy/coding/io/Lists"))
    train2 = sparse(vm, nu, ni, cells2)
    this.fields.update({"train": None, "trainMatrix": None, "rateDao": base.TwoD(train2), "numUsers": nu, "numItems": ni, "globalMean": gm,
                        "knn": 0, "similarityMeasure": measure, "similarityShrinkage": shrinkage, "cf": base.Conf(shrinkage),
                        "isRankingPred": True, "isUserSplitting": False, "isItemSplitting": False, "isCARSRecommender": False,
                        "minRate": 1.0, "maxRate": 5.0, "algoName": model, "itemCorrs": None, "itemMeans": None,
                        "userCorrs": None, "userMeans": None})
    this.call("initModel", [])
    rec = {"model": model, "measure": measure, "shrinkage": shrinkage, "global_mean": hexd(gm), "ranking": {}}
    if with_corrs:
        corrs = this.fields["itemCorrs" if model == "ItemKNN" else "userCorrs"]
        means = this.fields["itemMeans" if model == "ItemKNN" else "userMeans"]
        n = ni if model == "ItemKNN" else nu
        rec["corrs"] = [hexd(vm.call("librec/data/SymmMatrix", "get", "(II)D", [corrs, a, b])) for a in range(n) for b in range(a + 1, n)]
        rec["means"] = [hexd(x) for x in interp.to_list(means.fields["data"])]
    for knn in knns:
        this.fields["knn"] = knn
        rec["ranking"][str(knn)] = [[hexd(this.call("predict", [u, j, 0, False])) for j in range(ni)] for u in range(nu)]
    return rec


def mean_of(cells2):
    gm = 0.0
    for _, _, v in cells2:
        gm += v
    return gm / len(cells2)


def hand_witnesses(rec, nu, ni, cells2, gm):
    """(a)-(c) on the handmade matrix, from the restated similarities once they and every score are the reference's bit for bit"""
    kind = "item" if rec["model"] == "ItemKNN" else "user"
    u = np.array([c[0] for c in cells2])
    i = np.array([c[1] for c in cells2])
    r = np.array([c[2] for c in cells2])
    rows = knn_ref.rows_of(u, i, r, kind, nu, ni)
    n = len(rows)
    S = knn_ref.build_corrs(rows, nu if kind == "item" else ni, rec["measure"], rec["shrinkage"])
    means = knn_ref.row_means(rows, gm)
    lists = knn_ref.lists_of(u, i, r, kind, nu, ni)
    java = [float.fromhex(x) for x in rec["corrs"]]  # SymmMatrix.get: 0.0 where nothing is stored
    mine = [float(np.nan_to_num(S[a, b], nan=0.0)) for a in range(n) for b in range(a + 1, n)]
    assert [x.hex() for x in java] == [x.hex() for x in mine], "the restated similarities are not the reference's"
    assert [hexd(x) for x in means] == rec["means"]

    def keep_zero(uu, jj, knn):  # the score had SymmMatrix.row() kept the zero entries
        owner, target = (uu, jj) if kind == "item" else (jj, uu)
        nns = knn_ref.JavaIntHashMap()
        for e, rate in lists[owner]:
            sim = float(S[target, e])
            if sim == sim and rate > 0:
                nns.put(e, sim)
        if 0 < knn < len(nns):
            srt = sorted(nns.items(), key=lambda kv: -kv[1])
            nns.clear()
            for k, v in srt[:knn]:
                nns.put(k, v)
        if len(nns) == 0:
            return gm
        rate_of = dict(lists[owner])
        s = ws = 0.0
        for e, sim in nns.items():
            s += sim * (rate_of[e] - float(means[e]))
            ws += abs(sim)
        return float(means[target]) + knn_ref._div(s, ws) if ws > 0 else gm

    wit = {"zero_pair": None, "negative_survives_cut": None, "negative_cut": None, "zero_kept_would_differ": None}
    for a in range(n):
        for b in range(a + 1, n):
            if S[a, b] == 0.0 and rows[a] and rows[b]:
                wit["zero_pair"] = [a, b]
    for uu in range(nu):
        for jj in range(ni):
            owner, target = (uu, jj) if kind == "item" else (jj, uu)
            kept = [(e, float(S[target, e])) for e, rate in lists[owner] if knn_rank_ref.keeps(float(S[target, e]), rate)]
            for knn in HAND_KNNS:
                got = knn_rank_ref.ranking(kind, S, means, lists, uu, jj, knn, gm)
                assert hexd(got) == rec["ranking"][str(knn)][uu][jj], (rec["model"], uu, jj, knn)
                if 0 < knn < len(kept):
                    srt = sorted(kept, key=lambda kv: -kv[1])
                    if any(v < 0 for _, v in srt[:knn]):
                        wit["negative_survives_cut"] = [uu, jj, knn]
                    if any(v < 0 for _, v in srt[knn:]):
                        wit["negative_cut"] = [uu, jj, knn]
                if keep_zero(uu, jj, knn) != got:
                    wit["zero_kept_would_differ"] = [uu, jj, knn]
    assert all(v is not None for v in wit.values()), (rec["model"], wit)
    return wit


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CARSKIT_REFERENCE", "")
    rating = json.loads(gzip.open(os.path.join(ROOT, "tests", "golden", "reference_knn.json.gz"), "rb").read())
    nu, ni, cells2 = knn_matrix()
    assert [[u, j, hexd(v)] for u, j, v in cells2] == rating["knn_matrix"]["cells"]
    gm = mean_of(cells2)
    models = []
    for model in ("ItemKNN", "UserKNN"):
        for measure, shrinkage in RUNS:
            rec = run_knn_rank(ref, model, nu, ni, cells2, measure, shrinkage, KNNS, gm, with_corrs=False)
            old = next(m for m in rating["models"] if (m["model"], m["measure"], m["shrinkage"]) == (model, measure, shrinkage))
            differs = 0
            for knn in KNNS:
                for u in range(nu):
                    for j in range(ni):
                        bounded = min(max(float.fromhex(rec["ranking"][str(knn)][u][j]), 1.0), 5.0)
                        differs += hexd(bounded) != old["predict"][str(knn)][u][j]
            rec["differs_from_rating_mode"] = differs  # (cos of positive ratings is positive: its runs pin the unbounded scores only)
            models.append(rec)
            print(model, measure, shrinkage, "differs at", differs, flush=True)
        per_model = sum(m["differs_from_rating_mode"] for m in models if m["model"] == model)
        assert per_model > 0, (model, "ranking mode equals rating mode everywhere: the file would pin nothing new")
    hnu, hni, hcells = hand_matrix()
    assert hnu <= 8 and hni <= 10
    hgm = mean_of(hcells)
    hand = []
    for model in ("ItemKNN", "UserKNN"):
        rec = run_knn_rank(ref, model, hnu, hni, hcells, "PCC", -1, HAND_KNNS, hgm, with_corrs=True)
        rec["witnesses"] = hand_witnesses(rec, hnu, hni, hcells, hgm)
        hand.append(rec)
        print("hand", model, rec["witnesses"], flush=True)
    out = {"source": "ItemKNN / UserKNN / Recommender from source with isRankingPred = true, predict(u, j, 0, false) "
                     "(tests/tools/mint_reference_knn_rank.py); the 26 x 42 matrix is knn_matrix of reference_knn.json.gz",
           "no_tuple_treeifies": True,  # JdkHashMap raises on a bin it would treeify: the runs above completed
           "models": models,
           "hand_matrix": {"n_users": hnu, "n_items": hni, "cells": [[u, j, hexd(v)] for u, j, v in hcells]}, "hand": hand}
    path = os.path.join(ROOT, "tests", "golden", "reference_knn_rank.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    size = os.path.getsize(path)
    assert size <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "reference_knn.json.gz")), size
    print("wrote", path, size, "bytes,", len(models), "+", len(hand), "model runs")


if __name__ == "__main__":
    main()
