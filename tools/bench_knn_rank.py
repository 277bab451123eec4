#!/usr/bin/env python3
"""Top-N evaluation of ItemKNN / UserKNN (knn = 20, PCC) and SlopeOne on one GPU, one JSON line.

    tools/bench_knn_rank.py [--users N] [--runs R] [--cpu-users K]

Shapes: Frappe's pattern (957 users x 4 082 items; every user with a cell is a query user) and the synthetic 20 K items x 100 K users,
5 M cells of tools/bench_knn.py, where a stated sample of N query users (default 512) is evaluated against all candidates.  UserKNN is
not run on the synthetic shape: its 100 K x 100 K similarity matrix alone is 80 GB.  The evaluation's tuples are the 2-D cells in one
context (the training side: candidates and exclusions) and one test tuple per query user.

Per shape and model, R >= 3 runs (default 5) after a warm-up, alternating the two device forms; medians and the spread (max - min):
* `eval`: one eval_rankings call: wall ms (host clock around the call, which ends synchronised) and the device's scoring + selection ms
  (last_rank_ms, by events).
* baseline A, the composition the per-tuple entry points allow: ranking() (KNN) or predict() (SlopeOne) over every (query user,
  candidate) tuple, then the selection on the host (numpy: mask the exclusions, argpartition, sort): wall ms, and the device call alone.
  Its lists must equal the evaluation's.
* baseline B: a numpy restatement on one core over K sampled query users (default 2) and all candidates, extrapolated by the share of
  tuples.  It iterates a HashMap of the final capacity (it does not model treeifyBin's resizes of small tables), so it is held to the
  device within 1e-9, not bit for bit; the bit-exact restatements are tests/knn_rank_ref.py and tests/slopeone_ref.py.
Every (shape, model) runs in a child process under its own time limit; a failing child ends the benchmark."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KNN, GM, TOPN, THOLD = 20, 3.0, 10, -1.0
CASES = (("frappe", "item"), ("frappe", "user"), ("frappe", "slope"), ("synthetic", "item"), ("synthetic", "slope"))
LIMITS = {"frappe": 300, "synthetic": 600}


def stats(xs):
    return {"median": round(float(np.median(xs)), 3), "spread": round(float(max(xs) - min(xs)), 3), "runs": len(xs)}


def cpu_knn(kind, S_rows, means, lists, u, j):
    """ranking(u, j) at KNN on one core; S_rows: {target: its row of S, or the columns of it that the lists' `loc` index}"""
    owner, target = (u, j) if kind == "item" else (j, u)
    ids, rates, loc = lists[owner]
    sims = S_rows[target][loc]
    keep = (sims == sims) & (sims != 0.0) & (rates > 0)
    ids, rates, sims = ids[keep], rates[keep], sims[keep]
    m = len(ids)
    if m == 0:
        return GM
    cap = 16
    while m > cap * 3 // 4:
        cap *= 2
    hsh = (ids ^ (ids >> 16)) & (cap - 1)
    order = np.lexsort((np.arange(m), hsh))
    if KNN < m:
        srt = order[np.argsort(-sims[order], kind="stable")][:KNN]
        order = srt[np.lexsort((np.arange(KNN), hsh[srt]))]
    s = ws = 0.0
    for t in order.tolist():
        s += float(sims[t]) * (float(rates[t]) - float(means[ids[t]]))
        ws += abs(float(sims[t]))
    return float(means[target]) + s / ws if ws > 0 else GM


def cpu_slope(dev_rows, card_rows, lists, u, j):
    ids, rates, loc = lists[u]
    c = card_rows[j][loc].astype(np.float64)
    ok = (ids != j) & (c > 0)
    if not ok.any():
        return GM
    return float(np.cumsum(((dev_rows[j][loc] + rates) * c)[ok])[-1] / np.cumsum(c[ok])[-1])


def host_select(scores, users, cand, excl):
    """{user: [(item, score), ...]}: the candidates not excluded, by descending score, ties in candidate order, the first TOPN"""
    out = {}
    for q, u in enumerate(users.tolist()):
        row = scores[q].copy()
        row[excl[u]] = -np.inf
        row[~(row > THOLD)] = -np.inf                         # Recommender.evalRankings keeps the scores above binThold
        top = np.argpartition(-row, TOPN)[:TOPN] if len(row) > TOPN else np.arange(len(row))
        kth = row[top].min()
        top = np.nonzero(row >= kth)[0]                       # every tie of the last place, then a stable sort
        top = top[np.argsort(-row[top], kind="stable")][:TOPN]
        out[int(u)] = [(int(cand[p]), float(row[p])) for p in top if row[p] > -np.inf]
    return out


def one(shape, model, n_users_sample, n_runs, n_cpu_users):
    from bench_knn import frappe_cells, synthetic_cells
    from carskit_amd import capi
    nu, ni, u, i, r = frappe_cells() if shape == "frappe" else synthetic_cells()
    rng = np.random.default_rng(11)
    have = np.unique(u)
    users = have if shape == "frappe" else np.sort(rng.choice(have, n_users_sample, replace=False))
    users = users.astype(np.int32)
    ctx0 = np.zeros(len(u), np.int32)
    train = (u, i, ctx0, r)
    cand = np.array(capi.rank_plan(nu, ni, train, (users[:1], i[:1], ctx0[:1], r[:1]), -1.0, 0)[0], np.int32)
    pos_of = np.full(ni, -1, np.int64)
    pos_of[cand] = np.arange(len(cand))
    test_items = cand[rng.integers(0, len(cand), len(users))]
    test = (users, test_items, np.zeros(len(users), np.int32), np.full(len(users), 5.0))
    ro = np.lexsort((i, u))
    rptr = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=nu))])
    i_ro, r_ro = i[ro].astype(np.int64), r[ro]
    excl = {int(a): pos_of[i_ro[rptr[a]:rptr[a + 1]]] for a in users.tolist()}

    if model == "slope":
        h = capi.SlopeOneInstance(nu, ni)
        h.set_ratings(u, i, r)
        h.build()
        ev = lambda: h.eval_rankings(train, test, GM, bin_thold=THOLD, num_recs=TOPN, with_lists=True)  # noqa: E731
        per_tuple = lambda a, b: h.predict(a, b, GM)  # noqa: E731
    else:
        h = capi.KNNInstance(model, nu, ni)
        h.set_ratings(u, i, r)
        h.build("pcc", -1, 1.0, 5.0)
        ev = lambda: h.eval_rankings(train, test, KNN, GM, bin_thold=THOLD, num_recs=TOPN, with_lists=True)  # noqa: E731
        per_tuple = lambda a, b: h.ranking(a, b, KNN, GM)  # noqa: E731
    tu = np.repeat(users, len(cand))
    tj = np.tile(cand, len(users))

    def baseline_a():
        t0 = time.perf_counter()
        sc = per_tuple(tu, tj).reshape(len(users), len(cand))
        t1 = time.perf_counter()
        return host_select(sc, users, cand, excl), (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3, sc

    _, lists = ev()                                          # warm-up of both forms
    a_lists, _, _, scores = baseline_a()
    got = {k[0]: v for k, v in lists.items()}
    assert len(got) > 0 and all(got[k] == a_lists[k] for k in got), "baseline A's lists are not the evaluation's"
    wall, dev_ms, a_wall, a_dev = [], [], [], []
    for _ in range(n_runs):                                  # alternating
        t0 = time.perf_counter()
        ev()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(h.last_rank_ms())
        _, d, w, _ = baseline_a()
        a_dev.append(d)
        a_wall.append(w)

    # baseline B: the restatement on one core over sampled query users, all candidates
    co = np.lexsort((u, i))
    cptr = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=ni))])
    u_co, r_co = u[co].astype(np.int64), r[co]
    sample = rng.choice(len(users), min(n_cpu_users, len(users)), replace=False).tolist()
    # the items of the sampled users: the only columns of a candidate's row (of S, or of dev and card) that their scores read
    union = np.unique(np.concatenate([i_ro[rptr[users[q]]:rptr[users[q] + 1]] for q in sample] + [np.zeros(0, np.int64)]))
    rows_u = lambda a: (i_ro[rptr[a]:rptr[a + 1]], r_ro[rptr[a]:rptr[a + 1]], np.searchsorted(union, i_ro[rptr[a]:rptr[a + 1]]))  # noqa: E731
    cols_i = lambda b: (u_co[cptr[b]:cptr[b + 1]], r_co[cptr[b]:cptr[b + 1]], u_co[cptr[b]:cptr[b + 1]])  # noqa: E731
    if model == "slope":
        dev_rows, card_rows = {}, {}
        for b0 in range(0, ni, 2048):                         # every candidate's rows of dev and card
            d, c = h.deviation(b0, min(2048, ni - b0))
            for b in cand[(cand >= b0) & (cand < b0 + 2048)].tolist():
                dev_rows[b], card_rows[b] = d[b - b0][union], c[b - b0][union]
        lists_b = {int(users[q]): rows_u(int(users[q])) for q in sample}
        fn = lambda a, b: cpu_slope(dev_rows, card_rows, lists_b, a, b)  # noqa: E731
    else:
        n_ent = ni if model == "item" else nu
        vals, ptr = (r_co, cptr) if model == "item" else (r_ro, rptr)
        means = np.full(n_ent, GM)
        for e in np.nonzero(np.diff(ptr))[0].tolist():        # SparseVector.mean(): the sum in index order / count
            means[e] = np.cumsum(vals[ptr[e]:ptr[e + 1]])[-1] / (ptr[e + 1] - ptr[e])
        if model == "item":
            S_rows = {}
            for b0 in range(0, ni, 2048):
                blk = h.similarity(b0, min(2048, ni - b0))
                for b in cand[(cand >= b0) & (cand < b0 + 2048)].tolist():
                    S_rows[b] = blk[b - b0][union]
            lists_b = {int(users[q]): rows_u(int(users[q])) for q in sample}
        else:
            S_rows = {int(users[q]): h.similarity(int(users[q]), 1)[0] for q in sample}
            lists_b = {int(b): cols_i(int(b)) for b in cand.tolist()}
        fn = lambda a, b: cpu_knn(model, S_rows, means, lists_b, a, b)  # noqa: E731
    t0 = time.perf_counter()
    want = np.array([[fn(int(users[q]), int(b)) for b in cand.tolist()] for q in sample])
    cpu_s = time.perf_counter() - t0
    assert np.allclose(want, scores[sample], rtol=1e-9, atol=1e-9, equal_nan=True), "the timed restatement is not the device's computation"
    h.close()
    n_tuples = len(users) * len(cand)
    return {"shape": shape, "model": {"item": "ItemKNN", "user": "UserKNN", "slope": "SlopeOne"}[model], "knn": None if model == "slope" else KNN,
            "users": nu, "items": ni, "cells": int(len(r)), "query_users": int(len(users)), "query_users_sampled": shape != "frappe",
            "candidates": int(len(cand)), "tuples": int(n_tuples), "top_n": TOPN,
            "eval_wall_ms": stats(wall), "eval_score_select_ms": stats(dev_ms),
            "baseline_a_wall_ms": stats(a_wall), "baseline_a_device_call_ms": stats(a_dev),
            "eval_beats_a_beyond_a_spread": bool(np.median(wall) + (max(a_wall) - min(a_wall)) < np.median(a_wall)),
            "baseline_b_cpu_users": len(sample), "baseline_b_sample_s": round(cpu_s, 3),
            "baseline_b_s_extrapolated": round(cpu_s * len(users) / len(sample), 1)}


def main():
    args = sys.argv[1:]
    opt = lambda name, dflt: int(args[args.index(name) + 1]) if name in args else dflt  # noqa: E731
    n_users, n_runs, n_cpu = opt("--users", 512), max(3, opt("--runs", 5)), opt("--cpu-users", 2)
    if "--one" in args:
        k = args.index("--one")
        print(json.dumps(one(args[k + 1], args[k + 2], n_users, n_runs, n_cpu)))
        return 0
    runs = []
    for shape, model in CASES:
        cmd = ["timeout", "-k", "10", str(LIMITS[shape]), sys.executable, os.path.abspath(__file__), "--one", shape, model,
               "--users", str(n_users), "--runs", str(n_runs), "--cpu-users", str(n_cpu)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            runs.append({"shape": shape, "model": model, "error": "exit %d: %s" % (p.returncode, p.stderr.strip()[-600:])})
            break
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps({"bench": "knn_rank", "runs": runs}))
    return 0 if all("error" not in r for r in runs) else 1


if __name__ == "__main__":
    sys.exit(main())
