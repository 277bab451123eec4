#!/usr/bin/env python3
"""ItemKNN / UserKNN on one GPU: similarity build and prediction, one JSON line.

    tools/bench_knn.py [--tuples N]

Shapes: Frappe's 2-D matrix (ItemKNN over its 4 082 items, UserKNN over its 957 users) and a synthetic heavy-tailed one (20 K items x
100 K users, 5 M cells; ItemKNN, so the contracted dimension spans 25 LDS tiles).  Reported per run: build ms (device events), pairs/s
(non-empty pairs a < b), an UPPER BOUND of the intersection steps/s (every pair charged the partner's whole length; the kernel skips
the tiles where the anchor has no entry and walks PCC's tiles twice), and prediction ms per 1 M tuples (knn = 20, PCC).  A last run
times predictions at the candidate limit: UserKNN where one item is rated by CMI_KNN_MAX_CANDIDATES users, ms per tuple of that item.  Every shape runs in a child process
under its own time limit; a failing child ends the benchmark."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMITS = {"frappe": 300, "synthetic": 900, "popular": 600}


def frappe_cells():
    import gzip
    import tempfile
    from carskit_amd import dao
    tmp = tempfile.mkdtemp()
    src = os.path.join(tmp, "frappe.csv")
    open(src, "wb").write(gzip.open(os.path.join(ROOT, "tests", "golden", "frappe_compact.csv.gz"), "rb").read())
    dao.transform(src, os.path.join(tmp, "train.csv"))
    d = dao.DataDAO(os.path.join(tmp, "train.csv")).rating_data()
    key = d.u.astype(np.int64) * d.n_items + d.j
    uk, inv = np.unique(key, return_inverse=True)
    s = np.zeros(len(uk))
    c = np.zeros(len(uk))
    np.add.at(s, inv, d.r)
    np.add.at(c, inv, 1.0)
    return d.n_users, d.n_items, (uk // d.n_items).astype(np.int32), (uk % d.n_items).astype(np.int32), s / c


def synthetic_cells(n_items=20_000, n_users=100_000, cells=5_000_000, seed=1):
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, n_items + 1) ** 0.8   # heavy-tailed item popularity
    it = rng.choice(n_items, size=int(cells * 1.1), p=w / w.sum())
    us = rng.integers(0, n_users, size=len(it))
    key = np.unique(us.astype(np.int64) * n_items + it)[:cells]
    r = rng.integers(1, 6, len(key)).astype(np.float64)
    return n_users, n_items, (key // n_items).astype(np.int32), (key % n_items).astype(np.int32), r


def popular(n_tuples):
    """UserKNN, 16 384 users who all rated item 0 (plus 20 random items of 2 000 each): the tuples (u, 0) have the longest candidate
    list cmi_knn_predict_batch accepts"""
    from carskit_amd import capi
    nu, ni = 16384, 2000
    rng = np.random.default_rng(3)
    key = np.unique(np.concatenate([np.arange(nu, dtype=np.int64) * ni,
                                    rng.integers(0, nu, 20 * nu).astype(np.int64) * ni + rng.integers(1, ni, 20 * nu)]))
    u, i = (key // ni).astype(np.int32), (key % ni).astype(np.int32)
    r = rng.integers(1, 6, len(key)).astype(np.float64)
    h = capi.KNNInstance("user", nu, ni)
    h.set_ratings(u, i, r)
    h.build("pcc", -1, 1.0, 5.0)
    n = min(n_tuples, 2000)
    tu = rng.integers(0, nu, n).astype(np.int32)
    tj = np.zeros(n, np.int32)
    h.predict(tu[:8], tj[:8], 20, 3.0)
    t0 = time.perf_counter()
    h.predict(tu, tj, 20, 3.0, True, 1.0, 5.0)
    dt = time.perf_counter() - t0
    return {"shape": "popular", "model": "UserKNN", "candidate_list": nu, "predict_tuples": n,
            "predict_ms_per_tuple_at_limit": round(dt * 1e3 / n, 4), "build_ms": round(h.last_build_ms(), 3)}


def one(shape, kind, n_tuples):
    from carskit_amd import capi
    if shape == "popular":
        return popular(n_tuples)
    nu, ni, u, i, r = frappe_cells() if shape == "frappe" else synthetic_cells()
    ent, ctr = (i, u) if kind == "item" else (u, i)
    n = ni if kind == "item" else nu
    deg = np.bincount(ent, minlength=n).astype(np.float64)
    ne = int((deg > 0).sum())
    pairs = ne * (ne - 1) // 2
    # partner walks: every pair (a < b) walks b's entries (at most its length): sum over b of deg[b] * (non-empty rows before b)
    before = np.cumsum(deg > 0) - (deg > 0)
    steps = float((deg * before).sum())
    h = capi.KNNInstance(kind, nu, ni)
    h.set_ratings(u, i, r)
    ms = []
    for _ in range(3 if shape == "frappe" else 1):    # the first Frappe build warms up; the synthetic one is built once
        h.build("pcc", -1, 1.0, 5.0)
        ms.append(h.last_build_ms())
    b_ms = min(ms[1:]) if len(ms) > 1 else ms[0]
    rng = np.random.default_rng(2)
    tu = rng.integers(0, nu, n_tuples).astype(np.int32)
    tj = rng.integers(0, ni, n_tuples).astype(np.int32)
    h.predict(tu[:1000], tj[:1000], 20, 3.0)
    t0 = time.perf_counter()
    h.predict(tu, tj, 20, 3.0, True, 1.0, 5.0)
    p_s = time.perf_counter() - t0
    return {"shape": shape, "model": "ItemKNN" if kind == "item" else "UserKNN", "rows": n, "cells": int(len(r)), "pairs": pairs,
            "build_ms": round(b_ms, 3), "pairs_per_s": pairs / (b_ms * 1e-3), "intersection_steps_per_s_upper_bound": steps / (b_ms * 1e-3),
            "predict_ms_per_1M_tuples": round(p_s * 1e3 * 1e6 / n_tuples, 3), "predict_tuples": n_tuples}


def main():
    args = sys.argv[1:]
    n_tuples = int(args[args.index("--tuples") + 1]) if "--tuples" in args else 200_000
    if "--one" in args:
        k = args.index("--one")
        print(json.dumps(one(args[k + 1], args[k + 2], n_tuples)))
        return 0
    runs = []
    for shape, kind in (("frappe", "item"), ("frappe", "user"), ("synthetic", "item"), ("popular", "user")):
        cmd = ["timeout", "-k", "10", str(LIMITS[shape]), sys.executable, os.path.abspath(__file__), "--one", shape, kind,
               "--tuples", str(n_tuples)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            runs.append({"shape": shape, "kind": kind, "error": "exit %d: %s" % (p.returncode, p.stderr.strip()[-400:])})
            break
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps({"bench": "knn", "runs": runs}))
    return 0 if all("error" not in r for r in runs) else 1


if __name__ == "__main__":
    sys.exit(main())
