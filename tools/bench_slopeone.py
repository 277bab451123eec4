#!/usr/bin/env python3
"""SlopeOne on one GPU: deviation build and prediction, one JSON line.

    tools/bench_slopeone.py [--tuples N] [--anchors K]

Shapes: Frappe's 2-D matrix (4 082 items) and the synthetic heavy-tailed one of tools/bench_knn.py (20 K items x 100 K users, 5 M
cells, so an anchor column spans 25 LDS tiles).  Reported per shape: the build ms (device events, the zero-fill of the two n x n
matrices included), pairs/s (non-empty pairs a < b), prediction ms per 1 M tuples, and next to them (a) the CPU restatement on one
core, extrapolated from K sampled anchors (each anchor's partners b > a, by the walk over the anchor's users), and (b) the ItemKNN
`pcc` build on the same data in the same process.  Every shape runs in a child process under its own time limit; a failing child ends
the benchmark."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMITS = {"frappe": 300, "synthetic": 900}


def cpu_anchor(cols, rows, a):
    """the anchor's pairs (a, b > a) as the reference meets them: users of column a ascending, the user's items b > a; then the division
    and the mirror"""
    s, k = {}, {}
    for x, va in cols[a]:
        for b, vb in rows[x]:
            if b > a:
                s[b] = s.get(b, 0.0) + (va - vb)
                k[b] = k.get(b, 0) + 1
    return {b: (s[b] / k[b], 0.0 if s[b] == 0.0 else -(s[b] / k[b]), k[b]) for b in s}


def one(shape, n_tuples, n_anchors):
    from bench_knn import frappe_cells, synthetic_cells
    from carskit_amd import capi
    nu, ni, u, i, r = frappe_cells() if shape == "frappe" else synthetic_cells()
    deg = np.bincount(i, minlength=ni)
    ne = int((deg > 0).sum())
    pairs = ne * (ne - 1) // 2
    h = capi.SlopeOneInstance(nu, ni)
    h.set_ratings(u, i, r)
    ms = []
    for _ in range(3):            # the first build warms up
        h.build()
        ms.append(h.last_build_ms())
    b_ms = min(ms[1:])
    rng = np.random.default_rng(2)
    tu = rng.integers(0, nu, n_tuples).astype(np.int32)
    tj = rng.integers(0, ni, n_tuples).astype(np.int32)
    h.predict(tu[:1000], tj[:1000], 3.0)
    t0 = time.perf_counter()
    h.predict(tu, tj, 3.0, True, 1.0, 5.0)
    p_s = time.perf_counter() - t0
    # the sampled anchors' rows, for the CPU check below, before the matrices go
    anchors = sorted(set(np.random.default_rng(4).integers(0, ni - 1, n_anchors).tolist()))
    got = {a: h.deviation(a, 1) for a in anchors}
    h.close()
    # (b) the ItemKNN pcc build on the same cells
    kh = capi.KNNInstance("item", nu, ni)
    kh.set_ratings(u, i, r)
    kms = []
    for _ in range(3):
        kh.build("pcc", -1, 1.0, 5.0)
        kms.append(kh.last_build_ms())
    kh.close()
    # (a) the restatement on one core: K anchors, extrapolated by the share of the walk's steps they hold
    ro = np.lexsort((i, u))
    udeg = np.bincount(u, minlength=nu)
    rptr = np.concatenate([[0], np.cumsum(udeg)])
    ri, rv = i[ro], r[ro]
    co = np.lexsort((u, i))
    cptr = np.concatenate([[0], np.cumsum(deg)])
    cu, cv = u[co], r[co]
    cols = {a: list(zip(cu[cptr[a]:cptr[a + 1]].tolist(), cv[cptr[a]:cptr[a + 1]].tolist())) for a in anchors}
    rows = {x: list(zip(ri[rptr[x]:rptr[x + 1]].tolist(), rv[rptr[x]:rptr[x + 1]].tolist())) for a in anchors for x, _ in cols[a]}
    t0 = time.perf_counter()
    want = {a: cpu_anchor(cols, rows, a) for a in anchors}
    cpu_s = time.perf_counter() - t0
    for a in anchors:             # the timed rows are the device's rows, bit for bit
        d, c = got[a]
        for b, (dab, _, k) in want[a].items():
            assert float(d[0, b]).hex() == float(dab).hex() and c[0, b] == k, (a, b)
        assert int((c[0, a + 1:] > 0).sum()) == len(want[a]), a
    # steps of the whole build by that walk: every cell (x, a) meets the user's items above a
    steps_all = float((udeg[u[ro]] - 1 - (np.arange(len(r)) - rptr[u[ro]])).sum())
    steps_sample = float(sum(sum(1 for b, _ in rows[x] if b > a) for a in anchors for x, _ in cols[a]))
    cpu_full_s = cpu_s * steps_all / max(steps_sample, 1.0)
    return {"shape": shape, "model": "SlopeOne", "items": ni, "users": nu, "cells": int(len(r)), "pairs": pairs,
            "build_ms": round(b_ms, 3), "build_ms_first": round(ms[0], 3), "pairs_per_s": pairs / (b_ms * 1e-3),
            "predict_ms_per_1M_tuples": round(p_s * 1e3 * 1e6 / n_tuples, 3), "predict_tuples": n_tuples,
            "itemknn_pcc_build_ms": round(min(kms[1:]), 3), "build_vs_itemknn_pcc": round(b_ms / min(kms[1:]), 3),
            "cpu_restatement_anchors": len(anchors), "cpu_restatement_sample_s": round(cpu_s, 3),
            "cpu_restatement_build_s_extrapolated": round(cpu_full_s, 1), "pair_steps": steps_all}


def main():
    args = sys.argv[1:]
    n_tuples = int(args[args.index("--tuples") + 1]) if "--tuples" in args else 200_000
    n_anchors = int(args[args.index("--anchors") + 1]) if "--anchors" in args else 40
    if "--one" in args:
        print(json.dumps(one(args[args.index("--one") + 1], n_tuples, n_anchors)))
        return 0
    runs = []
    for shape in ("frappe", "synthetic"):
        cmd = ["timeout", "-k", "10", str(LIMITS[shape]), sys.executable, os.path.abspath(__file__), "--one", shape,
               "--tuples", str(n_tuples), "--anchors", str(n_anchors)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            runs.append({"shape": shape, "error": "exit %d: %s" % (p.returncode, p.stderr.strip()[-400:])})
            break
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    print(json.dumps({"bench": "slopeone", "runs": runs}))
    return 0 if all("error" not in r for r in runs) else 1


if __name__ == "__main__":
    sys.exit(main())
