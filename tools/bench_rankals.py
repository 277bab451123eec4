#!/usr/bin/env python3
"""RankALS on one GPU: the five phases of one iteration and its evaluation, one JSON line.

    tools/bench_rankals.py [--rows K] [--out FILE]

Shapes: Frappe's 2-D matrix (4 082 items x 957 users) and the synthetic heavy-tailed one of tools/bench_knn.py (20 K items x 100 K
users, 5 M cells), each at k = 10 and k = 64, `-sw on`.  Reported per shape: ms of the item moments, the user solves, the user moments
and the item solves (device events, the best of three iterations after the first), ms of the score fill and selection of one
evalRankings over a split of the cells (a query per test user scores every candidate item), and cells/s.

Next to them the CPU restatement (tests/rankals_ref.py, the hoisted form) on one core.  The sums every row needs (item moments, step
3's maps of all users, the user moments) are restated in full and timed as they are; K sampled users and K sampled items are solved
from them, compared bit for bit with the device's rows, and extrapolated to all users / items by the share of the
(entries x k^2 + k^3) steps they hold.  Every shape runs in a child process under its own time limit; a failing child ends the
benchmark."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = {"frappe_k10": ("frappe", 10, 300), "frappe_k64": ("frappe", 64, 300), "synthetic_k10": ("synthetic", 10, 900),
          "synthetic_k64": ("synthetic", 64, 900)}


def one(name, n_rows):
    from bench_knn import frappe_cells, synthetic_cells
    from carskit_amd import capi
    from tests import nmf_ref as nref
    from tests import rankals_ref as rref
    shape, k, _ = SHAPES[name]
    nu, ni, u, i, r = frappe_cells() if shape == "frappe" else synthetic_cells()
    nnz = int(np.count_nonzero(r))
    rng = np.random.default_rng(6)
    P0, Q0 = 0.1 * rng.standard_normal((nu, k)), 0.1 * rng.standard_normal((ni, k))
    h = capi.RankALSInstance(k, nu, ni)
    h.set_ratings(u, i, r)
    h.set_model(P0, Q0)
    h.iterate(True)
    first_ms = h.last_iter_ms()[:4]
    P1, Q1 = h.model()
    ms = []
    for _ in range(3):
        h.iterate(True)
        ms.append(h.last_iter_ms()[:4])
    best = min(ms, key=sum)
    it_ms = sum(best)
    out = {"shape": name, "model": "RankALS", "items": ni, "users": nu, "cells": nnz, "k": k, "support_weight": True,
           "item_moments_ms": round(best[0], 3), "user_solve_ms": round(best[1], 3), "user_moments_ms": round(best[2], 3),
           "item_solve_ms": round(best[3], 3), "iter_ms": round(it_ms, 3), "iter_ms_first": round(sum(first_ms), 3),
           "iters_timed": 3, "cells_per_s": nnz / (it_ms * 1e-3)}
    # the fifth phase, one evalRankings: every fifth cell is a test tuple in context 0, the others train; the second call is timed
    test = np.arange(len(r)) % 5 == 0
    z = np.zeros(len(r), np.int32)
    tup = lambda m: (u[m], i[m], z[m], np.where(r[m] != 0.0, r[m], 1.0))  # noqa: E731
    h.eval_rankings(tup(~test), tup(test), bin_thold=0.0, num_recs=10)
    t0 = time.perf_counter()
    h.eval_rankings(tup(~test), tup(test), bin_thold=0.0, num_recs=10)
    out["eval_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    out["score_and_select_ms"] = round(h.last_iter_ms()[4], 3)
    out["eval_queries"] = int(len(np.unique(u[test])))
    h.close()
    # the restatement on one core, from the model the device started from
    rows, cols = nref.rows_of(u, i, r, nu), nref.cols_of(u, i, r, ni)
    m = rref.from_csr(nu, ni, rows, cols, True)
    su = sorted(set(rng.choice(m.users, min(n_rows, len(m.users)), replace=False).tolist()))
    si = sorted(set(rng.integers(0, ni, n_rows).tolist()))
    t0 = time.perf_counter()
    sum_sq, sum_sqq = m.item_moments(Q0)
    sums = rref.UserSums(m, Q0, rows)
    t1 = time.perf_counter()
    with np.errstate(all="ignore"):
        pu = {a: m.solve_user(Q0, sum_sq, sum_sqq, a)[0] for a in su}
        t2 = time.perf_counter()
        mom = rref.user_moments_fast(m, P1, sums)     # the Q step reads the new P
        t3 = time.perf_counter()
        qi = {a: m.solve_item(P1, sums, sum_sq, mom, a) for a in si}
    t4 = time.perf_counter()
    for a in su:              # the timed rows are the device's rows, bit for bit
        assert pu[a].tobytes() == P1[a].tobytes(), ("user", a)
    for a in si:
        assert qi[a].tobytes() == Q1[a].tobytes(), ("item", a)
    work = lambda n_entries: n_entries * k * k + k ** 3  # noqa: E731
    user_all = sum(work(len(rows[a][0])) for a in m.users)
    item_all = sum(work(len(cols[a][0])) for a in range(ni))
    user_s = (t2 - t1) * user_all / max(sum(work(len(rows[a][0])) for a in su), 1)
    item_s = (t4 - t3) * item_all / max(sum(work(len(cols[a][0])) for a in si), 1)
    out.update({"longest_user": int(max(len(x[0]) for x in rows)), "longest_item": int(max(len(x[0]) for x in cols)),
                "cpu_restatement_rows": len(su) + len(si), "cpu_restatement_shared_sums_s": round((t1 - t0) + (t3 - t2), 3),
                "cpu_restatement_sample_s": round((t2 - t1) + (t4 - t3), 3),
                "cpu_restatement_iter_s_extrapolated": round((t1 - t0) + (t3 - t2) + user_s + item_s, 1)})
    return out


def main():
    args = sys.argv[1:]
    n_rows = int(args[args.index("--rows") + 1]) if "--rows" in args else 40
    if "--one" in args:
        print(json.dumps(one(args[args.index("--one") + 1], n_rows)))
        return 0
    runs = []
    for name, (_, _, limit) in SHAPES.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--one", name, "--rows", str(n_rows)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            runs.append({"shape": name, "error": "exit %d: %s" % (p.returncode, p.stderr.strip()[-400:])})
            break
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    line = json.dumps({"bench": "rankals", "runs": runs})
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    return 0 if all("error" not in r for r in runs) else 1


if __name__ == "__main__":
    sys.exit(main())
