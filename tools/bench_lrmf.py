#!/usr/bin/env python3
"""LRMF on one GPU: the stages of one iteration, one JSON line.

    tools/bench_lrmf.py [--budget N] [--out FILE]

Shapes: Frappe's 2-D matrix (957 users x 4 082 items; its counts mapped to 1 + log10(count), see one()) and the synthetic heavy-tailed one of tools/bench_knn.py (100 K users x 20 K
items, 5 M cells), each at k = 10 and k = 64, with the item rows of a unit in LDS and (CMI_LRMF_FLAG_GLOBAL_ROWS) in memory.  An
iteration visits every cell and recomputes the user's sum of n_u exps for each: sum n_u^2 inner products and exps.  Reported per run,
the best of the timed iterations after the first: ms of the epoch and of the loss (device events); the levels, the levels launched
alone, the runs of single-unit levels, the widest level, the units in the global form, the most users on one column (the lower bound
of the number of levels), the largest unit and sum n_u^2; for a shape of up to 2^22 loss terms, the loss as the reference's one chain
(CMI_LRMF_FLAG_STRICT) on a second handle.

The CPU restatement (tests/lrmf_ref.py) on one core: the units of level 1 depend on no other unit, so after the first iteration their
rows of P are the restatement's from the same start, compared bit for bit; their wall time, taken over as many of them as fit a budget
of inner products, is extrapolated to the whole iteration by the share of sum n_u^2.  Every run is a child process under its own time
limit; a failing child ends the benchmark."""
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
LR, REG = 0.01, 0.01


def one(name, form, budget):
    from bench_knn import frappe_cells, synthetic_cells
    from carskit_amd import capi
    from tests import lrmf_ref as lref
    from tests.util import same_bits_exact
    shape, k, _ = SHAPES[name]
    nu, ni, u, i, r = frappe_cells() if shape == "frappe" else synthetic_cells()
    if shape == "frappe":
        # Frappe's values are usage counts up to 3 630: Math.exp(r) overflows, userExp is Inf and the reference itself leaves in
        # iteration 1.  The benchmark keeps the matrix's pattern and maps the counts to 1 + log10(count), 1 .. 4.56
        r = 1.0 + np.log10(r)
    n = len(r)
    rng = np.random.default_rng(7)
    P0, Q0 = rng.random((nu, k)) / k, rng.random((ni, k))            # pred in [0, 1): a sum of n_u exps stays far from overflow
    flag = capi.LRMF_FLAG_GLOBAL_ROWS if form == "global" else 0
    h = capi.LRMFInstance(k, nu, ni, flags=flag)
    t0 = time.perf_counter()
    h.set_ratings(u, i, r)
    set_ms = (time.perf_counter() - t0) * 1e3
    h.set_model(P0, Q0)
    h.iterate(LR, REG, REG)
    first = h.last_iter_ms()[:2]
    P1, _ = h.model()
    ms = []
    for _ in range(2):
        h.iterate(LR, REG, REG)
        ms.append(h.last_iter_ms()[:2])
    best = min(ms, key=sum)
    sched = h.last_schedule()
    h.close()
    _, level_of, n_levels, chain = capi.lrmf_levels(nu, ni, u, i)
    n_u = np.bincount(u, minlength=nu).astype(np.int64)
    work = int(np.sum(n_u * n_u))
    out = {"shape": name, "form": form, "model": "LRMF", "users": nu, "items": ni, "cells": n, "stored_zeros": int(np.sum(r == 0.0)), "k": k,
           "epoch_ms": round(best[0], 3), "loss_ms": round(best[1], 3), "iter_ms": round(sum(best), 3), "iter_ms_first": round(sum(first), 3),
           "iters_timed": 2, "cells_per_s": n / (sum(best) * 1e-3), "inner_products": work, "inner_products_per_s": work / (best[0] * 1e-3),
           "set_ratings_wall_ms": round(set_ms, 1), "levels": sched["levels"], "levels_alone": sched["alone"], "runs": sched["runs"],
           "widest_level": sched["widest"], "global_units": sched["global_units"], "most_users_on_one_column": int(chain),
           "largest_unit": int(n_u.max()), "lds_rows": capi.lrmf_lds_rows(k), "us_per_level": round(best[0] * 1e3 / max(n_levels, 1), 2)}
    assert n_levels == sched["levels"]
    if form == "lds" and n * (k + 1) <= 1 << 22:   # what the reference's one-chain loss (CMI_LRMF_FLAG_STRICT) costs
        hs = capi.LRMFInstance(k, nu, ni, flags=capi.LRMF_FLAG_STRICT)
        hs.set_ratings(u, i, r)
        hs.set_model(P0, Q0)
        strict = []
        for _ in range(3):
            hs.iterate(LR, REG, REG)
            strict.append(hs.last_iter_ms()[1])
        hs.close()
        out.update({"loss_terms": n * (k + 1), "loss_ms_strict_chain": round(min(strict[1:]), 3)})
    if form == "lds":   # the restatement on one core over units of level 1
        users, w = [], 0
        for x in np.nonzero(level_of == 1)[0].tolist():
            if users and w + int(n_u[x]) ** 2 > budget:
                break
            users.append(x)
            w += int(n_u[x]) ** 2
        pick = np.isin(u, users)
        m = lref.LRMF(nu, ni, zip(u[pick].tolist(), i[pick].tolist(), r[pick].tolist()))
        P, Q = P0.tolist(), Q0.tolist()
        t0 = time.perf_counter()
        m.epoch(P, Q, LR, REG, REG)
        dt = time.perf_counter() - t0
        assert same_bits_exact(np.array([P[x] for x in users]), P1[users])
        out.update({"cpu_restatement_units": len(users), "cpu_restatement_inner_products": w, "cpu_restatement_s": round(dt, 3),
                    "cpu_restatement_iter_s_extrapolated": round(dt * work / w, 1), "level_1_units": int(np.sum(level_of == 1))})
    return out


def main():
    args = sys.argv[1:]
    budget = int(args[args.index("--budget") + 1]) if "--budget" in args else 100000
    if "--one" in args:
        p = args.index("--one")
        print(json.dumps(one(args[p + 1], args[p + 2], budget)))
        return 0
    runs = []
    for name, (_, _, limit) in SHAPES.items():
        for form in ("lds", "global"):
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--one", name, form, "--budget", str(budget)]
            p = subprocess.run(cmd, capture_output=True, text=True)
            if p.returncode != 0:
                runs.append({"shape": name, "form": form, "error": "exit %d: %s" % (p.returncode, p.stderr.strip()[-400:])})
                break
            runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
            print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
        if "error" in runs[-1]:
            break
    line = json.dumps({"bench": "lrmf", "runs": runs})
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    return 0 if all("error" not in r for r in runs) else 1


if __name__ == "__main__":
    sys.exit(main())
