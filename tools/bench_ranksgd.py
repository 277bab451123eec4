#!/usr/bin/env python3
"""RankSGD on one GPU: the stages of one iteration, one JSON line.

    tools/bench_ranksgd.py [--prefix N] [--out FILE]

Shapes: Frappe's 2-D matrix (957 users x 4 082 items; its counts mapped to 1 + log10(count), see one()) and the synthetic heavy-tailed one of tools/bench_knn.py (100 K users x 20 K
items, 5 M cells), each at k = 10 and k = 64, with CMI_RANKSGD_FLAG_NUM_RATES_SIZE: with the reference's own divisor (numRates is
never assigned there, so every draw returns the first item of the list) both matrices are refused, because the reference would not
end; the refusal's text is recorded.  An iteration visits every non-zero cell once.  Reported per shape, the best of two timed
iterations after the first: ms of the device tries (kernel and the copy of the items to the host), of the host walk that assigns them,
of the level build (host), of the epoch and of the loss (device events); the tries reserved and the tries the host had to supply past
them; the number of levels, of levels launched alone and of runs, and the widest level.  Next to them the same iteration on a handle
with CMI_RANKSGD_FLAG_HOST_SAMPLER (every try by the host), with the samples and the model compared.

The CPU restatement (tests/ranksgd_ref.py) on one core: its tries, walk and sequential update over the first users' cells (about N of
them) of the first iteration, the accepted items compared with the device's one by one, extrapolated to the whole iteration by the
share of cells.  Every shape runs in a child process under its own time limit; a failing child ends the benchmark."""
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
LR = 0.001


def one(name, prefix):
    from bench_knn import frappe_cells, synthetic_cells
    from carskit_amd import capi
    from tests import ranksgd_ref as rr
    shape, k, _ = SHAPES[name]
    nu, ni, u, i, r = frappe_cells() if shape == "frappe" else synthetic_cells()
    if shape == "frappe":
        # Frappe's values are usage counts up to 3 630: e = (pui - puj) - rui is then in the thousands and the iteration diverges to a
        # NaN loss at any usable learn rate (isConverged ends the reference's run as well).  The benchmark keeps the matrix's pattern
        # and maps the counts to 1 + log10(count), 1 .. 4.56, as tools/bench_lrmf.py does
        r = np.where(r > 0, 1.0 + np.log10(np.maximum(r, 1.0)), r)
    nnz = int(np.count_nonzero(r))
    rng = np.random.default_rng(7)
    P0, Q0 = 0.1 * rng.standard_normal((nu, k)), 0.1 * rng.standard_normal((ni, k))
    state = rr.random_state(1)
    SIZE = capi.RANKSGD_FLAG_NUM_RATES_SIZE
    refusal = None
    ref = capi.RankSGDInstance(k, nu, ni)
    try:
        ref.set_ratings(u, i, r)
    except capi.CmiError as e:
        refusal = str(e)[:160]
    ref.close()

    def run(flags):
        h = capi.RankSGDInstance(k, nu, ni, flags=flags)
        h.set_ratings(u, i, r)
        h.set_model(P0, Q0)
        h.set_random_state(state)
        first_samples = h.sample()
        h.iterate(LR)
        first = h.last_iter_ms()[:5]
        ms, sched = [], None
        for _ in range(2):
            h.iterate(LR)
            ms.append(h.last_iter_ms()[:5])
            sched = h.last_schedule()
        model = h.model()
        h.close()
        return first_samples, first, min(ms, key=sum), sched, model

    dev, first, best, sched, (P, Q) = run(SIZE)
    hdev, _, hbest, hsched, (hP, hQ) = run(SIZE | capi.RANKSGD_FLAG_HOST_SAMPLER)
    assert all(np.array_equal(a, b) for a, b in zip(dev[:4], hdev[:4])) and dev[4] == hdev[4]
    assert np.array_equal(P, hP) and np.array_equal(Q, hQ) and hsched["host_tries"] == 0
    out = {"shape": name, "model": "RankSGD", "num_rates": "size", "users": nu, "items": ni, "cells": nnz, "k": k,
           "reference_divisor_refused": refusal,
           "device_tries_ms": round(best[0], 3), "host_walk_ms": round(best[1], 3), "level_build_ms": round(best[2], 3),
           "epoch_ms": round(best[3], 3), "loss_ms": round(best[4], 3), "iter_ms": round(sum(best), 3),
           "iter_ms_first": round(sum(first), 3), "iters_timed": 2, "cells_per_s": nnz / (sum(best) * 1e-3),
           "levels": sched["levels"], "levels_alone": sched["alone"], "runs": sched["runs"], "widest_level": sched["widest"],
           "host_supplied_tries": sched["host_tries"],
           "host_sampler_tries_ms": round(hbest[0], 3), "host_sampler_walk_with_tries_ms": round(hbest[1], 3),
           "host_sampler_iter_ms": round(sum(hbest), 3)}
    # the restatement on one core over the first users' cells of the first iteration
    m = rr.RankSGD(nu, ni, zip(u.tolist(), i.tolist(), r.tolist()), rr.NUM_RATES_SIZE)
    users, n = 0, 0
    while users < nu and n < prefix:
        n += len(m.rows[users])
        users += 1
    rows, vals = m.rows, m.vals
    m.rows, m.vals = rows[:users], vals[:users]
    rnd = rr.JavaStream(state)
    t0 = time.perf_counter()
    tri, used = m.sample_iteration(rnd)
    t1 = time.perf_counter()
    assert len(tri) == n and [t[2] for t in tri] == dev[2][:n].tolist()
    Pl, Ql = P0.tolist(), Q0.tolist()
    t2 = time.perf_counter()
    rr.epoch(Pl, Ql, tri, LR)
    t3 = time.perf_counter()
    out.update({"cpu_restatement_prefix": n, "cpu_restatement_prefix_tries": used,
                "cpu_restatement_prefix_s": round((t1 - t0) + (t3 - t2), 3),
                "cpu_restatement_sampler_s_extrapolated": round((t1 - t0) * nnz / n, 2),
                "cpu_restatement_iter_s_extrapolated": round(((t1 - t0) + (t3 - t2)) * nnz / n, 1)})
    return out


def main():
    args = sys.argv[1:]
    prefix = int(args[args.index("--prefix") + 1]) if "--prefix" in args else 20000
    if "--one" in args:
        print(json.dumps(one(args[args.index("--one") + 1], prefix)))
        return 0
    runs = []
    for name, (_, _, limit) in SHAPES.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--one", name, "--prefix", str(prefix)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            runs.append({"shape": name, "error": "exit %d: %s" % (p.returncode, p.stderr.strip()[-400:])})
            break
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    line = json.dumps({"bench": "ranksgd", "runs": runs})
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    return 0 if all("error" not in r for r in runs) else 1


if __name__ == "__main__":
    sys.exit(main())
