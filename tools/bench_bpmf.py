#!/usr/bin/env python3
"""BPMF on one GPU: the five stages of one iteration and the device's gaussian stream, one JSON line.

    tools/bench_bpmf.py [--rows K] [--out FILE]

Shapes: Frappe's 2-D pattern (957 users x 4 082 items) and the synthetic heavy-tailed matrix of tools/bench_knn.py (100 K users x 20 K
items, 5 M cells), each at k = 10 and k = 64.  Reported per shape: ms of the moments, the hyper steps (host, wall clock), the two user
passes, the two item passes and the loss of one iteration (cmi_bpmf_last_iter_ms; the best of two iterations after the first), and the
wall time of the device's nextGaussian() stream for one user pass's draws beside the sequential walk of tests/bpmf_ref.py's Stream
(Python, one core, timed on 20 000 draws and extrapolated).

Next to them the CPU restatement (tests/bpmf_ref.py) on one core: K sampled users of one user pass are restated from the same inputs
and the same draws, compared bit for bit with the device's rows, and extrapolated to the four passes of an iteration by the share of
the (entries x k^2 + k^3) steps they hold.  Every shape runs in a child process under its own time limit; a failing child ends the
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
    from tests import bpmf_ref as ref
    from tests import nmf_ref as nref
    shape, k, _ = SHAPES[name]
    nu, ni, u, i, r = frappe_cells() if shape == "frappe" else synthetic_cells()
    nnz = int(np.count_nonzero(r))
    rng = np.random.default_rng(6)
    P0, Q0 = rng.standard_normal((nu, k)), rng.standard_normal((ni, k))
    state0 = ref.random_state(20261222)
    h = capi.BPMFInstance(k, nu, ni)
    h.set_ratings(u, i, r)
    gm = h.global_mean()
    h.set_model(P0, Q0)
    h.set_stream(state0)
    # one user pass alone, for the rows the restatement is compared on
    rows = nref.rows_of(u, i, r, nu)
    slots = [a for a in range(nu) if len(rows[a][0])]
    b = rng.standard_normal((k, k)) * 0.1
    alpha, mu = b @ b.T + np.eye(k), rng.standard_normal(k) * 0.1
    t0 = time.perf_counter()
    Z, _ = capi.java_next_gaussians(state0, k * len(slots))
    gauss_wall_ms = (time.perf_counter() - t0) * 1e3
    flags, draws = h.sample_side(0, alpha, mu)
    P1 = h.model()[0]
    assert not flags.any() and draws == k * len(slots)
    pick = sorted(set(rng.choice(len(slots), min(n_rows, len(slots)), replace=False).tolist()))
    t0 = time.perf_counter()
    got = {}
    with np.errstate(all="ignore"):
        for s in pick:
            a = slots[s]
            mean, L = ref.row_posterior(Q0, list(zip(rows[a][0].tolist(), rows[a][1].tolist())), gm, alpha, mu)
            got[a] = ref.mult(L, Z[k * s:k * (s + 1)]) + mean
    sample_s = time.perf_counter() - t0
    for a, row in got.items():          # the timed rows are the device's rows, bit for bit
        assert row.tobytes() == P1[a].tobytes(), ("user", a)
    work = lambda n_entries: n_entries * k * k + k ** 3  # noqa: E731
    cols = nref.cols_of(u, i, r, ni)
    all_work = sum(work(len(rows[a][0])) for a in slots) + sum(work(len(c[0])) for c in cols if len(c[0]))
    cpu_iter_s = 2 * sample_s * all_work / max(sum(work(len(rows[slots[s]][0])) for s in pick), 1)
    # the host's sequential walk of the stream
    st = ref.Stream(state0)
    t0 = time.perf_counter()
    for _ in range(20000):
        st.gaussian()
    host_walk_ms = (time.perf_counter() - t0) * 1e3 * (k * len(slots)) / 20000
    # whole iterations
    h.set_model(P0, Q0)
    h.set_stream(state0)
    h.init_hyper()
    h.iterate()
    first = h.last_iter_ms()
    ms = []
    for _ in range(2):
        h.iterate()
        ms.append(h.last_iter_ms())
    best = min(ms, key=sum)
    h.close()
    return {"shape": name, "model": "BPMF", "users": nu, "items": ni, "cells": nnz, "k": k, "moments_ms": round(best[0], 3),
            "hyper_host_ms": round(best[1], 3), "user_passes_ms": round(best[2], 3), "item_passes_ms": round(best[3], 3),
            "loss_ms": round(best[4], 3), "iter_ms": round(sum(best), 3), "iter_ms_first": round(sum(first), 3), "iters_timed": 2,
            "gaussians_of_a_user_pass": k * len(slots), "device_gaussians_wall_ms": round(gauss_wall_ms, 3),
            "python_stream_walk_ms_extrapolated": round(host_walk_ms, 1), "cpu_restatement_rows": len(pick),
            "cpu_restatement_sample_s": round(sample_s, 3), "cpu_restatement_iter_s_extrapolated": round(cpu_iter_s, 1)}


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
    line = json.dumps({"bench": "bpmf", "runs": runs})
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    return 0 if all("error" not in r for r in runs) else 1


if __name__ == "__main__":
    sys.exit(main())
