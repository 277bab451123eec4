#!/usr/bin/env python3
"""NMF on one GPU: the W phase, the H phase and the loss of one iteration, one JSON line.

    tools/bench_nmf.py [--rows K] [--out FILE]

Shapes: Frappe's 2-D matrix (4 082 items x 957 users) at k = 10, and the synthetic heavy-tailed one of tools/bench_knn.py (20 K items x
100 K users, 5 M cells) at k = 10 and k = 128.  Reported per shape: ms per phase and per iteration (device events, best of three
iterations after the first), cells/s, and the fraction of the device's measured copy rate (cmi_measure_hbm) that the iteration's bytes
amount to under this model:

    bytes per iteration = 2 * nnz * (8 k + 12)  +  nnz * (16 k + 12)

the two update phases gather one partner k-row of doubles per cell plus the cell's index and value (the second, coalesced read of the
row comes from the cache the first filled; the own row is k doubles a ROW, not a cell, and left out), and the loss reads both k-rows
per cell plus index and value.  Rows that stay in a cache make the real traffic smaller, so the fraction is a statement about the
model, not a measured bandwidth.

Next to them the CPU restatement (tests/nmf_ref.py) on one core: K sampled users and K sampled items restated from the same model,
compared bit for bit with the device's rows, and extrapolated to one iteration by the share of the (entries x k) steps they hold.
Every shape runs in a child process under its own time limit; a failing child ends the benchmark."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = {"frappe_k10": ("frappe", 10, 300), "synthetic_k10": ("synthetic", 10, 600), "synthetic_k128": ("synthetic", 128, 900)}


def one(name, n_rows):
    from bench_knn import frappe_cells, synthetic_cells
    from carskit_amd import capi
    from tests import nmf_ref as nref
    shape, k, _ = SHAPES[name]
    nu, ni, u, i, r = frappe_cells() if shape == "frappe" else synthetic_cells()
    nnz = int(np.count_nonzero(r))
    rng = np.random.default_rng(6)
    W0, H0 = 0.01 * rng.random((nu, k)), 0.01 * rng.random((k, ni))
    copy_gbs, _ = capi.measure_hbm(0, 2 << 30)
    h = capi.NMFInstance(k, nu, ni)
    h.set_ratings(u, i, r)
    h.set_model(W0, H0)
    first_loss = h.iterate()
    first_ms = h.last_iter_ms()
    W1, H1 = h.model()
    ms, losses = [], [first_loss]
    for _ in range(3):
        losses.append(h.iterate())
        ms.append(h.last_iter_ms())
    h.close()
    best = min(ms, key=sum)
    it_ms = sum(best)
    model_bytes = 2 * nnz * (8 * k + 12) + nnz * (16 * k + 12)
    # the restatement on one core: sampled rows of either phase from the model the device started from
    rows, cols = nref.rows_of(u, i, r, nu), nref.cols_of(u, i, r, ni)
    Ht0 = np.ascontiguousarray(H0.T)
    su = sorted(set(rng.integers(0, nu, n_rows).tolist()))
    si = sorted(set(rng.integers(0, ni, n_rows).tolist()))
    t0 = time.perf_counter()
    wu = {a: nref.update_row(W0[a], Ht0, *rows[a]) for a in su}
    wi = {a: nref.update_row(Ht0[a], W1, *cols[a]) for a in si}    # the H phase reads the new W
    cpu_s = time.perf_counter() - t0
    for a in su:              # the timed rows are the device's rows, bit for bit
        assert wu[a].tobytes() == W1[a].tobytes(), ("user", a)
    for a in si:
        assert wi[a].tobytes() == np.ascontiguousarray(H1[:, a]).tobytes(), ("item", a)
    sample = sum(len(rows[a][0]) for a in su) + sum(len(cols[a][0]) for a in si)
    cpu_full_s = cpu_s * (2.0 * nnz) / max(sample, 1)
    return {"shape": name, "model": "NMF", "items": ni, "users": nu, "cells": nnz, "k": k,
            "w_phase_ms": round(best[0], 3), "h_phase_ms": round(best[1], 3), "loss_ms": round(best[2], 3), "iter_ms": round(it_ms, 3),
            "iter_ms_first": round(sum(first_ms), 3), "cells_per_s": nnz / (it_ms * 1e-3), "model_bytes_per_iter": model_bytes,
            "model_gb_per_s": round(model_bytes / (it_ms * 1e-3) / 1e9, 1), "hbm_copy_gb_per_s": round(copy_gbs, 1),
            "fraction_of_hbm_copy": round(model_bytes / (it_ms * 1e-3) / 1e9 / copy_gbs, 4), "loss": losses,
            "longest_user": int(max(len(x[0]) for x in rows)), "longest_item": int(max(len(x[0]) for x in cols)),
            "cpu_restatement_rows": len(su) + len(si), "cpu_restatement_sample_s": round(cpu_s, 3),
            "cpu_restatement_update_phases_s_extrapolated": round(cpu_full_s, 1)}


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
    line = json.dumps({"bench": "nmf", "runs": runs})
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    return 0 if all("error" not in r for r in runs) else 1


if __name__ == "__main__":
    sys.exit(main())
