#!/usr/bin/env python3
"""SLIM on one GPU: the neighbour build, one iteration (sweep + loss chain) and one top-N evaluation, one JSON line.

    tools/bench_slim.py [--cols K] [--iters N] [--shapes NAME,NAME] [--out FILE]

Shapes: Frappe's 2-D matrix (4 082 items x 957 users) and the synthetic heavy-tailed one of tools/bench_knn.py (20 K items x 100 K
users, 5 M cells), each at knn = 10 and knn = 50 (cos, shrinkage 30; l1 = 0.1, l2 = 0.5; weights drawn in (0, 1)).  Reported per shape:
the similarity build (device events) and the whole cmi_slim_build_neighbors call (host clock: it holds the host-side cut), ms per
iteration (device events, best of three after the first), ms of one cmi_slim_eval_rankings (host clock around the call, best of three
after the first), and the step model of the sweep:

    steps per iteration = sum over columns j, coordinates i in nns(j), users u of column i:  len(nns(j)) - 1

one step being one neighbour looked up in one user's row (a binary search of about log2(row length) dependent loads from cache).  The
critical chain is the column with the largest share of it: its coordinates are walked one after the other by one wave, 64 users at a
time, so its time is about steps(j) / 64 lookups.

Next to them the CPU restatement on one core: K sampled columns restated here from the same weights with tests/slim_ref.py's
arithmetic (the contains() flags from tests/knn_ref.py), compared bit for bit with the device's columns, and extrapolated to one
iteration by the share of the steps they hold.  Every shape runs in a child process under its own time limit; a failing child ends
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

SHAPES = {"frappe_knn10": ("frappe", 10, 300), "frappe_knn50": ("frappe", 50, 300), "synthetic_knn10": ("synthetic", 10, 500),
          "synthetic_knn50": ("synthetic", 50, 800)}
L1, L2 = 0.1, 0.5


def restate_column(j, lst, w, rptr, ridx, rval, cptr, cidx, cval, found_of, l1, l2):
    """one column of SLIM.buildModel's loop body; returns the new weights.  This is tests/slim_ref.py's Slim.iterate written again over
    CSR arrays: the test class keeps a Python dict entry per cell, which 5 M cells do not allow here, so the time reported as the
    restatement's is the time of THIS copy; the bit-for-bit comparison of its columns with the device's is what ties it to the model"""
    w = w.copy()
    match = {}
    for t, i in enumerate(lst):
        grad = rate = errs = 0.0
        for q in range(cptr[i], cptr[i + 1]):
            u, rui = int(cidx[q]), float(cval[q])
            m = match.get(u)
            if m is None:
                r0, r1 = rptr[u], rptr[u + 1]
                items, found = ridx[r0:r1], found_of(u)
                pos = np.searchsorted(items, lst)
                m = [(s, float(rval[r0 + p])) for s, (p, k) in enumerate(zip(pos.tolist(), lst)) if p < len(items) and items[p] == k and found[p]]
                pj = int(np.searchsorted(items, j))
                match[u] = m = (m, float(rval[r0 + pj]) if pj < len(items) and items[pj] == j else 0.0)
            pred = 0.0
            for s, ruk in m[0]:
                if s != t:
                    pred += ruk * w[s]
            e = m[1] - pred
            grad += rui * e
            rate += rui * rui
            errs += e * e
        n = np.float64(cptr[i + 1] - cptr[i])
        with np.errstate(divide="ignore", invalid="ignore"):
            grad, rate = float(np.float64(grad) / n), float(np.float64(rate) / n)
            w[t] = float(np.float64(grad - l1 if grad > 0 else grad + l1) / np.float64(l2 + rate)) if l1 < abs(grad) else 0.0
    return w


def one(name, n_cols, n_iters=3):
    from bench_knn import frappe_cells, synthetic_cells
    from carskit_amd import capi
    from tests import knn_ref
    from tests.slim_ref import f32
    shape, knn, _ = SHAPES[name]
    nu, ni, u, i, r = frappe_cells() if shape == "frappe" else synthetic_cells()
    keep = r != 0.0
    u, i, r = u[keep], i[keep], r[keep]
    nnz = len(r)
    l1, l2 = f32(L1), f32(L2)
    h = capi.SLIMInstance(nu, ni)
    h.set_ratings(u, i, r)
    t0 = time.perf_counter()
    h.build_neighbors(knn, "cos", 30)
    build_call_s = time.perf_counter() - t0
    build_ms = h.last_build_ms()
    ptr, idx = h.neighbors()
    rng = np.random.default_rng(6)
    W0 = rng.random(len(idx))
    h.set_weights(W0)
    first_loss = h.iterate(l1, l2)
    first_ms = h.last_iter_ms()
    W1 = h.weights()
    ms, losses = [], [first_loss]
    for _ in range(n_iters):
        losses.append(h.iterate(l1, l2))
        ms.append(h.last_iter_ms())
    best = min(ms, key=sum)
    # one evaluation: every cell in one of three contexts, a fifth of them held out
    ctx = rng.integers(0, 3, nnz).astype(np.int32)
    held = rng.random(nnz) < 0.2
    train, test = (u[~held], i[~held], ctx[~held], r[~held]), (u[held], i[held], ctx[held], r[held])
    ev = []
    for _ in range(4):
        t0 = time.perf_counter()
        res = h.eval_rankings(train, test, bin_thold=-1.0, num_recs=10)
        ev.append((time.perf_counter() - t0) * 1e3)
    h.close()
    # the step model
    order_r, order_c = np.lexsort((i, u)), np.lexsort((u, i))
    rptr = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=nu))])
    cptr = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=ni))])
    ridx, rval, cidx, cval = i[order_r], r[order_r], u[order_c], r[order_c]
    col_len = np.diff(cptr)
    lens = np.diff(ptr)
    users = np.add.reduceat(np.concatenate([col_len[idx], [0]]), ptr[:-1])[:ni] * (lens > 0)   # per column: users over its coordinates
    steps = users * np.maximum(lens - 1, 0)
    crit = int(np.argmax(steps))
    # the restatement on one core: sampled columns from the weights the device started from
    found = {}

    def found_of(a):
        if a not in found:
            found[a] = knn_ref.findable([(int(k), 0.0) for k in ridx[rptr[a]:rptr[a + 1]]])
        return found[a]

    cand = np.nonzero((lens > 0) & (users < np.quantile(users[lens > 0], 0.9)))[0]
    sample = sorted(set(rng.choice(cand, min(n_cols, len(cand)), replace=False).tolist()))
    t0 = time.perf_counter()
    new = {j: restate_column(j, idx[ptr[j]:ptr[j + 1]].tolist(), W0[ptr[j]:ptr[j + 1]], rptr, ridx, rval, cptr, cidx, cval, found_of, l1, l2)
           for j in sample}
    cpu_s = time.perf_counter() - t0
    for j in sample:          # the timed columns are the device's columns, bit for bit
        assert new[j].tobytes() == W1[ptr[j]:ptr[j + 1]].tobytes(), ("column", j)
    share = float(steps[sample].sum()) / max(float(steps.sum()), 1.0)
    return {"shape": name, "model": "SLIM", "items": ni, "users": nu, "cells": nnz, "knn": knn, "list_entries": int(len(idx)),
            "build_similarity_ms": round(build_ms, 3), "build_neighbors_call_s": round(build_call_s, 3),
            "sweep_ms": round(best[0], 3), "loss_ms": round(best[1], 3), "iter_ms": round(sum(best), 3), "iter_ms_first": round(sum(first_ms), 3),
            "iter_ms_all": [round(sum(m), 3) for m in ms], "eval_ms": round(min(ev[1:]), 3), "eval_ms_first": round(ev[0], 3),
            "eval_ms_all": [round(x, 3) for x in ev[1:]], "eval_queries": res["n_queries"],
            "steps_per_iter": float(steps.sum()), "steps_per_s": float(steps.sum()) / (best[0] * 1e-3),
            "critical_column": crit, "critical_column_steps": float(steps[crit]), "critical_column_users": int(users[crit]),
            "critical_chain_ns_per_64_steps": round(best[0] * 1e6 / max(float(steps[crit]) / 64.0, 1.0), 2), "loss": losses,
            "longest_user": int(np.diff(rptr).max()), "longest_item": int(col_len.max()),
            "timed_iterations": n_iters, "cpu_restatement_columns": len(sample), "cpu_restatement_sample_s": round(cpu_s, 3), "cpu_restatement_step_share": share,
            "cpu_restatement_iter_s_extrapolated": round(cpu_s / max(share, 1e-30), 1)}


def main():
    args = sys.argv[1:]
    n_cols = int(args[args.index("--cols") + 1]) if "--cols" in args else 12
    n_iters = int(args[args.index("--iters") + 1]) if "--iters" in args else 3   # timed iterations after the first
    if "--one" in args:
        print(json.dumps(one(args[args.index("--one") + 1], n_cols, n_iters)))
        return 0
    runs = []
    names = args[args.index("--shapes") + 1].split(",") if "--shapes" in args else list(SHAPES)
    for name in names:
        limit = SHAPES[name][2]
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--one", name, "--cols", str(n_cols), "--iters", str(n_iters)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            runs.append({"shape": name, "error": "exit %d: %s" % (p.returncode, p.stderr.strip()[-400:])})
            break
        runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
        print(json.dumps(runs[-1]), file=sys.stderr, flush=True)
    line = json.dumps({"bench": "slim", "runs": runs})
    print(line)
    if "--out" in args:
        with open(args[args.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    return 0 if all("error" not in r for r in runs) else 1


if __name__ == "__main__":
    sys.exit(main())
