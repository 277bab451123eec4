#!/usr/bin/env python3
"""CPTF on one GPU, measured once: the epoch's cost per entry (the one-wave chain), the loss sum, prediction of 1 M key tuples and one
top-N evaluation, at k = 10 and k = 64 with the context rows in LDS and in memory, on two shapes:

  * frappe_pattern: the sizes of the Frappe set (957 users, 4082 items, 96203 entries, 8 context dimensions of 7, 7, 2, 3, 2, 9, 80 and
    233 conditions) with drawn keys;
  * synthetic: 100 K users x 20 K items, 5 M entries, 3 context dimensions of 5 conditions.

The comparison is tests/cptf_ref.py's epoch (numpy, one core) over a prefix of the entries whose rows equal the device's strict run bit
for bit, EXTRAPOLATED to the whole stream.  A compiled one-core loop was not timed; by arithmetic (a link is one division and about 6 more
floating-point operations per factor and dimension) it is probably faster than the one-wave chain at k = 10 and slower at k = 64.

    python tools/bench_cptf.py [--out profiles/cptf_bench.json] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from carskit_amd import capi  # noqa: E402
from tests import cptf_ref as cref  # noqa: E402

LRATE, REG = 0.001, 0.01
PREFIX = 2000

SHAPES = {"frappe_pattern": ([957, 4082, 7, 7, 2, 3, 2, 9, 80, 233], 96203),
          "synthetic": ([100000, 20000, 5, 5, 5], 5000000)}


def draw(dims, n, k, seed):
    rng = np.random.default_rng(seed)
    keys = np.stack([rng.integers(0, d, n) for d in dims], axis=1).astype(np.int32)
    r = rng.integers(1, 6, n).astype(np.float64)
    scale = (3.0 / k) ** (1.0 / len(dims))
    M = [scale * (1.0 + 0.1 * rng.standard_normal((d, k))) for d in dims]
    return keys, r, M


def bench_shape(name, dims, n, k):
    keys, r, M = draw(dims, n, k, 1)
    out = {"shape": name, "dims": dims, "entries": n, "k": k, "ctx_bytes": sum(dims[2:]) * k * 8, "forms": {}}
    for form, flag in (("lds", 0), ("global", capi.CPTF_FLAG_GLOBAL_CTX)):
        h = capi.CPTFInstance(k, dims, flags=flag)
        h.set_entries(keys, r)
        h.set_model(M)
        try:
            loss = h.iterate(LRATE, REG)
        except capi.CmiError as e:
            loss = e.loss
        ms = h.last_iter_ms()
        in_lds = h.ctx_in_lds()
        h.close()
        if form == "lds" and not in_lds:
            out["forms"][form] = "the context rows do not fit the LDS budget: not run"
            continue
        out["forms"][form] = {"epoch_ms": ms[0], "us_per_entry": 1e3 * ms[0] / n, "loss_ms": ms[1], "loss": loss}
    # prediction of 1 M tuples (host wall time of the call: upload, kernel, copy back) and one top-N evaluation (device loop, events)
    h = capi.CPTFInstance(k, dims)
    h.set_model(M)
    pk = keys[np.random.default_rng(2).integers(0, n, 1000000)]
    h.predict(pk[:1000])
    t0 = time.perf_counter()
    h.predict(pk)
    out["predict_1m_wall_ms"] = 1e3 * (time.perf_counter() - t0)
    n_ctx = 64
    rng = np.random.default_rng(3)
    ctx_keys = np.stack([rng.integers(0, d, n_ctx) for d in dims[2:]], axis=1)
    h.set_context_keys(ctx_keys)
    h.set_rating_range(1.0, 5.0)
    nt = min(n, 50000)
    tup = np.unique(np.stack([keys[:nt, 0], keys[:nt, 1], rng.integers(0, n_ctx, nt).astype(np.int32)], axis=1), axis=0)   # no tuple twice
    tup = tup[rng.permutation(len(tup))]
    cut = len(tup) * 4 // 5
    cols = lambda t: (t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy(), np.full(len(t), 4.0))   # noqa: E731
    train, test = cols(tup[:cut]), cols(tup[cut:])
    t0 = time.perf_counter()
    res = h.eval_rankings(train, test, num_recs=10)
    out["topn"] = {"queries": res["n_queries"], "candidates": int(len(np.unique(train[1]))), "device_loop_ms": h.last_iter_ms()[2],
                   "wall_ms": 1e3 * (time.perf_counter() - t0)}
    h.close()
    # the restatement on one core over a prefix, its rows equal to the device's strict run
    p = min(PREFIX, n)
    want = [m.copy() for m in M]
    t0 = time.perf_counter()
    cref.epoch_strict(want, keys[:p], r[:p], LRATE, REG)
    ref_s = time.perf_counter() - t0
    h = capi.CPTFInstance(k, dims, flags=capi.CPTF_FLAG_STRICT)
    h.set_entries(keys[:p], r[:p])
    h.set_model(M)
    h.iterate(LRATE, REG)
    got = h.model()
    h.close()
    same = all(np.array_equal(a.view(np.int64), b.view(np.int64)) for a, b in zip(got, want))
    out["restatement_one_core"] = {"prefix": p, "rows_equal_bit_for_bit": bool(same), "us_per_entry": 1e6 * ref_s / p,
                                   "epoch_ms_extrapolated": 1e3 * ref_s / p * n,
                                   "note": "numpy restatement, extrapolated from the prefix; a compiled one-core loop was not timed"}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cptf_bench.json"))
    ap.add_argument("--small", action="store_true", help="a fiftieth of the synthetic shape: to try the tool")
    a = ap.parse_args()
    runs = []
    for name, (dims, n) in SHAPES.items():
        if a.small and name == "synthetic":
            dims, n = [2000, 400, 5, 5, 5], 100000
        for k in (10, 64):
            runs.append(bench_shape(name, dims, n, k))
            print(json.dumps(runs[-1]), flush=True)
    doc = {"tool": "tools/bench_cptf.py", "lrate": LRATE, "reg": REG, "samples_per_form": 1, "warm_up": 0, "runs": runs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
