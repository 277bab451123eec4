#!/usr/bin/env python3
"""predict / evalRatings through the C ABI on one GPU, one JSON line: ms per call, upload and copy-back included.

    tools/bench_eval_paths.py [--tuples N] [--reps R]

Timed, with the stream drained before and every call returning drained: Instance.predict, eval_ratings and eval_resident on N test
tuples (default 2 M) for CAMF_CI k = 128 fp32 (eval_kernel) and SVD++ k = 64 fp32 (ext_eval_kernel, about ten training items a user),
and FMInstance.predict at k = 64.  Each figure is the median of R calls (default 5) after one that warms up.  The states are random:
nothing is trained, the path's cost does not depend on the numbers."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NU, NI, N_DIMS, CONDS_PER_DIM, N_TRAIN = 100_000, 20_000, 3, 4, 1_000_000
SCALE = (1.0, 5.0)


def timed(call, sync, reps):
    call()
    ms = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ms)), 3)


def main():
    from carskit_amd import capi
    args = sys.argv[1:]
    n = int(args[args.index("--tuples") + 1]) if "--tuples" in args else 2_000_000
    reps = int(args[args.index("--reps") + 1]) if "--reps" in args else 5
    rng = np.random.default_rng(1)
    nc = N_DIMS * CONDS_PER_DIM
    # every context: one condition of each dimension
    ctxs = np.stack(np.meshgrid(*[d * CONDS_PER_DIM + np.arange(CONDS_PER_DIM) for d in range(N_DIMS)], indexing="ij"), -1).reshape(-1, N_DIMS)
    ctx_ptr, ctx_conds = (np.arange(len(ctxs) + 1) * N_DIMS).astype(np.int32), ctxs.reshape(-1).astype(np.int32)
    cells = rng.choice(NU * NI, N_TRAIN, replace=False)
    tu, tj = (cells // NI).astype(np.int32), (cells % NI).astype(np.int32)
    tc, tr = rng.integers(0, len(ctxs), N_TRAIN).astype(np.int32), rng.integers(1, 6, N_TRAIN).astype(np.float64)
    u, j = rng.integers(0, NU, n).astype(np.int32), rng.integers(0, NI, n).astype(np.int32)
    ctx, r = rng.integers(0, len(ctxs), n).astype(np.int32), rng.integers(1, 6, n).astype(np.float64)
    out = {"bench": "eval_paths", "tuples": n, "reps": reps, "runs": []}
    for model, k in (("CAMF_CI", 128), ("SVD++", 64)):
        contextual = model != "SVD++"
        inst = capi.Instance(model, k, NU, NI, nc, flags=0 if contextual else capi.FLAG_SCHED_SERIAL)
        inst.set_hparams(1e-3, 1e-3, 1e-3, 1e-3, 3.0)
        if contextual:
            inst.set_ratings(tu, tj, tc, tr, ctx_ptr, ctx_conds)
        else:
            inst.set_ratings(tu, tj, None, tr)
        inst.set_states({name: (0.1 * rng.standard_normal(inst.state_shape(name))).astype(np.float32) for name in capi.MODEL_STATES[model]})
        c = ctx if contextual else None
        inst.set_eval_ratings(u, j, c, r)
        run = {"model": model, "k": k,
               "predict_ms": timed(lambda: inst.predict(u, j, c, bound=SCALE), inst.synchronize, reps),
               "eval_ratings_ms": timed(lambda: inst.eval_ratings(u, j, c, r, *SCALE), inst.synchronize, reps),
               "eval_resident_ms": timed(lambda: inst.eval_resident(*SCALE), inst.synchronize, reps)}
        assert inst.eval_resident(*SCALE) == inst.eval_ratings(u, j, c, r, *SCALE)
        out["runs"].append(run)
        inst.close()
    k = 64
    fm = capi.FMInstance(k, NU, NI, nc, N_DIMS)
    p = NU + NI + nc
    fm.set_model(3.0, 0.1 * rng.standard_normal(p), 0.1 * rng.standard_normal((p, k)))
    cond = rng.integers(0, nc, n).astype(np.int32)
    out["runs"].append({"model": "FM", "k": k, "predict_ms": timed(lambda: fm.predict(u, j, cond, bound=SCALE), fm.synchronize, reps)})
    fm.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
