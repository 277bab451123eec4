#!/usr/bin/env python3
"""Mint tests/golden/reference_evalratings_scales.json.gz by EXECUTING the reference's `Recommender.evalRatings` at rating scales other
than 1..5 (build container only).

    python oracle/mint_reference_evalratings_scales.py [/root/reference]

tests/golden/reference_src.json runs evalRatings() (Recommender.java:504-594) with minRate = 1 and maxRate = 5, where the rounding
`Math.round(pred / minRate) * minRate` multiplies and divides by one and the lower bound equals the rounding unit.  Here the same
interpreted source (oracle/mint_reference_src.py: run_model) runs one epoch of buildModel() on a tiny problem whose ratings lie on a
half-star scale (0.5 .. 5.0) or on 2 .. 10, from initial containers loud enough that the predictions spread over several levels, then evalRatings() over held-out cells with `minRate` / `maxRate` set to that scale.

Inputs, the model after the epoch and the measures (MAE, RMSE, NMAE, rMAE, rRMSE, MPE) are written as data, doubles as hex."""
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import mint_reference_src as M  # noqa: E402

SCALES = ((0.5, 5.0), (2.0, 10.0))
GRID = (("CAMF_CUCI", 7, 5, 2, 3, 60, 3), ("CAMF_C", 6, 8, 3, 2, 70, 4), ("BiasedMF", 8, 6, 2, 2, 60, 5))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    rng = np.random.default_rng(20261018)
    out = {"source": "Recommender.evalRatings of the reference at minRate / maxRate other than 1 / 5, interpreted from source "
                     "(see oracle/mint_reference_evalratings_scales.py); doubles are C99 hex strings", "cases": []}
    for (model, nu, ni, nd, cpd, n, k) in GRID:
        for lo, hi in SCALES:
            prob = M.problem(rng, nu, ni, nd, cpd, n)
            levels = int(round(hi / lo))
            for cell in prob["cells"]:                          # ratings on the case's scale: minRate, 2 minRate, ..., maxRate
                cell[2] = lo * float(rng.integers(1, levels + 1))
            held = [c for i, c in enumerate(prob["cells"]) if i % 3 == 2]            # every third cell is test data
            prob["cells"] = [c for i, c in enumerate(prob["cells"]) if i % 3 != 2]
            # louder initial containers than run_model's own draws, which would leave every prediction within a level of the mean
            nc = prob["n_conds"]
            shapes = {"P": (nu, k), "Q": (ni, k), "userBias": (nu,), "itemBias": (ni,), "condBias": (nc,), "ucBias": (nu, nc), "icBias": (ni, nc)}
            init = {name: (0.6 * lo * rng.standard_normal(shapes[name])).tolist() for name in ("P", "Q") + M.STATE[model]}
            rec = M.run_model(ref, model, prob, k, 1, seed=int(rng.integers(1 << 30)), test_cells=held, min_rate=lo, max_rate=hi,
                              init_override=init)
            rec["min_rate"], rec["max_rate"] = lo, hi
            out["cases"].append(rec)
            ev = {name: float.fromhex(v) for name, v in rec["eval_ratings"].items()}
            print("%-10s %.1f..%.1f  %d test cells: MAE %.6f  RMSE %.6f  NMAE %.6f  rMAE %.6f  rRMSE %.6f"
                  % (model, lo, hi, len(held), ev["MAE"], ev["RMSE"], ev["NMAE"], ev["rMAE"], ev["rRMSE"]), flush=True)
    path = os.path.join(ROOT, "tests", "golden", "reference_evalratings_scales.json.gz")
    with open(path, "wb") as f:                                   # no file name and no time in the header: reruns give the same bytes
        with gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as z:
            z.write(json.dumps(out, indent=0).encode())
    print("wrote", path)


if __name__ == "__main__":
    main()
