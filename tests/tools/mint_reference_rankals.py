#!/usr/bin/env python3
"""Mint tests/golden/reference_rankals.json.gz by EXECUTING the reference (no JVM: oracle/jvm interprets it).

RankALS runs from its SOURCE (src/carskit/alg/baseline/ranking/RankALS.java + generic/IterativeRecommender.java +
generic/Recommender.java, through oracle/jvm/javasrc.py) with librec's DenseMatrix / DenseVector / SparseMatrix / SparseVector from the
jar's bytecode (DenseMatrix.inv / mult / add / minus / scale / setRow / row / rowMult, DenseVector.add / minus / scale / outer,
SparseMatrix.rows / row / get / columnSize, SparseVector.getCount and its iterator).

* buildModel() runs with P and Q injected from a seeded numpy draw (gaussian, std 0.1, stored in the file).  buildModel has no
  per-iteration hook and its loop is `for (iter = 1; iter < numIters; iter++)`, so the state after iteration t is the state after a run
  with numIters = t + 1 from the same start; t = 1, 2, 3.  s and sum_s come from the source's own loop of initModel (restated in
  `weights` below with the same calls on the same matrix, since initModel would redraw P and Q).  predict(u, j) of every cell is
  recorded after the last run.
    - the 26 x 42 `knn_matrix` of tests/golden/reference_knn.json.gz (read from that file, not stored again): k in {3, 10} x -sw on / off;
    - the `handmade` 7 x 6 matrix below at k = 1 (DenseMatrix.inv's n = 1 branch) and k = 2, -sw on and off: a stored zero cell, a
      negative value, a user with no cell, a user whose only cell is a stored zero, an item with no cell, a user with one entry.  The
      file also records what rows(), getCount() and columnSize() make of them;
* `inv`: DenseMatrix.inv() from bytecode on small matrices (a row swap, a pivot tie, a zero column at i = 0 and at i = 1, n = 1 with
  0.0, a NaN, a well-conditioned 10 x 10);
* `init`: one initModel() from Randoms.seed(1) on 4 x 3, k = 2: P, Q, s, sum_s.

Doubles are stored as float.hex().

Stand-ins (the JDK / the DAO / the configuration are not part of the interpreted sources): rateDao.toTraditionalSparseMatrix returns the
2-D matrix the caller built; algoOptions.isOn("-sw") answers from the run's setting; java.util.HashMap is javasrc's (RankALS only puts
and gets by key).

    python tests/tools/mint_reference_rankals.py /path/to/reference"""
import gzip
import json
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle.jvm import javasrc  # noqa: E402
from oracle.jvm.interp import VM, Box, to_list  # noqa: E402
from mint_reference_slopeone import TwoD, hexd  # noqa: E402

ITERS = 3
DM, SM, SV = "librec/data/DenseMatrix", "librec/data/SparseMatrix", "librec/data/SparseVector"


class Options:
    """algoOptions: LineConfiger.isOn("-sw")"""

    def __init__(self, sw):
        self.sw = sw

    def jcall(self, vm, name, desc, args):
        if name == "isOn":
            assert str(getattr(args[0], "s", args[0])).strip("'\"") == "-sw", args
            return bool(self.sw)
        raise KeyError("algoOptions." + name)


def handmade():
    cells = [(0, 0, 5.0 / 3.0), (0, 1, 4.0), (0, 2, 2.5),
             (1, 0, 3.0), (1, 1, 3.5), (1, 3, 0.0),   # (1, 3): a stored zero
             (2, 3, 4.0),                             # one entry
             (3, 3, 2.0), (3, 4, -1.5),               # a negative value
             (4, 0, 2.0), (4, 2, 1.0), (4, 4, 5.0),
             (6, 1, 0.0)]                             # user 5: no cell; user 6: only a stored zero; item 5: no cell
    return 7, 6, cells


def new_this(ref):
    from oracle.mint_reference_src import CLASS_MAP
    vm = VM([os.path.join(ref, "lib", "librec-v1.4-alpha.jar"), os.path.join(ref, "lib", "happy.coding.utils-1.2.6.jar")])
    src = [os.path.join(ref, "src", "carskit", "alg", "baseline", "ranking", "RankALS.java"),
           os.path.join(ref, "src", "carskit", "generic", "IterativeRecommender.java"),
           os.path.join(ref, "src", "carskit", "generic", "Recommender.java")]
    this = javasrc.This(vm, src, dict(CLASS_MAP, SparseVector=SV, VectorEntry="librec/data/VectorEntry"))
    return vm, this


def flat(m):
    return [hexd(x) for row in to_list(m.fields["data"]) for x in row]


def ints(c):
    return [int(x.v if isinstance(x, Box) else x) for x in (c.items if hasattr(c, "items") else to_list(c))]


def run_rankals(spec):
    ref, name, nu, ni, cells, k, sw, seed, store_cells = spec
    from oracle.mint_reference_src import dense, sparse, vector
    rng = np.random.default_rng(seed)
    P0, Q0 = 0.1 * rng.standard_normal((nu, k)), 0.1 * rng.standard_normal((ni, k))
    rec = {"name": name, "n_users": nu, "n_items": ni, "k": k, "sw": bool(sw), "P0": [hexd(x) for x in P0.ravel()],
           "Q0": [hexd(x) for x in Q0.ravel()], "iters": []}
    this = None
    for t in range(1, ITERS + 1):
        vm, this = new_this(ref)
        train = sparse(vm, nu, ni, cells)
        # RankALS.initModel's own loop over the items (RankALS.java:73-79), on the same matrix
        s, sum_s = [], 0.0
        for i in range(ni):
            si = float(vm.call(SM, "columnSize", "(I)I", [train, i])) if sw else 1.0
            s.append(si)
            sum_s += si
        this.fields.update({"train": train, "P": dense(vm, P0), "Q": dense(vm, Q0), "numFactors": k, "numIters": t + 1, "numUsers": nu,
                            "numItems": ni, "isSupportWeight": bool(sw), "s": vector(vm, s), "sum_s": sum_s, "verbose": False,
                            "algoName": "RankALS", "foldInfo": "", "algoOptions": Options(sw)})
        this.call("buildModel", [])
        rec["iters"].append({"P": flat(this.fields["P"]), "Q": flat(this.fields["Q"])})
        if t == 1:
            rec["s"], rec["sum_s"] = [hexd(x) for x in s], hexd(sum_s)
            rec["rows"] = ints(vm.call(SM, "rows", "()Ljava/util/List;", [train]))
            rec["row_count"] = [int(vm.call(SV, "getCount", "()I", [vm.call(SM, "row", "(I)L%s;" % SV, [train, u])])) for u in range(nu)]
            rec["column_size"] = [int(vm.call(SM, "columnSize", "(I)I", [train, i])) for i in range(ni)]
    rec["predict"] = [[hexd(this.call("predict", [u, j])) for j in range(ni)] for u in range(nu)]
    if store_cells:
        rec["cells"] = [[u, j, hexd(v)] for u, j, v in cells]
    print(name, "k =", k, "sw =", sw, flush=True)
    return rec


def run_init(ref, nu, ni, k, seed, sw):
    from oracle.mint_reference_src import sparse
    vm, this = new_this(ref)
    cells = [(u, j, 1.0 + (u + j) % 4) for u in range(nu) for j in range(ni) if (u + 2 * j) % 3]
    this.fields.update({"train": None, "trainMatrix": None, "rateDao": TwoD(sparse(vm, nu, ni, cells)), "numUsers": nu, "numItems": ni,
                        "numFactors": k, "initByNorm": True, "initMean": 0.0, "initStd": 0.1, "isUserSplitting": False,
                        "isItemSplitting": False, "isCARSRecommender": False, "P": None, "Q": None, "s": None, "sum_s": 0.0,
                        "isSupportWeight": False, "algoOptions": Options(sw)})
    vm.call("librec/util/Randoms", "seed", "(J)V", [seed])
    this.call("initModel", [])
    return {"seed": seed, "n_users": nu, "n_items": ni, "k": k, "sw": bool(sw), "cells": [[u, j, hexd(v)] for u, j, v in cells],
            "P": flat(this.fields["P"]), "Q": flat(this.fields["Q"]), "s": [hexd(x) for x in to_list(this.fields["s"].fields["data"])],
            "sum_s": hexd(this.fields["sum_s"])}


def inv_cases():
    rng = np.random.default_rng(20261103)
    nan = float("nan")
    well = rng.standard_normal((10, 10)) + 10.0 * np.eye(10)
    return [("row_swap", [[0.0, 2.0, 1.0], [1.0, 1.0, 0.5], [4.0, -1.0, 3.0]]),
            ("pivot_tie", [[2.0, 1.0, 0.0], [-2.0, 3.0, 1.0], [2.0, 0.5, 5.0]]),
            ("singular_2x2", [[1.0, 2.0], [2.0, 4.0]]),
            ("zero_column_0", [[0.0, 1.0, 2.0], [0.0, 3.0, 4.0], [0.0, 5.0, 7.0]]),
            ("zero_column_1", [[2.0, 4.0, 1.0], [1.0, 2.0, 3.0], [3.0, 6.0, -1.0]]),
            ("n1", [[4.0]]),
            ("n1_zero", [[0.0]]),
            ("n1_negative_zero", [[-0.0]]),
            ("nan_entry", [[1.0, 2.0, 0.5], [nan, 1.0, 3.0], [0.25, -1.0, 2.0]]),
            ("nan_pivot_column", [[nan, 1.0], [nan, 2.0]]),
            ("inf_entry", [[float("inf"), 1.0], [1.0, 2.0]]),
            ("tiny_pivot", [[1e-300, 1.0], [1.0, 1.0]]),
            ("well_10x10", well.tolist())]


def run_inv(ref):
    from oracle.mint_reference_src import dense
    vm = VM([os.path.join(ref, "lib", "librec-v1.4-alpha.jar"), os.path.join(ref, "lib", "happy.coding.utils-1.2.6.jar")])
    out = []
    for name, a in inv_cases():
        r = vm.call(DM, "inv", "()L%s;" % DM, [dense(vm, np.array(a, dtype=np.float64))])
        out.append({"name": name, "n": len(a), "A": [hexd(x) for row in a for x in row], "inv": flat(r)})
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CARSKIT_REFERENCE", "")
    km = json.loads(gzip.open(os.path.join(ROOT, "tests", "golden", "reference_knn.json.gz"), "rb").read())["knn_matrix"]
    kcells = [(u, j, float.fromhex(v)) for u, j, v in km["cells"]]
    nu, ni, hcells = handmade()
    specs = []
    for k, seed in ((3, 20261104), (10, 20261105)):
        for sw in (True, False):
            specs.append((ref, "knn_matrix", km["n_users"], km["n_items"], kcells, k, sw, seed, False))
    for k, seed in ((1, 20261106), (2, 20261107)):
        for sw in (True, False):
            specs.append((ref, "handmade", nu, ni, hcells, k, sw, seed, True))
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        runs = pool.map(run_rankals, specs, chunksize=1)
    out = {"source": "RankALS / IterativeRecommender / Recommender from source, librec DenseMatrix / DenseVector / SparseMatrix / "
                     "SparseVector from lib/librec-v1.4-alpha.jar bytecode (tests/tools/mint_reference_rankals.py)",
           "runs": runs, "inv": run_inv(ref), "init": run_init(ref, 4, 3, 2, 1, True)}
    path = os.path.join(ROOT, "tests", "golden", "reference_rankals.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print("wrote", path, len(runs), "runs", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
