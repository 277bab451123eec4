#!/usr/bin/env python3
"""Mint tests/golden/reference_lrmf.json.gz by EXECUTING the reference (no JVM: oracle/jvm interprets it).

LRMF runs from its SOURCE (src/carskit/alg/baseline/ranking/LRMF.java + generic/IterativeRecommender.java + generic/Recommender.java,
through oracle/jvm/javasrc.py) with librec's DenseMatrix / DenseVector / SparseMatrix (its MatrixEntry iterator, getColumns) from the
jar's bytecode.

* initModel() runs as it stands (super.initModel() draws P and Q from librec's Randoms, then userExp is summed over the iterator); P and
  Q are then replaced by a seeded numpy draw (uniform(0, 1), stored in the file).  buildModel has no per-iteration hook, so the state
  after iteration t is the state after a run with numIters = t from the same start; t = 1, 2, 3 (bold driver off, no decay: lRate
  stays).  Per t the file holds P, Q and loss; predict(u, j) of every cell is recorded after the last run.
    - the 26 x 42 `knn_matrix` of tests/golden/reference_knn.json.gz (read from that file, not stored again) at k in {3, 10};
    - the 7 x 6 `handmade` matrix of tests/tools/mint_reference_rankals.py at k in {1, 2}: a stored zero beside other cells, an empty
      user, a one-cell user and a user whose only cell is a stored zero.  That user's uexp is 0.0, the loss is non-finite in iteration 1
      and isConverged() ends the run through System.exit(-1): the file holds that one iteration (`exited`: true) with P, Q and loss as
      they stood at the exit;
    - `handmade_finite`, the same matrix without that user's cell, at k in {1, 2}: three finite iterations with the stored zero beside
      other cells.
  Per run the file records what librec makes of the matrix: `entries`, the (row, column, value) of every MatrixEntry in iterator order
  -- stored zeros are among them --, `columns`, getColumns(u) of every user -- stored zeros are not --, and `user_exp`.

Doubles are stored as float.hex().

Stand-ins (the JDK and the configuration are not part of the interpreted sources): Math.exp and Math.log are the fdlibm restatements of
tests/bpr_ref.py (StrictMath's; Math's are specified to 1 ulp only).

    python tests/tools/mint_reference_lrmf.py /path/to/reference"""
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
from oracle.jvm.interp import VM, to_list  # noqa: E402
from mint_reference_slopeone import TwoD, hexd  # noqa: E402
from mint_reference_rankals import handmade, flat  # noqa: E402
from tests import bpr_ref  # noqa: E402

ITERS = 3
SM = "librec/data/SparseMatrix"
javasrc.STATIC_CALLS[("Math", "exp")] = bpr_ref.fdlibm_exp
javasrc.STATIC_CALLS[("Math", "log")] = bpr_ref.fdlibm_log


def f32(x):
    return float(np.float32(x))


def new_this(ref):
    from oracle.mint_reference_src import CLASS_MAP
    vm = VM([os.path.join(ref, "lib", "librec-v1.4-alpha.jar"), os.path.join(ref, "lib", "happy.coding.utils-1.2.6.jar")])
    src = [os.path.join(ref, "src", "carskit", "alg", "baseline", "ranking", "LRMF.java"),
           os.path.join(ref, "src", "carskit", "generic", "IterativeRecommender.java"),
           os.path.join(ref, "src", "carskit", "generic", "Recommender.java")]
    cmap = dict(CLASS_MAP, MatrixEntry="librec/data/MatrixEntry")
    return vm, javasrc.This(vm, src, cmap)


def entries_of(vm, train):
    it = vm.invoke("interface", "java/lang/Iterable", "iterator", "()Ljava/util/Iterator;", [train])
    out = []
    while vm.invoke("interface", "java/util/Iterator", "hasNext", "()Z", [it]):
        me = vm.invoke("interface", "java/util/Iterator", "next", "()Ljava/lang/Object;", [it])
        row = vm.invoke("interface", "librec/data/MatrixEntry", "row", "()I", [me])
        col = vm.invoke("interface", "librec/data/MatrixEntry", "column", "()I", [me])
        val = vm.invoke("interface", "librec/data/MatrixEntry", "get", "()D", [me])
        out.append([int(row), int(col), hexd(val)])
    return out


def ints(c):
    return [int(getattr(x, "v", x)) for x in (c.items if hasattr(c, "items") else to_list(c))]


def run_lrmf(spec):
    ref, name, nu, ni, cells, k, seed, store_cells = spec
    from oracle.mint_reference_src import dense, sparse
    rng = np.random.default_rng(seed)
    P0, Q0 = rng.random((nu, k)), rng.random((ni, k))
    lrate, reg_u, reg_i = f32(0.05), f32(0.02), f32(0.03)
    rec = {"name": name, "n_users": nu, "n_items": ni, "k": k, "seed": seed, "lrate": hexd(lrate), "reg_u": hexd(reg_u),
           "reg_i": hexd(reg_i), "P0": [hexd(x) for x in P0.ravel()], "Q0": [hexd(x) for x in Q0.ravel()], "iters": [], "exited": False}
    this = None
    for t in range(1, ITERS + 1):
        vm, this = new_this(ref)
        train = sparse(vm, nu, ni, cells)
        this.fields.update({"train": None, "trainMatrix": None, "rateDao": TwoD(train), "numFactors": k, "numIters": t, "numUsers": nu,
                            "numItems": ni, "initByNorm": False, "initMean": 0.0, "initStd": 0.1, "isUserSplitting": False,
                            "isItemSplitting": False, "isCARSRecommender": False, "P": None, "Q": None, "userExp": None,
                            "lRate": lrate, "initLRate": lrate, "maxLRate": f32(-1.0), "decay": f32(-1.0),
                            "isBoldDriver": False, "regU": reg_u, "regI": reg_i, "loss": 0.0, "last_loss": 0.0, "measure": 0.0,
                            "last_measure": 0.0, "earlyStopMeasure": None, "verbose": False, "isResultsOut": False, "algoName": "LRMF",
                            "foldInfo": "", "__enums__": ("Measure",)})
        vm.call("librec/util/Randoms", "seed", "(J)V", [seed])
        this.call("initModel", [])
        train = this.fields["train"]
        if t == 1:
            rec["user_exp"] = [hexd(x) for x in to_list(vm.call("librec/data/DenseVector", "getData", "()[D", [this.fields["userExp"]]))]
            rec["columns"] = [ints(vm.call(SM, "getColumns", "(I)Ljava/util/List;", [train, u])) for u in range(nu)]
            rec["entries"] = entries_of(vm, train)
        this.fields["P"], this.fields["Q"] = dense(vm, P0), dense(vm, Q0)
        try:
            this.call("buildModel", [])
        except javasrc.JavaExit:
            rec["exited"] = True
        rec["iters"].append({"P": flat(this.fields["P"]), "Q": flat(this.fields["Q"]), "loss": hexd(this.fields["loss"])})
        if rec["exited"]:
            assert t == 1, "the run left in iteration 1 or never"
            break
    rec["predict"] = [[hexd(this.call("predict", [u, j])) for j in range(ni)] for u in range(nu)]
    if store_cells:
        rec["cells"] = [[u, j, hexd(v)] for u, j, v in cells]
    print(name, "k =", k, "exited" if rec["exited"] else "", flush=True)
    return rec


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CARSKIT_REFERENCE", "")
    km = json.loads(gzip.open(os.path.join(ROOT, "tests", "golden", "reference_knn.json.gz"), "rb").read())["knn_matrix"]
    kcells = [(u, j, float.fromhex(v)) for u, j, v in km["cells"]]
    nu, ni, hcells = handmade()
    fcells = [c for c in hcells if c[0] != 6]
    assert len(fcells) == len(hcells) - 1
    specs = [(ref, "handmade", nu, ni, hcells, 1, 20270201, True), (ref, "handmade", nu, ni, hcells, 2, 20270202, True),
             (ref, "handmade_finite", nu, ni, fcells, 1, 20270201, True), (ref, "handmade_finite", nu, ni, fcells, 2, 20270202, True),
             (ref, "knn_matrix", km["n_users"], km["n_items"], kcells, 3, 20270203, False),
             (ref, "knn_matrix", km["n_users"], km["n_items"], kcells, 10, 20270204, False)]
    if len(sys.argv) > 2:   # a subset of the runs, to try the tool
        specs = [specs[int(x)] for x in sys.argv[2].split(",")]
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        runs = pool.map(run_lrmf, specs, chunksize=1)
    out = {"source": "LRMF / IterativeRecommender / Recommender from source, librec DenseMatrix / DenseVector / SparseMatrix from "
                     "lib/librec-v1.4-alpha.jar bytecode; Math.exp / Math.log = fdlibm (tests/tools/mint_reference_lrmf.py)",
           "runs": runs}
    path = os.path.join(ROOT, "tests", "golden", "reference_lrmf.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print("wrote", path, len(runs), "runs", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
