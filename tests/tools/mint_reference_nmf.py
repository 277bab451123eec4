#!/usr/bin/env python3
"""Mint tests/golden/reference_nmf.json.gz by EXECUTING the reference (no JVM: oracle/jvm interprets it).

NMF runs from its SOURCE (src/carskit/alg/baseline/cf/NMF.java + generic/IterativeRecommender.java + generic/Recommender.java, through
oracle/jvm/javasrc.py) with librec's DenseMatrix / DenseVector / SparseMatrix / SparseVector from the jar's bytecode.

* three buildModel() runs with W and H injected from a seeded numpy draw (uniform in [0, 0.01), stored in the file): the 26 x 42
  `knn_matrix` of tests/golden/reference_knn.json.gz (read from that file, not stored again) at k = 3 and k = 10, and the `handmade`
  6 x 5 matrix of the SlopeOne mint at k = 2; 3 iterations each.  W, H (k x numItems) and the loss are recorded after every iteration
  (at the isConverged() call), predict(u, j) and predict(u, j, 0, true) for every (u, j) after the last;
* one initModel() run from Randoms.seed(1) on 4 x 3, k = 2: W and H, which pins init(0.01) and the P / Q draws before it.

Doubles are stored as float.hex().

Stand-ins (the JDK / the DAO are not part of the interpreted sources): rateDao.toTraditionalSparseMatrix returns the 2-D matrix the
caller built.

    python tests/tools/mint_reference_nmf.py /path/to/reference"""
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle.jvm import javasrc  # noqa: E402
from oracle.jvm.interp import VM, f32, to_list  # noqa: E402
from mint_reference_slopeone import TwoD, handmade, hexd  # noqa: E402

ITERS = 3


def sources(ref):
    return [os.path.join(ref, "src", "carskit", "alg", "baseline", "cf", "NMF.java"),
            os.path.join(ref, "src", "carskit", "generic", "IterativeRecommender.java"),
            os.path.join(ref, "src", "carskit", "generic", "Recommender.java")]


def new_this(ref):
    from oracle.mint_reference_src import CLASS_MAP
    vm = VM([os.path.join(ref, "lib", "librec-v1.4-alpha.jar"), os.path.join(ref, "lib", "happy.coding.utils-1.2.6.jar")])
    this = javasrc.This(vm, sources(ref), dict(CLASS_MAP, SparseVector="librec/data/SparseVector", MatrixEntry="librec/data/MatrixEntry"))
    return vm, this


def flat(m):
    return [hexd(x) for row in to_list(m.fields["data"]) for x in row]


def run_nmf(ref, name, nu, ni, cells, k, seed, min_rate=1.0, max_rate=5.0, store_cells=True):
    from oracle.mint_reference_src import dense, sparse
    vm, this = new_this(ref)
    rng = np.random.default_rng(seed)
    W0, H0 = 0.01 * rng.random((nu, k)), 0.01 * rng.random((k, ni))
    F = this.fields
    F.update({"W": dense(vm, W0), "H": dense(vm, H0), "V": sparse(vm, nu, ni, cells), "numFactors": k, "numIters": ITERS, "numUsers": nu,
              "numItems": ni, "lRate": -1.0, "loss": 0.0, "last_loss": 0.0, "isUserSplitting": False, "isItemSplitting": False,
              "isRankingPred": False, "minRate": min_rate, "maxRate": max_rate, "algoName": "NMF", "verbose": False, "foldInfo": "",
              "measure": 0.0, "last_measure": 0.0, "earlyStopMeasure": None, "isResultsOut": False, "initLRate": f32(-1.0),
              "maxLRate": f32(-1.0), "decay": f32(-1.0), "isBoldDriver": False, "__enums__": ("Measure",)})
    trace = []
    # called at the head of isConverged(iter), which then runs from source (no early-stop measure: it never ends the loop here)
    this.hooks["isConverged"] = lambda th, args: trace.append({"W": flat(th.fields["W"]), "H": flat(th.fields["H"]),
                                                               "loss": hexd(th.fields["loss"])})
    this.call("buildModel", [])
    assert len(trace) == ITERS
    rec = {"name": name, "n_users": nu, "n_items": ni, "k": k, "min_rate": hexd(min_rate), "max_rate": hexd(max_rate),
           "W0": [hexd(x) for x in W0.ravel()], "H0": [hexd(x) for x in H0.ravel()], "iters": trace,
           "predict": [[hexd(this.call("predict", [u, j])) for j in range(ni)] for u in range(nu)],
           "predict_bounded": [[hexd(this.call("predict", [u, j, 0, True])) for j in range(ni)] for u in range(nu)]}
    if store_cells:
        rec["cells"] = [[u, j, hexd(v)] for u, j, v in cells]
    return rec


def run_init(ref, nu, ni, k, seed):
    from oracle.mint_reference_src import sparse
    vm, this = new_this(ref)
    cells = [(u, j, 1.0 + (u + j) % 4) for u in range(nu) for j in range(ni) if (u + 2 * j) % 3]
    this.fields.update({"train": None, "trainMatrix": None, "rateDao": TwoD(sparse(vm, nu, ni, cells)), "numUsers": nu, "numItems": ni,
                        "numFactors": k, "initByNorm": True, "initMean": 0.0, "initStd": 0.1, "isUserSplitting": False,
                        "isItemSplitting": False, "isCARSRecommender": False, "W": None, "H": None, "V": None, "P": None, "Q": None})
    vm.call("librec/util/Randoms", "seed", "(J)V", [seed])
    this.call("initModel", [])
    return {"seed": seed, "n_users": nu, "n_items": ni, "k": k, "W": flat(this.fields["W"]), "H": flat(this.fields["H"])}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CARSKIT_REFERENCE", "")
    km = json.loads(gzip.open(os.path.join(ROOT, "tests", "golden", "reference_knn.json.gz"), "rb").read())["knn_matrix"]
    kcells = [(u, j, float.fromhex(v)) for u, j, v in km["cells"]]
    runs = []
    for k, seed in ((3, 20261019), (10, 20261020)):
        runs.append(run_nmf(ref, "knn_matrix", km["n_users"], km["n_items"], kcells, k, seed, store_cells=False))
        print("knn_matrix k =", k, flush=True)
    nu, ni, cells = handmade()
    runs.append(run_nmf(ref, "handmade", nu, ni, cells, 2, 20261021))
    out = {"source": "NMF / IterativeRecommender / Recommender from source, librec DenseMatrix / DenseVector / SparseMatrix / SparseVector "
                     "from lib/librec-v1.4-alpha.jar bytecode (tests/tools/mint_reference_nmf.py)",
           "runs": runs, "init": run_init(ref, 4, 3, 2, 1)}
    path = os.path.join(ROOT, "tests", "golden", "reference_nmf.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print("wrote", path, len(runs), "runs")


if __name__ == "__main__":
    main()
