#!/usr/bin/env python3
"""Mint tests/golden/reference_slopeone.json.gz by EXECUTING the reference (no JVM: oracle/jvm interprets it).

SlopeOne runs from its SOURCE (src/carskit/alg/baseline/cf/SlopeOne.java + generic/Recommender.java, through oracle/jvm/javasrc.py)
with librec's DenseMatrix / SparseMatrix / SparseVector from the jar's bytecode: initModel(), buildModel(), then predict(u, j, 0, true)
(bounded to [minRate, maxRate]) and predict(u, j) for every (u, j).  Two matrices:

* `knn_matrix`: the 26 x 42 matrix of tests/golden/reference_knn.json.gz (read from that file, not stored again): duplicated columns
  (zero deviations: +0.0 on both sides of the diagonal), fractional cells, an empty user, an empty item, users with 25-40 items;
* `handmade`: 6 x 5, item pairs without a common user (card 0), a user who rated one item only and a user without ratings (the
  globalMean branch), predictions outside [1, 5].

dev, card and the predictions are stored in full, doubles as float.hex().

Stand-in (the JDK / the DAO are not part of the interpreted sources): rateDao.toTraditionalSparseMatrix returns the 2-D matrix the
caller built (its own derivation is pinned by tests/golden/reference_dao.json).

    python tests/tools/mint_reference_slopeone.py /path/to/reference"""
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.jvm import javasrc  # noqa: E402
from oracle.jvm.interp import VM  # noqa: E402

DM = "librec/data/DenseMatrix"


def hexd(x):
    return float(x).hex()


class TwoD:
    """rateDao: toTraditionalSparseMatrix(trainMatrix) returns the prepared 2-D matrix"""

    def __init__(self, m):
        self.m = m

    def jcall(self, vm, name, desc, args):
        if name == "toTraditionalSparseMatrix":
            return self.m
        raise KeyError("rateDao." + name)


def handmade():
    cells = [(0, 0, 5.0 / 3.0), (0, 1, 4.0), (0, 2, 2.5),
             (1, 0, 3.0), (1, 1, 3.5),
             (2, 3, 4.0),                      # rated item 3 only
             (3, 3, 2.0), (3, 4, 7.0 / 3.0),
             (4, 2, 1.0), (4, 4, 5.0)]         # user 5: no ratings; items {0, 1} and {3} share no user
    return 6, 5, cells


def global_mean(cells):
    s = 0.0
    for _, _, v in cells:
        s += v
    return s / len(cells)


def run_slopeone(ref, name, nu, ni, cells, min_rate=1.0, max_rate=5.0, store_cells=True):
    from oracle.mint_reference_src import CLASS_MAP, sparse
    vm = VM([os.path.join(ref, "lib", "librec-v1.4-alpha.jar"), os.path.join(ref, "lib", "happy.coding.utils-1.2.6.jar")])
    src = [os.path.join(ref, "src", "carskit", "alg", "baseline", "cf", "SlopeOne.java"),
           os.path.join(ref, "src", "carskit", "generic", "Recommender.java")]
    this = javasrc.This(vm, src, dict(CLASS_MAP))
    gm = global_mean(cells)
    this.fields.update({"train": None, "trainMatrix": None, "rateDao": TwoD(sparse(vm, nu, ni, cells)), "numUsers": nu, "numItems": ni,
                        "globalMean": gm, "isRankingPred": False, "isUserSplitting": False, "isItemSplitting": False,
                        "isCARSRecommender": False, "minRate": min_rate, "maxRate": max_rate, "algoName": "SlopeOne",
                        "devMatrix": None, "cardMatrix": None})
    this.call("initModel", [])
    this.call("buildModel", [])
    get = lambda m, a, b: vm.call(DM, "get", "(II)D", [this.fields[m], a, b])  # noqa: E731
    card = [[get("cardMatrix", a, b) for b in range(ni)] for a in range(ni)]
    assert all(float(c) == int(c) for row in card for c in row)
    rec = {"name": name, "n_users": nu, "n_items": ni, "global_mean": hexd(gm), "min_rate": hexd(min_rate), "max_rate": hexd(max_rate),
           "dev": [[hexd(get("devMatrix", a, b)) for b in range(ni)] for a in range(ni)],
           "card": [[int(c) for c in row] for row in card],
           "predict_bounded": [[hexd(this.call("predict", [u, j, 0, True])) for j in range(ni)] for u in range(nu)],
           "predict": [[hexd(this.call("predict", [u, j])) for j in range(ni)] for u in range(nu)]}
    if store_cells:
        rec["cells"] = [[u, j, hexd(v)] for u, j, v in cells]
    return rec


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CARSKIT_REFERENCE", "")
    km = json.loads(gzip.open(os.path.join(ROOT, "tests", "golden", "reference_knn.json.gz"), "rb").read())["knn_matrix"]
    runs = [run_slopeone(ref, "knn_matrix", km["n_users"], km["n_items"], [(u, j, float.fromhex(v)) for u, j, v in km["cells"]],
                         store_cells=False)]
    print("knn_matrix", flush=True)
    nu, ni, cells = handmade()
    runs.append(run_slopeone(ref, "handmade", nu, ni, cells))
    out = {"source": "SlopeOne / Recommender from source, librec DenseMatrix / SparseMatrix / SparseVector from lib/librec-v1.4-alpha.jar "
                     "bytecode (tests/tools/mint_reference_slopeone.py)", "runs": runs}
    path = os.path.join(ROOT, "tests", "golden", "reference_slopeone.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print("wrote", path, len(runs), "runs")


if __name__ == "__main__":
    main()
