#!/usr/bin/env python3
"""Mint tests/golden/reference_cptf.json.gz by EXECUTING the reference (no JVM: oracle/jvm interprets it).

CPTF runs from its SOURCE (src/carskit/alg/cars/adaptation/independent/CPTF.java + generic/TensorRecommender.java +
generic/IterativeRecommender.java + generic/Recommender.java, through oracle/jvm/javasrc.py) with librec's DenseMatrix from the jar's
bytecode: initModel() (M[d] = new DenseMatrix(dimensions[d], numFactors), M[d].init(1, 0.1) from librec's Randoms), buildModel(), the
two predicts.

`runs` pin the MODEL's arithmetic: the order of the products, of the sum over f, of the loss terms, the unguarded division, the
rate <= 0 skip; their trainTensor is a stand-in list (below).  `tensors` pin the TENSOR: DataDAO.toSparseTensor from source,
TensorRecommender's fold split over librec's SparseTensor from the jar's bytecode, getKeys, predict(u, j, c) and evalRatings
(tests/tools/mint_reference_cptf_tensor.py, which names the stand-ins it adds and the JDK / guava behaviour they assume).

Per run: initModel() runs as it stands (its draw from Randoms.seed(1) is stored once, `init`); M is then replaced by a seeded numpy
draw (stored).  buildModel has no per-iteration hook, so the state after iteration t is the state after a run with numIters = t from
the same start; t = 1, 2, 3 (bold driver off, no decay).  Per t: M and the loss.  After t = 3: predict(keys) of a list of key tuples,
free and through TensorRecommender.predict(keys, true).

Runs (tensors() below): three tensors of at most 120 entries with 1 and 3 context dimensions, one of them
with stored rates <= 0, one with two entries on the same keys (what the reference's size() - 1 keys make of two contexts of one pair),
each at k in {1, 3, 10}; `zero` has one zero element on a row that is trained twice, so its loss is NaN in the first iteration, where
IterativeRecommender.isConverged ends the program (System.exit(-1)): that run holds the state after its one sweep (`exits_after`).

Doubles are stored as float.hex().

Stand-ins (the JDK, the configuration and the data layer are not part of the interpreted sources): trainTensor is a Python list of
entries with keys() -> int[] and get() -> double, iterated in list order, which is what librec's TensorIterator does over its parallel
lists; isConverged runs from IterativeRecommender's source with verbose off and no early-stop measure.

    python tests/tools/mint_reference_cptf.py /path/to/reference"""
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle.jvm import javasrc  # noqa: E402
from oracle.jvm.interp import VM, JArray, to_list  # noqa: E402
from oracle.mint_reference_src import CLASS_MAP, dense  # noqa: E402

ITERS = 3


def hexd(x):
    return float(x).hex()


def f32(x):
    return float(np.float32(x))


class Entry:
    """librec.data.TensorEntry as CPTF.java:81-83 uses it"""

    def __init__(self, keys, rate):
        self._keys, self._rate = [int(x) for x in keys], float(rate)

    def keys(self):
        return JArray("I", list(self._keys))

    def get(self):
        return self._rate


def new_this(ref):
    vm = VM([os.path.join(ref, "lib", "librec-v1.4-alpha.jar"), os.path.join(ref, "lib", "happy.coding.utils-1.2.6.jar")])
    g = os.path.join(ref, "src", "carskit", "generic")
    src = [os.path.join(ref, "src", "carskit", "alg", "cars", "adaptation", "independent", "CPTF.java"),
           os.path.join(g, "TensorRecommender.java"), os.path.join(g, "IterativeRecommender.java"), os.path.join(g, "Recommender.java")]
    return vm, javasrc.This(vm, src, dict(CLASS_MAP))


def prepared(ref, dims, k, t, lrate, reg, entries, lo, hi):
    vm, this = new_this(ref)
    this.fields.update({"M": None, "numDimensions": len(dims), "dimensions": JArray("I", [int(d) for d in dims]), "userDimension": 0,
                        "itemDimension": 1, "numFactors": k, "numIters": t, "trainTensor": [Entry(ks, r) for ks, r in entries],
                        "lRate": lrate, "initLRate": lrate, "maxLRate": f32(-1.0), "decay": f32(-1.0), "isBoldDriver": False,
                        "reg": reg, "loss": 0.0, "last_loss": 0.0, "measure": 0.0, "last_measure": 0.0, "earlyStopMeasure": None,
                        "verbose": False, "isResultsOut": False, "algoName": "CPTF", "foldInfo": "", "minRate": lo, "maxRate": hi,
                        "__enums__": ("Measure",)})
    vm.call("librec/util/Randoms", "seed", "(J)V", [1])
    this.call("initModel", [])
    return vm, this


def matrices(this):
    M = this.fields["M"]
    return M.data if isinstance(M, JArray) else M


def flat(this):
    return [hexd(x) for m in matrices(this) for row in to_list(m.fields["data"]) for x in row]


def run_cptf(ref, name, dims, k, seed, entries, zero=None):
    rng = np.random.default_rng(seed)
    scale = (3.0 / k) ** (1.0 / len(dims))
    M0 = [scale * (1.0 + 0.1 * rng.standard_normal((n, k))) for n in dims]
    if zero is not None:
        M0[zero[0]][zero[1], zero[2]] = 0.0
    lrate, reg, lo, hi = f32(0.013), f32(0.027), 1.0, 5.0
    grid = np.stack([g.ravel() for g in np.meshgrid(*[np.arange(min(n, 2)) for n in dims], indexing="ij")], axis=1).tolist()
    rec = {"name": "%s k=%d" % (name, k), "dims": dims, "k": k, "seed": seed, "lrate": hexd(lrate), "reg": hexd(reg),
           "min_rate": hexd(lo), "max_rate": hexd(hi), "keys": [x for ks, _ in entries for x in ks],
           "rates": [hexd(r) for _, r in entries], "M0": [hexd(x) for m in M0 for x in m.ravel()], "iters": [],
           "predict_keys": [x for ks in grid for x in ks]}
    for t in range(1, ITERS + 1):
        vm, this = prepared(ref, dims, k, t, lrate, reg, entries, lo, hi)
        if t == 1 and "init" not in rec:
            rec["init"] = flat(this)
        arr = matrices(this)
        for d in range(len(dims)):
            arr[d] = dense(vm, M0[d])
        try:
            this.call("buildModel", [])
        except javasrc.JavaExit:   # IterativeRecommender.isConverged on a NaN / Inf loss: System.exit(-1), after :111 of that sweep
            assert not np.isfinite(this.fields["loss"])
            rec["exits_after"] = len(rec["iters"]) + 1
        rec["iters"].append({"M": flat(this), "loss": hexd(this.fields["loss"])})
        if "exits_after" in rec:
            break
    rec["predict"] = [hexd(javasrc.unbox(this.call("predict", [JArray("I", list(ks))]))) for ks in grid]
    rec["predict_bounded"] = [hexd(javasrc.unbox(this.call("predict", [JArray("I", list(ks)), True]))) for ks in grid]
    print(rec["name"], "loss", [float.fromhex(it["loss"]) for it in rec["iters"]], flush=True)
    return rec


def tensors():
    """name -> (dims, entries)"""
    rng = np.random.default_rng(20271001)
    out = {}
    dims = [5, 6, 3]
    out["one_ctx"] = (dims, [([int(rng.integers(0, n)) for n in dims], float(rng.integers(1, 6))) for _ in range(60)])
    dims = [6, 7, 2, 3, 2]
    ents = [([int(rng.integers(0, n)) for n in dims], float(rng.integers(0, 6))) for _ in range(120)]       # rates of 0: skipped
    ents[5] = (ents[5][0], -1.0)
    out["three_ctx_zero_rates"] = (dims, ents)
    dims = [4, 4, 2, 2]
    ents = [([int(rng.integers(0, n)) for n in dims], float(rng.integers(1, 6))) for _ in range(40)]
    ents[7] = (list(ents[3][0]), 2.0)                                                                         # the same keys twice
    ents[8] = (list(ents[3][0]), 5.0)
    out["collapsed_keys"] = (dims, ents)
    return out


def tensor_cases(ref):
    """the built tensor, getKeys, one fold, predict(u, j, c) and evalRatings, executed: 3, 1 and 0 context dimensions (librec's
    SparseTensor refuses fewer than 3 dimensions: recorded), and few users with many cells each (HashSet order of the positions)"""
    from mint_reference_cptf_tensor import executed_case, tensor_case
    specs = [("three_ctx", 6, 7, [2, 3, 2], 60, 8, 1), ("one_ctx", 5, 6, [3], 40, 6, 2), ("no_ctx", 5, 6, [], 20, 4, 3),
             ("busy_users", 3, 8, [4], 90, 10, 4)]
    out = [tensor_case(ref, *a) for a in specs]
    # user 0 holds the positions 3 and 4 of the rate tensor: in a HashSet of 4 slots they iterate as 4, 3
    out.append(executed_case(ref, "hash_order", 2, 3, [1, 1, 1, 0], [0, 1, 2, 0], [[0], [1]], {0: 0, 1: 0},
                             [(0, 0, 1.0), (1, 0, 2.0), (2, 0, 3.0), (3, 0, 4.0), (3, 1, 5.0)], [(3, 0, 4.0)], np.random.default_rng(5)))
    for r in out:
        print(r["name"], r.get("dims", r.get("refused")), flush=True)
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CARSKIT_REFERENCE", "")
    runs = []
    for name, (dims, ents) in tensors().items():
        for k in (1, 3, 10):
            runs.append(run_cptf(ref, name, dims, k, 20271000 + k, ents))
    dims, ents = tensors()["one_ctx"]
    runs.append(run_cptf(ref, "zero", dims, 3, 20271009, ents, zero=(1, ents[0][0][1], 1)))
    init = runs[0].pop("init")
    for r in runs[1:]:
        r.pop("init", None)
    out = {"source": "CPTF / TensorRecommender / IterativeRecommender / Recommender from source, librec DenseMatrix from "
                     "lib/librec-v1.4-alpha.jar bytecode (tests/tools/mint_reference_cptf.py); trainTensor is a stand-in list of entries: "
                     "the tensor build and the fold split are not executed",
           "tensor_source": "DataDAO.toSparseTensor, TensorRecommender.getKeys / evalRatings and CPTF.predict(u, j, c) from source, "
                            "librec's SparseTensor from bytecode (tests/tools/mint_reference_cptf_tensor.py, which names its stand-ins)",
           "tensors": tensor_cases(ref), "runs": runs, "init": {"seed": 1, "dims": runs[0]["dims"], "k": runs[0]["k"], "M": init}}
    path = os.path.join(ROOT, "tests", "golden", "reference_cptf.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print("wrote", path, len(runs), "runs", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
