#!/usr/bin/env python3
"""Mint tests/golden/reference_bpmf.json.gz by EXECUTING the reference (no JVM: oracle/jvm interprets it).

BPMF runs from its SOURCE (src/carskit/alg/baseline/cf/BPMF.java + generic/IterativeRecommender.java + generic/Recommender.java, through
oracle/jvm/javasrc.py) with librec's DenseMatrix / DenseVector / SparseMatrix / SparseVector / Randoms / Stats and happy.coding's
math.Randoms from the jars' bytecode.  BPMF's own `Randoms` is happy.coding's; DenseMatrix.init draws from librec's: two java.util.Random
objects, both seeded here (`seed_init` for librec's, `seed_gibbs` for happy.coding's).

* `runs`: buildModel() on
    - the 26 x 42 `knn_matrix` of tests/golden/reference_knn.json.gz (read from that file, not stored again) at k in {3, 10};
    - the `handmade` 7 x 6 matrix of mint_reference_rankals.py at k in {1, 2}: a user with no cell, a user whose only cell is a stored
      zero, an item with no cell, a row of one entry, a negative value;
    - the `generated` 24 x 22 matrix (generated() below, stored in the file) at k = 17: 4 to 8 cells a user, a user and an item with no
      cell, a stored zero; wishart() there reaches SparseVector.inner over 11 and 13 indices.
  buildModel has no per-iteration hook, so the state after iteration t is a run with numIters = t from the same seeds, t = 0 (the drawn
  P and Q), 1, 2, 3: P, Q and the loss; every (spec, t) is a process of the pool.  predict(u, j) of every cell after the last run.  globalMean is the caller's here (the driver
  takes it from the contextual matrix, Recommender.java:265): the mean of the non-zero cells, stored in the file.
* from bytecode, apart: `cholesky` (DenseMatrix.cholesky(), the UPPER factor or null), `cov` (cov() and columnMean()), `gamma`
  (Randoms.gamma(alpha, 2), 50 draws each from a seed), `gaussian` (1 000 Randoms.gaussian(0, 1) from a seed), and `wishart`
  (BPMF.wishart(scale, df) from source, with the draws it took).

Doubles are stored as float.hex().

Stand-ins registered HERE (nothing under oracle/ changes): Math.exp is the fdlibm exp of tests/bpr_ref.py (Math.exp is specified to 1 ulp
only; the project defines it as StrictMath's); java.util.Arrays.binarySearch(int[], int) over the whole array.  isConverged() is
IterativeRecommender's own, with verbose off.

    python tests/tools/mint_reference_bpmf.py /path/to/reference"""
import gzip
import json
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle.jvm import interp, javasrc  # noqa: E402
from oracle.jvm.interp import VM, to_list  # noqa: E402
from mint_reference_slopeone import hexd  # noqa: E402
from mint_reference_rankals import flat, handmade  # noqa: E402
from tests.bpr_ref import fdlibm_exp  # noqa: E402

ITERS = 3
DM, SM, SV = "librec/data/DenseMatrix", "librec/data/SparseMatrix", "librec/data/SparseVector"
HAPPY, LIBREC = "happy/coding/math/Randoms", "librec/util/Randoms"
GAMMA_ALPHAS = (1.0, 1.5, 13.0, 50.5, 5000.0)

interp.HOST_STATICS[("java/lang/Math", "exp")] = lambda vm, v: fdlibm_exp(v)
interp.HOST_STATICS[("java/util/Arrays", "binarySearch", "([II)I")] = lambda vm, arr, key: interp._binary_search(vm, arr, 0, len(arr.data), key)


def new_vm(ref):
    return VM([os.path.join(ref, "lib", "librec-v1.4-alpha.jar"), os.path.join(ref, "lib", "happy.coding.utils-1.2.6.jar")])


def new_this(ref):
    from oracle.mint_reference_src import CLASS_MAP
    vm = new_vm(ref)
    src = [os.path.join(ref, "src", "carskit", "alg", "baseline", "cf", "BPMF.java"),
           os.path.join(ref, "src", "carskit", "generic", "IterativeRecommender.java"),
           os.path.join(ref, "src", "carskit", "generic", "Recommender.java")]
    this = javasrc.This(vm, src, dict(CLASS_MAP, Randoms=HAPPY, SparseVector=SV, MatrixEntry="librec/data/MatrixEntry"))
    return vm, this


def generated():
    """24 users x 22 items for the k = 17 run: 4 to 8 cells a user, user 5 with no cell, item 13 with no cell, one stored zero (the third
    cell of user 9); both sides longer than k, so that cov() is not singular by construction"""
    rng = np.random.default_rng(20261218)
    nu, ni = 24, 22
    cells = []
    for u in range(nu):
        if u == 5:
            continue
        c = int(rng.integers(4, 9))
        for j in sorted(rng.choice([j for j in range(ni) if j != 13], size=c, replace=False).tolist()):
            cells.append((u, j, float(rng.integers(1, 11)) / 2.0))
    third9 = next(n for n, c in enumerate(cells) if c[0] == 9) + 2
    cells[third9] = (9, cells[third9][1], 0.0)
    return nu, ni, cells


def run_to(task):
    """buildModel() with numIters = t from the spec's seeds: what the record holds of that state"""
    spec, t = task
    ref, name, nu, ni, cells, k, seed_init, seed_gibbs, store_cells = spec
    from oracle.mint_reference_src import sparse
    nz = [v for _, _, v in cells if v != 0.0]
    gm = 0.0
    for v in nz:
        gm += v
    gm /= len(nz)
    vm, this = new_this(ref)
    train = sparse(vm, nu, ni, cells)
    vm.call(LIBREC, "seed", "(J)V", [seed_init])
    vm.call(HAPPY, "seed", "(J)V", [seed_gibbs])
    this.fields.update({"train": train, "P": None, "Q": None, "numFactors": k, "numIters": t, "numUsers": nu, "numItems": ni,
                        "globalMean": gm, "loss": 0.0, "last_loss": 0.0, "measure": 0.0, "last_measure": 0.0, "lRate": -1.0,
                        "initLRate": -1.0, "maxLRate": -1.0, "decay": -1.0, "isBoldDriver": False, "earlyStopMeasure": None,
                        "verbose": False, "isResultsOut": False, "isUserSplitting": False, "isItemSplitting": False,
                        "algoName": "BPMF", "foldInfo": "", "__enums__": ("Measure",)})
    this.call("buildModel", [])
    out = {"global_mean": hexd(gm), "P": flat(this.fields["P"]), "Q": flat(this.fields["Q"]), "loss": hexd(this.fields["loss"])}
    if t == 1:
        out["row_count"] = [int(vm.call(SV, "getCount", "()I", [vm.call(SM, "row", "(I)L%s;" % SV, [train, u])])) for u in range(nu)]
        out["col_count"] = [int(vm.call(SV, "getCount", "()I", [vm.call(SM, "column", "(I)L%s;" % SV, [train, j])])) for j in range(ni)]
    if t == ITERS:
        out["predict"] = [[hexd(this.call("predict", [u, j])) for j in range(ni)] for u in range(nu)]
    print(name, "k =", k, "numIters =", t, flush=True)
    return out


def assemble(spec, parts):
    """the record of one spec from its runs with numIters = 0 .. ITERS"""
    ref, name, nu, ni, cells, k, seed_init, seed_gibbs, store_cells = spec
    rec = {"name": name, "n_users": nu, "n_items": ni, "k": k, "seed_init": seed_init, "seed_gibbs": seed_gibbs,
           "global_mean": parts[0]["global_mean"], "iters": [{"P": p["P"], "Q": p["Q"], "loss": p["loss"]} for p in parts[1:]]}
    rec["P0"], rec["Q0"] = parts[0]["P"], parts[0]["Q"]
    rec["row_count"], rec["col_count"] = parts[1]["row_count"], parts[1]["col_count"]
    rec["predict"] = parts[ITERS]["predict"]
    if store_cells:
        rec["cells"] = [[u, j, hexd(v)] for u, j, v in cells]
    return rec


def chol_cases():
    rng = np.random.default_rng(20261201)
    nan = float("nan")
    b = rng.standard_normal((10, 10))
    return [("spd_3x3", [[4.0, 2.0, 0.6], [2.0, 5.0, 1.5], [0.6, 1.5, 3.0]]),
            ("indefinite", [[1.0, 2.0], [2.0, 1.0]]),
            ("semidefinite", [[1.0, 1.0], [1.0, 1.0]]),
            ("semidefinite_3x3", [[1.0, 1.0, 0.5], [1.0, 1.0, 2.0], [0.5, 2.0, 9.0]]),
            ("asymmetric", [[4.0, 1.0, 7.0], [2.0, 5.0, -3.0], [0.5, 1.5, 3.0]]),
            ("nan_entry", [[4.0, 2.0], [nan, 5.0]]),
            ("nan_upper_entry", [[4.0, nan], [2.0, 5.0]]),
            ("n1", [[4.0]]),
            ("n1_zero", [[0.0]]),
            ("n1_negative", [[-1.0]]),
            ("spd_10x10", (b @ b.T + 10.0 * np.eye(10)).tolist())]


def run_small(ref):
    from oracle.mint_reference_src import dense
    vm, this = new_this(ref)
    out = {"cholesky": [], "cov": [], "gamma": [], "wishart": []}
    for name, a in chol_cases():
        r = vm.call(DM, "cholesky", "()L%s;" % DM, [dense(vm, np.array(a, dtype=np.float64))])
        out["cholesky"].append({"name": name, "n": len(a), "A": [hexd(x) for row in a for x in row], "upper": None if r is None else flat(r)})
    rng = np.random.default_rng(20261202)
    with_nan = rng.standard_normal((5, 3))
    with_nan[2, 1] = float("nan")
    for name, x in (("one_row", [[1.5, -2.0, 0.25]]), ("two_rows", [[1.0, 2.0], [3.0, -1.0]]), ("6x4", rng.standard_normal((6, 4)).tolist()),
                    ("nan_entry", with_nan.tolist()), ("40x3", (rng.standard_normal((40, 3)) * 3.0 + 1.0).tolist())):
        m = dense(vm, np.array(x, dtype=np.float64))
        c = vm.call(DM, "cov", "()L%s;" % DM, [m])
        out["cov"].append({"name": name, "rows": len(x), "k": len(x[0]), "X": [hexd(v) for row in x for v in row], "cov": flat(c),
                           "mean": [hexd(vm.call(DM, "columnMean", "(I)D", [m, f])) for f in range(len(x[0]))]})
    for a in GAMMA_ALPHAS:
        vm.call(HAPPY, "seed", "(J)V", [20261203])
        out["gamma"].append({"alpha": hexd(a), "seed": 20261203,
                             "draws": [hexd(vm.call(HAPPY, "gamma", "(DD)D", [float(a), 2.0])) for _ in range(50)]})
    vm.call(HAPPY, "seed", "(J)V", [20261204])
    out["gaussian"] = {"seed": 20261204, "draws": [hexd(vm.call(HAPPY, "gaussian", "(DD)D", [0.0, 1.0])) for _ in range(1000)]}
    for p, seed in ((1, 20261205), (2, 20261206), (3, 20261207), (7, 20261208)):
        b = np.random.default_rng(seed).standard_normal((p, p))
        scale = (b @ b.T + p * np.eye(p)) / 10.0
        vm.call(HAPPY, "seed", "(J)V", [seed])
        w = this.call("wishart", [dense(vm, scale), float(p + 30)])
        after = vm.call(HAPPY, "gaussian", "(DD)D", [0.0, 1.0])   # the next draw: where the stream stands
        out["wishart"].append({"p": p, "seed": seed, "df": hexd(float(p + 30)), "scale": [hexd(x) for x in scale.ravel()], "W": flat(w),
                               "next_gaussian": hexd(after)})
    return out


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CARSKIT_REFERENCE", "")
    km = json.loads(gzip.open(os.path.join(ROOT, "tests", "golden", "reference_knn.json.gz"), "rb").read())["knn_matrix"]
    kcells = [(u, j, float.fromhex(v)) for u, j, v in km["cells"]]
    nu, ni, hcells = handmade()
    specs = [(ref, "knn_matrix", km["n_users"], km["n_items"], kcells, 3, 20261210, 20261211, False),
             (ref, "knn_matrix", km["n_users"], km["n_items"], kcells, 10, 20261212, 20261213, False),
             (ref, "handmade", nu, ni, hcells, 1, 20261214, 20261215, True),
             (ref, "handmade", nu, ni, hcells, 2, 20261216, 20261217, True)]
    gu, gi, gcells = generated()
    specs.append((ref, "generated", gu, gi, gcells, 17, 20261219, 20261220, True))
    # every (spec, numIters) is a run of its own: the dearest first (a row costs k^3 in the interpreter)
    tasks = sorted(((s, t) for s in range(len(specs)) for t in range(ITERS + 1)), key=lambda st: -specs[st[0]][5] ** 3 * specs[st[0]][2] * st[1])
    with multiprocessing.Pool(min(len(tasks), os.cpu_count() or 1)) as pool:
        parts = dict(zip(tasks, pool.map(run_to, [(specs[s], t) for s, t in tasks], chunksize=1)))
    runs = [assemble(spec, [parts[(s, t)] for t in range(ITERS + 1)]) for s, spec in enumerate(specs)]
    out = {"source": "BPMF / IterativeRecommender / Recommender from source, librec and happy.coding from the jars' bytecode "
                     "(tests/tools/mint_reference_bpmf.py)", "runs": runs}
    out.update(run_small(ref))
    path = os.path.join(ROOT, "tests", "golden", "reference_bpmf.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print("wrote", path, len(runs), "runs", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
