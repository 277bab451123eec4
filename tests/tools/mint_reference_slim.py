#!/usr/bin/env python3
"""Mint tests/golden/reference_slim.json.gz by EXECUTING the reference (no JVM: oracle/jvm interprets it).

SLIM runs from its SOURCE (src/carskit/alg/baseline/ranking/SLIM.java + generic/IterativeRecommender.java + generic/Recommender.java,
through oracle/jvm/javasrc.py) with librec's DenseMatrix / SymmMatrix / SparseMatrix / SparseVector from the jar's bytecode
(SymmMatrix.row, SparseVector.toMap / contains / get, SparseMatrix.row / column / columns / get), happy.coding's Sims and Lists.sortMap
from bytecode.  Every run is Randoms.seed(1), initModel(), buildModel() with 5 iterations.  Recorded per run: the neighbour lists in the
order the loops walk them, W's listed cells after initModel and after iterations 1, 2 and 5 (at the isConverged() call), every
iteration's loss, predict(u, j) for every cell.

* the 26 x 42 `knn_matrix` of tests/golden/reference_knn.json.gz (read from that file): knn in {1, 3, 5, 12, 1000, 0} x
  (l1, l2) in {(1, 1), (0.1, 0.5), (0, 0)}, similarity pcc without shrinkage;
* the `edge_matrix` below (stored in the file): a stored zero cell, users whose row length is no power of two with entries
  SparseVector.contains misses, knn in {3, 4, 6, 7, 12, 13, 24, 25} (one each side of every growth step of the value set) with cos and
  shrinkage 30.

Stand-ins (the JDK and guava's collection classes are not interpreted):
* `java.util.HashMap` (SparseVector.toMap's, from bytecode): JdkHashMap of mint_reference_knn.py, a port of JDK 8's table;
* `HashMultimap.create()`: a map from key to a java.util.HashSet stand-in whose first table is established from guava-18.0.jar's
  BYTECODE: HashMultimap.DEFAULT_VALUES_PER_KEY (the class file's constant) goes through Maps.capacity (run from bytecode) into
  `new HashSet(n)`, which JDK 8 turns into a table of tableSizeFor(n) slots at load 0.75;
* `train.rowCache(cacheSpec)`: a cache that loads train.row(u) once (a guava LoadingCache returns the same vectors);
* rateDao.toTraditionalSparseMatrix returns the 2-D matrix the caller built.

    python tests/tools/mint_reference_slim.py /path/to/reference"""
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
from oracle.jvm.interp import VM, Box, JCollection, f32, to_list  # noqa: E402
from mint_reference_knn import Conf, JdkHashMap, TwoD, hexd  # noqa: E402

ITERS = 5
KEEP = (1, 2, 5)


class SizedHashMap(JdkHashMap):
    """JdkHashMap with HashMap(int initialCapacity): the first table has tableSizeFor(n) slots; plus the lookups bytecode may ask for"""

    def __init__(self, initial=None):
        super().__init__()
        if initial is not None:
            cap = 1
            while cap < initial:
                cap <<= 1
            self.table, self.threshold = [[] for _ in range(cap)], cap * 3 // 4

    def jcall(self, vm, name, desc, args):
        if name == "get":
            k = int(args[0].v)
            for node in (self.table or [[]])[self.hash(k) & (len(self.table or [0]) - 1)]:
                if node[0] == k:
                    return node[1]
            return None
        if name == "containsKey":
            return int(self.jcall(vm, "get", desc, args) is not None)
        if name == "keySet":
            return JCollection([Box(k, "Integer") for b in self.table or [] for k, _ in b])
        return super().jcall(vm, name, desc, args)


class SetMultimap:
    """guava HashMultimap<Integer, Integer>: key -> HashSet(set_capacity) (AbstractSetMultimap.createCollection ->
    Sets.newHashSetWithExpectedSize(expectedValuesPerKey) -> new HashSet(Maps.capacity(...)))"""
    JAVA_TYPES = ("com/google/common/collect/Multimap",)

    def __init__(self, set_capacity):
        self.cap, self.d = set_capacity, {}

    def jcall(self, vm, name, desc, args):
        k = int(args[0].v)
        if name == "put":
            s = self.d.setdefault(k, SizedHashMap(self.cap))
            return int(s.put(int(args[1].v), True) is None)
        if name == "get":
            s = self.d.get(k)
            return JCollection([Box(x, "Integer") for b in (s.table if s else []) for x, _ in b])
        raise KeyError("HashMultimap." + name)


class RowCache:
    def __init__(self, train):
        self.train, self.rows = train, {}

    def jcall(self, vm, name, desc, args):
        if name != "get":
            raise KeyError("LoadingCache." + name)
        u = int(args[0].v)
        if u not in self.rows:
            self.rows[u] = self.train.jcall(vm, "row", "", [u])
        return self.rows[u]


class Train:
    """the librec SparseMatrix `train`, with rowCache() answered here"""

    def __init__(self, m):
        self.m = m

    def jcall(self, vm, name, desc, args):
        if name == "rowCache":
            return RowCache(self)
        return javasrc.vm_call(vm, self.m, self.m.cls_name, name, args, static=False)


def set_capacity(ref):
    """the argument of `new HashSet(n)` behind HashMultimap.create(), from guava's bytecode"""
    vm = VM([os.path.join(ref, "lib", "guava-18.0.jar")])
    per_key = [f for f in vm.jar.load("com/google/common/collect/HashMultimap").fields if f[1] == "DEFAULT_VALUES_PER_KEY"][0][3][1]
    return int(vm.call("com/google/common/collect/Maps", "capacity", "(I)I", [int(per_key)]))


def edge_matrix():
    """14 users x 30 items: every pair of items has common users, so every item has 28+ candidates; user rows of 5-7 and 17-23
    entries; cell (3, 4) is a stored 0.0; item 29 is rated by one user"""
    rng = np.random.default_rng(20261101)
    nu, ni = 14, 30
    cells = {}
    for u in range(nu):
        p = 0.22 if u >= 10 else 0.7
        for j in range(ni - 1):
            if u < 2 or rng.random() < p:
                cells[(u, j)] = float(rng.integers(1, 6)) if rng.random() < 0.8 else float(rng.integers(1, 10)) / 2.0
    cells[(3, 4)] = 0.0
    cells[(5, 29)] = 3.0
    return nu, ni, sorted((u, j, v) for (u, j), v in cells.items())


def run_slim(spec):
    ref, name, nu, ni, cells, knn, l1, l2, measure, shrinkage, setcap = spec
    from oracle.mint_reference_src import CLASS_MAP, sparse
    interp.HOST_CLASSES["java/util/HashMap"] = SizedHashMap
    javasrc.JHashMap = SizedHashMap
    javasrc.STATIC_CALLS[("HashMultimap", "create")] = lambda: SetMultimap(setcap)
    vm = VM([os.path.join(ref, "lib", "librec-v1.4-alpha.jar"), os.path.join(ref, "lib", "happy.coding.utils-1.2.6.jar")])
    src = [os.path.join(ref, "src", "carskit", "alg", "baseline", "ranking", "SLIM.java"),
           os.path.join(ref, "src", "carskit", "generic", "IterativeRecommender.java"),
           os.path.join(ref, "src", "carskit", "generic", "Recommender.java")]
    this = javasrc.This(vm, src, dict(CLASS_MAP, Sims="happy/coding/math/Sims", Lists="happy/coding/io/Lists",
                                      SparseVector="librec/data/SparseVector", VectorEntry="librec/data/VectorEntry"))
    F = this.fields
    F.update({"train": None, "trainMatrix": None, "rateDao": TwoD(Train(sparse(vm, nu, ni, cells))), "numUsers": nu, "numItems": ni,
              "numFactors": 2, "initByNorm": True, "initMean": 0.0, "initStd": 0.1, "isUserSplitting": False, "isItemSplitting": False,
              "isCARSRecommender": False, "P": None, "Q": None, "W": None, "itemNNs": None, "allItems": None, "userCache": None,
              "itemCache": None, "cacheSpec": "maximumSize=200,expireAfterAccess=2m", "knn": knn, "regL1": f32(l1), "regL2": f32(l2),
              "similarityMeasure": measure, "similarityShrinkage": shrinkage, "cf": Conf(shrinkage), "minRate": 1.0, "maxRate": 5.0,
              "numIters": ITERS, "loss": 0.0, "last_loss": 0.0, "isRankingPred": True, "algoName": "SLIM", "verbose": False, "foldInfo": "",
              "globalMean": 0.0})
    vm.call("librec/util/Randoms", "seed", "(J)V", [1])
    this.call("initModel", [])

    def lists():
        out = []
        for j in range(ni):
            c = F["itemNNs"].jcall(vm, "get", "", [Box(j, "Integer")]) if knn > 0 else F["allItems"]
            out.append([int(x.v if isinstance(x, Box) else x) for x in (c.items if hasattr(c, "items") else to_list(c))])
        return out

    nbr = lists()

    def weights():
        data = to_list(F["W"].fields["data"])
        return [[hexd(data[i][j]) for i in nbr[j]] for j in range(ni)]

    rec = {"name": name, "n_users": nu, "n_items": ni, "knn": knn, "l1": l1, "l2": l2, "measure": measure, "shrinkage": shrinkage,
           "neighbors": nbr, "W0": weights(), "W": {}, "loss": []}

    def at_converged(th, args):
        it = int(args[0])
        rec["loss"].append(hexd(th.fields["loss"]))
        if it in KEEP:
            rec["W"][str(it)] = weights()

    this.hooks["isConverged"] = at_converged
    this.call("buildModel", [])
    rec["predict"] = [[hexd(this.call("predict", [u, j])) for j in range(ni)] for u in range(nu)]
    print(name, knn, l1, l2, len(rec["loss"]), "iterations", flush=True)
    return rec


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CARSKIT_REFERENCE", "")
    setcap = set_capacity(ref)
    km = json.loads(gzip.open(os.path.join(ROOT, "tests", "golden", "reference_knn.json.gz"), "rb").read())["knn_matrix"]
    kcells = [(u, j, float.fromhex(v)) for u, j, v in km["cells"]]
    specs = []
    for knn in (1000, 0, 12, 5, 3, 1):
        for l1, l2 in ((1.0, 1.0), (0.1, 0.5), (0.0, 0.0)):
            specs.append((ref, "knn_matrix", km["n_users"], km["n_items"], kcells, knn, l1, l2, "pcc", -1, setcap))
    nu, ni, ecells = edge_matrix()
    for knn in (25, 24, 13, 12, 7, 6, 4, 3):
        specs.append((ref, "edge_matrix", nu, ni, ecells, knn, 0.1, 0.5, "cos", 30, setcap))
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        runs = pool.map(run_slim, specs, chunksize=1)
    runs.sort(key=lambda r: (r["name"] != "knn_matrix", r["knn"], -r["l1"]))
    out = {"source": "SLIM / IterativeRecommender / Recommender from source; librec and happy.coding from their jars' bytecode; the value "
                     "set's first table from guava-18.0.jar's bytecode (tests/tools/mint_reference_slim.py)",
           "hashset_initial_capacity": setcap,
           "edge_matrix": {"n_users": nu, "n_items": ni, "cells": [[u, j, hexd(v)] for u, j, v in ecells]}, "runs": runs}
    path = os.path.join(ROOT, "tests", "golden", "reference_slim.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print("wrote", path, len(runs), "runs")


if __name__ == "__main__":
    main()
