#!/usr/bin/env python3
"""Mint tests/golden/reference_knn.json.gz by EXECUTING the reference (no JVM: oracle/jvm interprets it).

* `sims`: happy.coding.math.Sims (pcc, cos, msd, cpc, exJaccard) run from the BYTECODE of lib/happy.coding.utils-1.2.6.jar on common
  lists: hand-made ones (constant common values, a single common entry, no overlap, identical vectors, anti-correlation, +-Infinity)
  and pairs of the DePaul and Frappe 2-D matrices.
* `models`: ItemKNN and UserKNN run from their SOURCE (src/carskit/alg/baseline/cf/{ItemKNN,UserKNN}.java + generic/Recommender.java,
  through oracle/jvm/javasrc.py) on a small matrix built for it: initModel() -> Recommender.buildCorrs -> correlation() (list building,
  the isNaN guard, shrinkage with n = is.size(), cos-binary's SparseVector.inner from the librec jar's bytecode, Sims from the happy jar's
  bytecode), the itemMeans / userMeans loop, and predict(u, j, c, true) for every (u, j) and several knn -- Lists.sortMap from bytecode.
  Every similarity measure and shrinkage in {-1, 30} is built; predictions cover pcc and cos.  The matrix has duplicated columns / rows
  (exact ties at the knn cut) and users / items with 25-40 candidates, so the first map grows to 64 slots and the re-put after the cut
  lands in that kept table, not in a fresh 16-slot one.

Stand-ins (the JDK is not part of the reference tree): `java.util.HashMap` is `JdkHashMap` below, a port of JDK 8's putVal / resize /
treeifyBin / clear over a real bin table (clear() keeps the table); Double.isInfinite; `cf.getInt("num.shrinkage")` as
Integer.parseInt of the configured value; rateDao.toTraditionalSparseMatrix returns the 2-D matrix the caller built (its own derivation
is pinned by tests/golden/reference_dao.json).

    python tests/tools/mint_reference_knn.py /path/to/reference"""
import json
import math

import numpy as np
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.jvm import interp  # noqa: E402
from oracle.jvm import javasrc  # noqa: E402
from oracle.jvm.interp import VM, Box, HostEntry, JCollection  # noqa: E402

# stand-ins for JDK statics the interpreter has no host implementation of
interp.HOST_STATICS.setdefault(("java/lang/Double", "isInfinite"), lambda vm, v: int(math.isinf(v)))
# java.util.Arrays.binarySearch(int[], key) (SparseVector.contains): the whole-array form of the range search interp.py provides
interp.HOST_STATICS.setdefault(("java/util/Arrays", "binarySearch", "([II)I"), lambda vm, a, k: interp._binary_search(vm, a, 0, len(a.data), k))

DESC = "(Ljava/util/List;Ljava/util/List;)D"


def hexd(x):
    return float(x).hex()


def sims_bytecode(vm, method, a, b, median):
    A = JCollection([Box(float(x), "Double") for x in a])
    B = JCollection([Box(float(x), "Double") for x in b])
    name = {"cos": "cos", "msd": "msd", "cpc": "cpc", "exjaccard": "exJaccard", "pcc": "pcc"}[method]
    if method == "cpc":
        return vm.call("happy/coding/math/Sims", "cpc", "(Ljava/util/List;Ljava/util/List;D)D", [A, B, median])
    return vm.call("happy/coding/math/Sims", name, DESC, [A, B])


def matrix_pairs(name, limit=60, min_common=1):
    """pairs of columns (items) of the DePaul or Frappe 2-D matrix: the common lists in ascending user order, cell means over contexts"""
    import gzip
    from carskit_amd import dao
    tmp = tempfile.mkdtemp()
    if name == "depaul":
        shutil.copyfile(os.path.join(ROOT, "tests", "golden", "depaul_ratings_compact.csv"), os.path.join(tmp, "r.csv"))
    else:
        open(os.path.join(tmp, "r.csv"), "wb").write(gzip.open(os.path.join(ROOT, "tests", "golden", "frappe_compact.csv.gz"), "rb").read())
    dao.transform(os.path.join(tmp, "r.csv"), os.path.join(tmp, "train.csv"))
    d = dao.DataDAO(os.path.join(tmp, "train.csv")).rating_data()
    cells = {}
    for t in range(d.n):
        s, c = cells.get((int(d.u[t]), int(d.j[t])), (0.0, 0))
        cells[(int(d.u[t]), int(d.j[t]))] = (s + float(d.r[t]), c + 1)
    cols = {}
    for (u, j), (s, c) in sorted(cells.items()):
        cols.setdefault(j, []).append((u, s / c))
    items = sorted(cols, key=lambda j: -len(cols[j]))[:120] if name == "frappe" else sorted(cols)
    out = []
    for x in range(len(items)):
        for y in range(x + 1, len(items)):
            iv, jv = dict(cols[items[x]]), cols[items[y]]
            a = [iv[k] for k, _ in jv if k in iv]
            b = [v for k, v in jv if k in iv]
            if len(a) >= min_common:
                out.append((a, b))
            if len(out) >= limit:
                return out
    return out


class JdkHashMap:
    """java.util.HashMap<Integer, Double> of JDK 8: a table of bins (lists in insertion order).  putVal appends to its bin; a bin that
    reaches 9 nodes calls treeifyBin, which resizes a table below 64 slots (MIN_TREEIFY_CAPACITY) and builds a tree bin otherwise (not
    ported: refused); ++size > threshold resizes.  resize() doubles the table and threshold and splits every bin into the same index
    and index + oldCap keeping the relative order; clear() empties the bins and keeps the table."""
    JAVA_TYPES = ("java/util/Map", "java/util/HashMap")

    def __init__(self):
        self.table, self.threshold, self.size = None, 0, 0

    @staticmethod
    def hash(k):
        h = k & 0xFFFFFFFF
        return h ^ (h >> 16)

    def resize(self):
        old = self.table
        if old is None:
            cap, thr = 16, 12
        else:
            cap, thr = 2 * len(old), 2 * self.threshold
        new = [[] for _ in range(cap)]
        for b in old or []:
            for node in b:
                new[self.hash(node[0]) & (cap - 1)].append(node)
        self.table, self.threshold = new, thr

    def put(self, k, v):
        if self.table is None:
            self.resize()
        b = self.table[self.hash(k) & (len(self.table) - 1)]
        for node in b:
            if node[0] == k:
                old, node[1] = node[1], v
                return old
        b.append([k, v])
        if len(b) >= 9:                      # binCount >= TREEIFY_THRESHOLD - 1
            if len(self.table) < 64:
                self.resize()
            else:
                raise RuntimeError("treeifyBin: a tree bin (not ported)")
        self.size += 1
        if self.size > self.threshold:
            self.resize()
        return None

    def jcall(self, vm, name, desc, args):
        if name == "<init>":
            return None
        if name == "put":
            old = self.put(int(args[0].v), args[1])
            return old
        if name == "size":
            return self.size
        if name == "clear":
            for b in self.table or []:
                b.clear()
            self.size = 0
            return None
        if name == "entrySet":
            return JCollection([HostEntry(Box(k, "Integer"), v) for b in self.table or [] for k, v in b])
        raise KeyError("HashMap." + name)


class Conf:
    """Recommender.cf as correlation() reads it: getInt(key) = Integer.parseInt(value)"""

    def __init__(self, shrinkage):
        self.shrinkage = shrinkage

    def jcall(self, vm, name, desc, args):
        if name == "getInt":
            return int(self.shrinkage)
        raise KeyError("cf." + name)


class TwoD:
    """rateDao: toTraditionalSparseMatrix(trainMatrix) returns the prepared 2-D matrix"""

    def __init__(self, m):
        self.m = m

    def jcall(self, vm, name, desc, args):
        if name == "toTraditionalSparseMatrix":
            return self.m
        raise KeyError("rateDao." + name)


def knn_matrix():
    """users x items of the model runs: items 20..27 duplicate items 0..7 (ties), users 20..23 duplicate users 0..3, a dense block of
    40 items rated by users 0..11 (ItemKNN: 25+ candidates), an empty user (24) and an empty item (41)"""
    rng = np.random.default_rng(20261015)
    nu, ni = 26, 42
    cells = {}
    for u in range(20):
        for j in range(40):
            if (u < 12 and rng.random() < 0.85) or rng.random() < 0.3:
                cells[(u, j)] = float(rng.integers(1, 6)) / float(rng.integers(1, 4)) if rng.random() < 0.3 else float(rng.integers(1, 6))
    for (u, j), v in list(cells.items()):
        if 20 <= j < 28:
            cells.pop((u, j))
    for (u, j), v in list(cells.items()):
        if j < 8:
            cells[(u, j + 20)] = v
    for (u, j), v in list(cells.items()):
        if u < 4:
            cells[(u + 20, j)] = v
    for u in range(20, 24):
        cells.pop((u, 40), None)
        cells[(u, 40)] = 2.0
    cells[(25, 41 - 1)] = 4.0
    return nu, ni, sorted((u, j, v) for (u, j), v in cells.items())


def run_knn(ref, model, nu, ni, cells2, measure, shrinkage, knns, gm, min_rate=1.0, max_rate=5.0, predict=True):
    from oracle.mint_reference_src import CLASS_MAP, sparse
    javasrc.JHashMap = JdkHashMap   # `new HashMap<>()` in the interpreted predict()
    vm = VM([os.path.join(ref, "lib", "librec-v1.4-alpha.jar"), os.path.join(ref, "lib", "happy.coding.utils-1.2.6.jar")])
    src = [os.path.join(ref, "src", "carskit", "alg", "baseline", "cf", model + ".java"),
           os.path.join(ref, "src", "carskit", "generic", "Recommender.java")]
    this = javasrc.This(vm, src, dict(CLASS_MAP, Sims="happy/coding/math/Sims", Lists="happy/coding/io/Lists"))
    train2 = sparse(vm, nu, ni, cells2)
    this.fields.update({"train": None, "trainMatrix": None, "rateDao": TwoD(train2), "numUsers": nu, "numItems": ni, "globalMean": gm,
                        "knn": 0, "similarityMeasure": measure, "similarityShrinkage": shrinkage, "cf": Conf(shrinkage),
                        "isRankingPred": False, "isUserSplitting": False, "isItemSplitting": False, "isCARSRecommender": False,
                        "minRate": min_rate, "maxRate": max_rate, "algoName": model, "itemCorrs": None, "itemMeans": None,
                        "userCorrs": None, "userMeans": None})
    this.call("initModel", [])
    corrs = this.fields["itemCorrs" if model == "ItemKNN" else "userCorrs"]
    means = this.fields["itemMeans" if model == "ItemKNN" else "userMeans"]
    n = ni if model == "ItemKNN" else nu
    rec = {"model": model, "measure": measure, "shrinkage": shrinkage, "global_mean": hexd(gm),
           "corrs": [hexd(vm.call("librec/data/SymmMatrix", "get", "(II)D", [corrs, a, b])) for a in range(n) for b in range(a + 1, n)],
           "means": [hexd(x) for x in interp.to_list(means.fields["data"])]}
    if predict:
        rec["predict"] = {}
        for knn in knns:
            this.fields["knn"] = knn
            rec["predict"][str(knn)] = [[hexd(this.call("predict", [u, j, 0, True])) for j in range(ni)] for u in range(nu)]
    return rec


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CARSKIT_REFERENCE", "")
    vm = VM(os.path.join(ref, "lib", "happy.coding.utils-1.2.6.jar"))
    hand = [([3.0, 3.0], [3.0, 3.0]), ([3.0, 3.0], [3.0, 4.0]), ([2.0], [5.0]), ([], []), ([1.0, 2.0, 5.0], [1.0, 2.0, 5.0]),
            ([1.0, 5.0], [5.0, 1.0]), ([1e-170], [1e140]), ([-1e-170], [1e140]), ([5 / 3, 2.5, 4.0], [2.0, 7 / 3, 3.5])]
    cases = []
    for src, pairs in (("hand", hand), ("depaul", matrix_pairs("depaul")), ("frappe", matrix_pairs("frappe", 60, 2))):
        for a, b in pairs:
            rec = {"source": src, "a": [hexd(x) for x in a], "b": [hexd(x) for x in b], "median": hexd(3.0)}
            for m in ("pcc", "cos", "msd", "cpc", "exjaccard"):
                v = sims_bytecode(vm, m, a, b, 3.0)
                rec[m] = "nan" if isinstance(v, float) and math.isnan(v) else hexd(v)
            cases.append(rec)
    nu, ni, cells2 = knn_matrix()
    gm = 0.0
    for _, _, v in cells2:
        gm += v
    gm /= len(cells2)
    models = []
    for model in ("ItemKNN", "UserKNN"):
        for measure, shrinkage in (("PCC", -1), ("pcc", 30), ("cos", 30), ("cos", -1), ("COS-Binary", 30), ("cos-binary", -1), ("msd", -1),
                                   ("MSD", 30), ("cpc", 30), ("exjaccard", -1), ("exJaccard", 30), ("unknown-name", 30)):
            predict = (measure, shrinkage) in (("PCC", -1), ("cos", 30))
            models.append(run_knn(ref, model, nu, ni, cells2, measure, shrinkage, (0, 1, 5, 12, 1000), gm, predict=predict))
            print(model, measure, shrinkage, flush=True)
    out = {"source": "happy.coding.math.Sims from lib/happy.coding.utils-1.2.6.jar bytecode; ItemKNN / UserKNN / Recommender from source "
                     "(tests/tools/mint_reference_knn.py)",
           "cases": cases, "knn_matrix": {"n_users": nu, "n_items": ni, "cells": [[u, j, hexd(v)] for u, j, v in cells2]}, "models": models}
    import gzip
    path = os.path.join(ROOT, "tests", "golden", "reference_knn.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print("wrote", path, len(cases), "Sims cases,", len(models), "model runs")


if __name__ == "__main__":
    main()
