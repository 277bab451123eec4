#!/usr/bin/env python3
"""Mint tests/golden/reference_bpr.json.gz by EXECUTING the reference (no JVM: oracle/jvm interprets it).

BPR runs from its SOURCE (src/carskit/alg/baseline/ranking/BPR.java + generic/IterativeRecommender.java + generic/Recommender.java,
through oracle/jvm/javasrc.py) with librec's DenseMatrix / SparseMatrix / SparseVector and happy.coding's Randoms from the jars'
bytecode (SparseMatrix.row, SparseVector.getCount / getIndex / contains, DenseMatrix.rowMult / get / add, Randoms.seed / uniform(int)).

* buildModel() runs with P and Q injected from a seeded numpy draw (uniform(0, 1), stored in the file) and happy.coding's Randoms seeded
  with the run's seed.  buildModel has no per-iteration hook, so the state after iteration t is the state after a run with numIters = t
  from the same start and seed; t = 1, 2, 3 (bold driver off, no decay: lRate stays).  Per t the file holds P, Q, loss, the 48-bit state
  of the java.util.Random stream, and the triples of iteration t.  The triples are read off the log of what the run drew: every
  userCache.get(u) opens an attempt; the nextInt(bound) before it gave u, the first after it (if the row has entries) the slot of i in
  getIndex(), the last before the next attempt's u draw the accepted j.  predict(u, j) of every cell is recorded after the last run.
    - the 26 x 42 `knn_matrix` of tests/golden/reference_knn.json.gz (read from that file, not stored again) at k in {3, 10};
    - the 7 x 6 `handmade` matrix of tests/tools/mint_reference_rankals.py at k in {1, 2}: a stored zero, an empty user, a user whose
      only cell is a stored zero, a one-entry user.
  Per row the file records getCount(), len(getIndex()) and contains(j) of every item: a stored 0.0 is in neither, so is.length ==
  getCount(); contains misses entries of the upper half of a row whose count is no power of two.
* `init`: one IterativeRecommender.initModel() with initByNorm = false from librec's Randoms.seed(1) on 4 x 3, k = 2: P, Q.

Doubles are stored as float.hex().

Stand-ins (the JDK, Guava's cache and the configuration are not part of the interpreted sources):
* java.util.Random.nextInt(bound): the interpreter's HostRandom raises on it; here it is the published algorithm (the power-of-two
  branch, the rejection loop on bits - val + (bound - 1) < 0) over the already pinned next();
* Math.exp and Math.log: the fdlibm restatements of tests/bpr_ref.py (StrictMath's; Math's are specified to 1 ulp only);
* userCache.get(u): train.row(u), what the cache's loader returns.
The source interpreter has no do-while statement: BPR.java's one `do { S } while (C);` is handed to it as
`while (true) { S if (!(C)) break; }`, the same statement by the language's definition (S holds no break or continue); the rewrite
asserts that it changed exactly that text.

    python tests/tools/mint_reference_bpr.py /path/to/reference"""
import gzip
import json
import multiprocessing
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle.jvm import interp, javasrc  # noqa: E402
from oracle.jvm.interp import VM, to_list  # noqa: E402
from mint_reference_slopeone import TwoD, hexd  # noqa: E402
from mint_reference_rankals import handmade, flat  # noqa: E402
from tests import bpr_ref  # noqa: E402

ITERS = 3
SM, SV = "librec/data/SparseMatrix", "librec/data/SparseVector"
HC_RANDOMS = "happy/coding/math/Randoms"
LOG = []   # ("int", bound, value) and ("get", u) in the order the run made them


def f32(x):
    return float(np.float32(x))


class LoggedRandom(interp.HostRandom):
    """HostRandom plus nextInt(bound) from the published algorithm over its next()"""
    last = None

    def jcall(self, vm, name, desc, args):
        if name == "<init>":
            LoggedRandom.last = self
        if name == "nextInt" and args:
            bound = int(args[0])
            r = self.r.next(31)
            m = bound - 1
            if bound & m == 0:
                r = (bound * r) >> 31
            else:
                u = r
                while True:
                    r = u % bound
                    if ((u - r + m + (1 << 31)) & 0xFFFFFFFF) - (1 << 31) >= 0:
                        break
                    u = self.r.next(31)
            LOG.append(("int", bound, r))
            return r
        return super().jcall(vm, name, desc, args)


interp.HOST_CLASSES["java/util/Random"] = LoggedRandom
interp.HOST_STATICS.setdefault(("java/util/Arrays", "binarySearch", "([II)I"),
                               lambda vm, a, k: interp._binary_search(vm, a, 0, len(a.data), k))
javasrc.STATIC_CALLS[("Math", "exp")] = bpr_ref.fdlibm_exp
javasrc.STATIC_CALLS[("Math", "log")] = bpr_ref.fdlibm_log


class UserCache:
    """userCache: LoadingCache.get(u) = train.row(u)"""

    def __init__(self, vm, train):
        self.vm, self.train = vm, train

    def jcall(self, vm, name, desc, args):
        if name == "get":
            u = int(getattr(args[0], "v", args[0]))
            LOG.append(("get", u))
            return self.vm.call(SM, "row", "(I)L%s;" % SV, [self.train, u])
        raise KeyError("userCache." + name)


def without_do_while(path):
    """a temporary copy of BPR.java with its do-while written as a while (see the module's text)"""
    text = open(path).read()
    m = re.search(r"do \{\s*(j = Randoms\.uniform\(numItems\);)\s*\} while \((pu\.contains\(j\))\);", text)
    assert m and text.count("do {") == 1, "BPR.java's do-while is not where it was"
    text = text[:m.start()] + "while (true) { %s if (!(%s)) break; }" % (m.group(1), m.group(2)) + text[m.end():]
    out = os.path.join(tempfile.mkdtemp(prefix="mint_bpr_"), "BPR.java")
    with open(out, "w") as f:
        f.write(text)
    return out


def new_this(ref, with_bpr=True):
    from oracle.mint_reference_src import CLASS_MAP
    vm = VM([os.path.join(ref, "lib", "librec-v1.4-alpha.jar"), os.path.join(ref, "lib", "happy.coding.utils-1.2.6.jar")])
    src = [os.path.join(ref, "src", "carskit", "generic", "IterativeRecommender.java"),
           os.path.join(ref, "src", "carskit", "generic", "Recommender.java")]
    if with_bpr:
        src.insert(0, without_do_while(os.path.join(ref, "src", "carskit", "alg", "baseline", "ranking", "BPR.java")))
    cmap = dict(CLASS_MAP, SparseVector=SV, VectorEntry="librec/data/VectorEntry")
    if with_bpr:
        cmap["Randoms"] = HC_RANDOMS   # BPR.java imports happy.coding.math.Randoms
    return vm, javasrc.This(vm, src, cmap)


def triples_of(log, index):
    """the accepted (u, i, j) of every sample from the run's log; index[u] = getIndex() of train.row(u)"""
    gets = [p for p, e in enumerate(log) if e[0] == "get"]
    out = []
    for n, p in enumerate(gets):
        u = log[p][1]
        assert log[p - 1][0] == "int" and log[p - 1][2] == u
        if not index[u]:
            continue
        end = (gets[n + 1] - 1) if n + 1 < len(gets) else len(log)   # the next attempt's u draw, or the end of the run
        assert log[p + 1][1] == len(index[u]) and end - (p + 1) >= 2
        out.append((u, index[u][log[p + 1][2]], log[end - 1][2]))
    return out


def run_bpr(spec):
    ref, name, nu, ni, cells, k, seed, store_cells = spec
    from oracle.mint_reference_src import dense, sparse
    rng = np.random.default_rng(seed)
    P0, Q0 = rng.random((nu, k)), rng.random((ni, k))
    lrate, reg_u, reg_i = f32(0.05), f32(0.02), f32(0.03)
    rec = {"name": name, "n_users": nu, "n_items": ni, "k": k, "seed": seed, "lrate": hexd(lrate), "reg_u": hexd(reg_u),
           "reg_i": hexd(reg_i), "P0": [hexd(x) for x in P0.ravel()], "Q0": [hexd(x) for x in Q0.ravel()], "iters": []}
    this = None
    before = 0
    for t in range(1, ITERS + 1):
        vm, this = new_this(ref)
        train = sparse(vm, nu, ni, cells)
        rows = [vm.call(SM, "row", "(I)L%s;" % SV, [train, u]) for u in range(nu)]
        index = [[int(x) for x in to_list(vm.call(SV, "getIndex", "()[I", [r]))] for r in rows]
        if t == 1:
            rec["row_count"] = [int(vm.call(SV, "getCount", "()I", [r])) for r in rows]
            rec["index_len"] = [len(ix) for ix in index]
            rec["contains"] = [[int(bool(vm.call(SV, "contains", "(I)Z", [r, j]))) for j in range(ni)] for r in rows]
        this.fields.update({"train": train, "P": dense(vm, P0), "Q": dense(vm, Q0), "numFactors": k, "numIters": t, "numUsers": nu,
                            "numItems": ni, "lRate": lrate, "initLRate": lrate, "maxLRate": f32(-1.0), "decay": f32(-1.0),
                            "isBoldDriver": False, "regU": reg_u, "regI": reg_i, "loss": 0.0, "last_loss": 0.0, "measure": 0.0,
                            "last_measure": 0.0, "earlyStopMeasure": None, "verbose": False, "isResultsOut": False, "algoName": "BPR",
                            "foldInfo": "", "userCache": UserCache(vm, train), "__enums__": ("Measure",)})
        del LOG[:]
        vm.call(HC_RANDOMS, "seed", "(J)V", [seed])
        this.call("buildModel", [])
        tri = triples_of(LOG, index)
        assert len(tri) == t * nu * 100, (len(tri), t)
        rec["iters"].append({"P": flat(this.fields["P"]), "Q": flat(this.fields["Q"]), "loss": hexd(this.fields["loss"]),
                             "state": int(LoggedRandom.last.r.seed), "triples": [list(x) for x in tri[before:]]})
        before = len(tri)
    rec["predict"] = [[hexd(this.call("predict", [u, j])) for j in range(ni)] for u in range(nu)]
    if store_cells:
        rec["cells"] = [[u, j, hexd(v)] for u, j, v in cells]
    print(name, "k =", k, flush=True)
    return rec


def run_init(ref, nu, ni, k, seed):
    from oracle.mint_reference_src import sparse
    vm, this = new_this(ref, with_bpr=False)
    cells = [(u, j, 1.0 + (u + j) % 4) for u in range(nu) for j in range(ni) if (u + 2 * j) % 3]
    this.fields.update({"train": None, "trainMatrix": None, "rateDao": TwoD(sparse(vm, nu, ni, cells)), "numUsers": nu, "numItems": ni,
                        "numFactors": k, "initByNorm": False, "initMean": 0.0, "initStd": 0.1, "isUserSplitting": False,
                        "isItemSplitting": False, "isCARSRecommender": False, "P": None, "Q": None})
    vm.call("librec/util/Randoms", "seed", "(J)V", [seed])
    this.call("initModel", [])
    return {"seed": seed, "n_users": nu, "n_items": ni, "k": k, "P": flat(this.fields["P"]), "Q": flat(this.fields["Q"])}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CARSKIT_REFERENCE", "")
    km = json.loads(gzip.open(os.path.join(ROOT, "tests", "golden", "reference_knn.json.gz"), "rb").read())["knn_matrix"]
    kcells = [(u, j, float.fromhex(v)) for u, j, v in km["cells"]]
    nu, ni, hcells = handmade()
    specs = [(ref, "handmade", nu, ni, hcells, 1, 20261201, True), (ref, "handmade", nu, ni, hcells, 2, 20261202, True),
             (ref, "knn_matrix", km["n_users"], km["n_items"], kcells, 3, 20261203, False),
             (ref, "knn_matrix", km["n_users"], km["n_items"], kcells, 10, 20261204, False)]
    if len(sys.argv) > 2:   # a subset of the runs, to try the tool
        specs = [specs[int(x)] for x in sys.argv[2].split(",")]
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        runs = pool.map(run_bpr, specs, chunksize=1)
    out = {"source": "BPR / IterativeRecommender / Recommender from source, librec DenseMatrix / SparseMatrix / SparseVector from "
                     "lib/librec-v1.4-alpha.jar and happy.coding Randoms from lib/happy.coding.utils-1.2.6.jar bytecode; Math.exp / "
                     "Math.log = fdlibm (tests/tools/mint_reference_bpr.py)",
           "runs": runs, "init": run_init(ref, 4, 3, 2, 1)}
    path = os.path.join(ROOT, "tests", "golden", "reference_bpr.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print("wrote", path, len(runs), "runs", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
