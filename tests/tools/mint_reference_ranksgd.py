#!/usr/bin/env python3
"""Mint tests/golden/reference_ranksgd.json.gz by EXECUTING the reference (no JVM: oracle/jvm interprets it).

RankSGD runs from its SOURCE (src/carskit/alg/baseline/ranking/RankSGD.java + generic/IterativeRecommender.java +
generic/Recommender.java, through oracle/jvm/javasrc.py) with librec's DenseMatrix / SparseMatrix / SparseVector and happy.coding's
Randoms (random -> uniform() -> uniform(0.0, 1.0) -> Random.nextDouble) and Lists (sortMap, Lists$1.compare) from the jars' bytecode.

numRates.  Recommender.java:141 declares `numRates`; NO source file of the reference assigns it, so RankSGD.java:71 divides by 0:
prob = +Infinity for every item with a cell, NaN (not put) for the others.  The list is then the HashMap's own iteration order, the
first running sum is +Infinity, every try returns the list's first item, and a user whose row contains() it loops for ever.  LibRec's
RankSGD (which the file says it was modified from) has numRates = trainMatrix.size().  The file holds both, labelled per run:
  * "num_rates": "reference" -- the field as the reference leaves it (0).  One full run, on the `escape` matrix below, where the loop
    ends: the list's first item (32) is held by one user only, in the upper half of a row of 5, where contains() misses it; that
    user's cell on item 32 is a sample with j == i.  For every other matrix the item list alone (`lists`): buildModel would not end.
  * "num_rates": "size" -- the field injected as train.size() before initModel: RankSGD.java's own code on a list with finite
    probabilities (the sort, the running sums, rejections).  This is NOT what the reference computes; it pins the source's statements.
    - the 26 x 42 `knn_matrix` of tests/golden/reference_knn.json.gz (read from that file, not stored again) at k in {3, 10};
    - the 7 x 6 `handmade` matrix of tests/tools/mint_reference_rankals.py at k in {1, 2};
    - `ties`, 6 x 40: nine items whose ids collide in a 16-slot table (1, 17, 33, 2, 18, 34, 3, 19, 35), seven of them with two
      cells each, so the sorted list is not in ascending-id order (asserted below).

Per run: initModel() runs as it stands (super.initModel() draws P and Q, then the item list is built); the file records the list (keys,
probabilities), rows(), size() and columnSize(j) of the matrix.  P and Q are then replaced by a seeded numpy draw (gaussian, std 0.1,
stored).  buildModel has no per-iteration hook, so the state after iteration t is the state after a run with numIters = t from the
same start and seed; t = 1, 2, 3 (bold driver off, no decay).  Per t: P, Q, loss, the 48-bit state of the stream, every random() value
of iteration t (packed: see pack53; the two knn_matrix runs share a seed and so a stream, stored
once: `randoms_as` names the run that holds it) and the accepted j per cell (the second argument of every second predict(u, .) call).
`init`: one IterativeRecommender.initModel() with initByNorm = true from librec's Randoms.seed(1) on 4 x 3, k = 2: P, Q.

Doubles are stored as float.hex().

Stand-ins (the JDK and the configuration are not part of the interpreted sources): java.util.HashMap is javasrc's JHashMap (the JDK 8
iteration order); its entrySet(), which the interpreter lacks, is added here as that order's (key, value) entries; ArrayList(Collection)
copies in iteration order; Collections.sort is a stable sort under Lists$1.compare; rateDao.toTraditionalSparseMatrix returns the 2-D
matrix the caller built (DataDAO.java:1241-1257 builds it with the same Table / Multimap constructor).

    python tests/tools/mint_reference_ranksgd.py /path/to/reference"""
import base64
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
from oracle.jvm.interp import VM, Box, HostEntry, JCollection, to_list  # noqa: E402
from mint_reference_slopeone import TwoD, hexd  # noqa: E402
from mint_reference_rankals import handmade, flat  # noqa: E402

ITERS = 3
SM, SV = "librec/data/SparseMatrix", "librec/data/SparseVector"
HC_RANDOMS = "happy/coding/math/Randoms"
LOG = []   # every nextDouble() in the order the run made them


class LoggedRandom(interp.HostRandom):
    last = None

    def jcall(self, vm, name, desc, args):
        if name == "<init>":
            LoggedRandom.last = self
        r = super().jcall(vm, name, desc, args)
        if name == "nextDouble":
            LOG.append(r)
        return r


interp.HOST_CLASSES["java/util/Random"] = LoggedRandom
interp.HOST_STATICS.setdefault(("java/util/Arrays", "binarySearch", "([II)I"),
                               lambda vm, a, k: interp._binary_search(vm, a, 0, len(a.data), k))

_jhashmap_jcall = javasrc.JHashMap.jcall


def _jhashmap_with_entry_set(self, vm, name, desc, args):
    if name == "entrySet":
        return JCollection([HostEntry(k, self.d[k]) for k in self._ordered()])
    return _jhashmap_jcall(self, vm, name, desc, args)


javasrc.JHashMap.jcall = _jhashmap_with_entry_set


def pack53(values):
    """random() values are multiples of 2^-53 below 1: [count, base64 of the 53-bit integers packed from the low end]"""
    big = 0
    for t, x in enumerate(values):
        m = int(x * 9007199254740992.0)
        assert 0 <= m < 1 << 53 and m / 9007199254740992.0 == x
        big |= m << (53 * t)
    return [len(values), base64.b64encode(big.to_bytes((53 * len(values) + 7) // 8, "little")).decode()]


def f32(x):
    return float(np.float32(x))


def ties():
    rows = {0: [1, 17, 33, 2], 1: [17, 2, 18, 34], 2: [33, 3, 19], 3: [1, 35, 18], 4: [2, 3], 5: [19, 35, 34, 1]}
    return 6, 40, [(u, j, 1.0 + (u + j) % 5) for u, js in rows.items() for j in js]


def escape():
    rows = {0: [17, 18, 19, 20, 32], 1: [17, 18], 2: [19], 3: [20, 33]}
    return 5, 40, [(u, j, 1.0 + (u + 2 * j) % 4) for u, js in rows.items() for j in js]


def new_this(ref, with_ranksgd=True):
    from oracle.mint_reference_src import CLASS_MAP
    vm = VM([os.path.join(ref, "lib", "librec-v1.4-alpha.jar"), os.path.join(ref, "lib", "happy.coding.utils-1.2.6.jar")])
    src = [os.path.join(ref, "src", "carskit", "generic", "IterativeRecommender.java"),
           os.path.join(ref, "src", "carskit", "generic", "Recommender.java")]
    cmap = dict(CLASS_MAP, SparseVector=SV, VectorEntry="librec/data/VectorEntry")
    if with_ranksgd:
        src.insert(0, os.path.join(ref, "src", "carskit", "alg", "baseline", "ranking", "RankSGD.java"))
        cmap["Randoms"] = HC_RANDOMS   # RankSGD.java imports happy.coding.math.Randoms ...
        cmap["Lists"] = "happy/coding/io/Lists"
    return vm, javasrc.This(vm, src, cmap)


def ints(c):
    return [int(x.v if isinstance(x, Box) else x) for x in (c.items if hasattr(c, "items") else to_list(c))]


def prepared(ref, nu, ni, cells, k, t, lrate, num_rates, seed):
    """a RankSGD after its own initModel(); returns (vm, this, train)"""
    from oracle.mint_reference_src import sparse
    vm, this = new_this(ref)
    train = sparse(vm, nu, ni, cells)
    fields = {"train": None, "trainMatrix": None, "rateDao": TwoD(train), "numFactors": k, "numIters": t, "numUsers": nu,
              "numItems": ni, "initByNorm": True, "initMean": 0.0, "initStd": 0.1, "isUserSplitting": False,
              "isItemSplitting": False, "isCARSRecommender": False, "P": None, "Q": None, "itemProbs": None,
              "lRate": lrate, "initLRate": lrate, "maxLRate": f32(-1.0), "decay": f32(-1.0), "isBoldDriver": False,
              "loss": 0.0, "last_loss": 0.0, "measure": 0.0, "last_measure": 0.0, "earlyStopMeasure": None, "verbose": False,
              "isResultsOut": False, "algoName": "RankSGD", "foldInfo": "", "__enums__": ("Measure",)}
    # `protected int numUsers, numItems, numRates;` and nothing else: the field keeps Java's default unless the run injects size()
    fields["numRates"] = int(vm.call(SM, "size", "()I", [train])) if num_rates == "size" else 0
    this.fields.update(fields)
    vm.call("librec/util/Randoms", "seed", "(J)V", [seed])
    this.call("initModel", [])
    return vm, this, this.fields["train"]


def item_list(this):
    ents = this.fields["itemProbs"].items
    return [int(e.k.v) for e in ents], [hexd(e.v.v) for e in ents]


def matrix_facts(vm, train, ni):
    return {"rows": ints(vm.call(SM, "rows", "()Ljava/util/List;", [train])), "size": int(vm.call(SM, "size", "()I", [train])),
            "column_size": [int(vm.call(SM, "columnSize", "(I)I", [train, j])) for j in range(ni)]}


def run_ranksgd(spec):
    ref, name, nu, ni, cells, k, seed, num_rates, store_cells = spec
    from oracle.mint_reference_src import dense
    rng = np.random.default_rng(seed)
    P0, Q0 = 0.1 * rng.standard_normal((nu, k)), 0.1 * rng.standard_normal((ni, k))
    lrate = f32(0.05)
    rec = {"name": name, "n_users": nu, "n_items": ni, "k": k, "seed": seed, "num_rates": num_rates, "lrate": hexd(lrate),
           "P0": [hexd(x) for x in P0.ravel()], "Q0": [hexd(x) for x in Q0.ravel()], "iters": []}
    before_r = before_j = 0
    for t in range(1, ITERS + 1):
        vm, this, train = prepared(ref, nu, ni, cells, k, t, lrate, num_rates, seed)
        if t == 1:
            rec["items"], rec["probs"] = item_list(this)
            rec["num_rates_value"] = int(this.fields["numRates"])
            rec.update(matrix_facts(vm, train, ni))
        this.fields["P"], this.fields["Q"] = dense(vm, P0), dense(vm, Q0)
        preds = []
        inner = this.call

        def call(name_, args, *a, _inner=inner, _preds=preds, **kw):
            if name_ == "predict" and len(args) == 2:
                _preds.append((int(javasrc.unbox(args[0])), int(javasrc.unbox(args[1]))))
            return _inner(name_, args, *a, **kw)
        this.call = call
        del LOG[:]
        vm.call(HC_RANDOMS, "seed", "(J)V", [seed])
        this.call("buildModel", [])
        this.call = inner
        nz = sorted((u, j) for u, j, v in cells if v != 0.0)
        assert len(preds) == 2 * t * len(nz), (len(preds), t, len(nz))
        for c in range(t * len(nz)):
            assert preds[2 * c] == nz[c % len(nz)] and preds[2 * c + 1][0] == nz[c % len(nz)][0]
        js = [preds[2 * c + 1][1] for c in range(t * len(nz))]
        rec["iters"].append({"P": flat(this.fields["P"]), "Q": flat(this.fields["Q"]), "loss": hexd(this.fields["loss"]),
                             "state": int(LoggedRandom.last.r.seed), "j": js[before_j:], "randoms": pack53(LOG[before_r:])})
        before_j, before_r = len(js), len(LOG)
    if store_cells:
        rec["cells"] = [[u, j, hexd(v)] for u, j, v in cells]
    print(name, "k =", k, num_rates, flush=True)
    return rec


def run_list(ref, name, nu, ni, cells):
    """the item list of the reference as it stands (numRates = 0) on a matrix where buildModel would not end"""
    vm, this, train = prepared(ref, nu, ni, cells, 1, 1, f32(0.05), "reference", 1)
    items, probs = item_list(this)
    rec = {"name": name, "n_users": nu, "n_items": ni, "num_rates_value": int(this.fields["numRates"]), "items": items, "probs": probs}
    rec.update(matrix_facts(vm, train, ni))
    return rec


def run_init(ref, nu, ni, k, seed):
    from oracle.mint_reference_src import sparse
    vm, this = new_this(ref, with_ranksgd=False)
    cells = [(u, j, 1.0 + (u + j) % 4) for u in range(nu) for j in range(ni) if (u + 2 * j) % 3]
    this.fields.update({"train": None, "trainMatrix": None, "rateDao": TwoD(sparse(vm, nu, ni, cells)), "numUsers": nu, "numItems": ni,
                        "numFactors": k, "initByNorm": True, "initMean": 0.0, "initStd": 0.1, "isUserSplitting": False,
                        "isItemSplitting": False, "isCARSRecommender": False, "P": None, "Q": None})
    vm.call("librec/util/Randoms", "seed", "(J)V", [seed])
    this.call("initModel", [])
    return {"seed": seed, "n_users": nu, "n_items": ni, "k": k, "P": flat(this.fields["P"]), "Q": flat(this.fields["Q"])}


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("CARSKIT_REFERENCE", "")
    km = json.loads(gzip.open(os.path.join(ROOT, "tests", "golden", "reference_knn.json.gz"), "rb").read())["knn_matrix"]
    kcells = [(u, j, float.fromhex(v)) for u, j, v in km["cells"]]
    nu, ni, hcells = handmade()
    tu, ti, tcells = ties()
    eu, ei, ecells = escape()
    specs = [(ref, "escape", eu, ei, ecells, 2, 20270300, "reference", True),
             (ref, "handmade", nu, ni, hcells, 1, 20270301, "size", True), (ref, "handmade", nu, ni, hcells, 2, 20270302, "size", True),
             (ref, "ties", tu, ti, tcells, 2, 20270305, "size", True),
             (ref, "knn_matrix", km["n_users"], km["n_items"], kcells, 3, 20270303, "size", False),
             (ref, "knn_matrix", km["n_users"], km["n_items"], kcells, 10, 20270303, "size", False)]
    if len(sys.argv) > 2:   # a subset of the runs, to try the tool
        specs = [specs[int(x)] for x in sys.argv[2].split(",")]
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        runs = pool.map(run_ranksgd, specs, chunksize=1)
    for n, r in enumerate(runs):   # the two knn_matrix runs share a seed, so one stream: its values are stored once
        for e in range(n):
            if all(a["randoms"] == b["randoms"] for a, b in zip(runs[e]["iters"], r["iters"])):
                for it in r["iters"]:
                    del it["randoms"]
                r["randoms_as"] = e
                break
    lists = [run_list(ref, "handmade", nu, ni, hcells), run_list(ref, "ties", tu, ti, tcells),
             run_list(ref, "knn_matrix", km["n_users"], km["n_items"], kcells)]
    for r in runs + lists:   # the ties list must not be in ascending-id order
        if r["name"] == "ties":
            assert r["items"] != sorted(r["items"]), r["items"]
    out = {"source": "RankSGD / IterativeRecommender / Recommender from source, librec DenseMatrix / SparseMatrix / SparseVector from "
                     "lib/librec-v1.4-alpha.jar and happy.coding Randoms / Lists from lib/happy.coding.utils-1.2.6.jar bytecode "
                     "(tests/tools/mint_reference_ranksgd.py).  num_rates 'reference': the field as the reference leaves it (0); "
                     "'size': injected as train.size(), not what the reference computes",
           "runs": runs, "lists": lists, "init": run_init(ref, 4, 3, 2, 1)}
    path = os.path.join(ROOT, "tests", "golden", "reference_ranksgd.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print("wrote", path, len(runs), "runs", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
