"""CPU restatement of the reference's SLIM (src/carskit/alg/baseline/ranking/SLIM.java; test infrastructure, never imported by
carskit_amd/ or tools/).

* `Slim(n_users, n_items, cells)`: the 2-D train matrix.  A stored 0.0 takes no part anywhere: SparseMatrix.row() / column() leave it
  out and get() returns the same 0.0 as for an absent cell.
* `neighbors(knn, ...)`: initModel's lists in the order everything after walks them.  knn > 0: per item j the row of buildCorrs(false)
  (ascending index; a similarity of 0.0 or NaN is not in it, negative ones are) goes into a java.util.HashMap; if knn < size it is cut
  as in ItemKNN.predict (Lists.sortMap descending and stable over the map's entry order, the first knn, clear() keeps the table, re-put);
  the survivors go, in the map's entry order, into the multimap's value set: a java.util.HashSet made by
  Sets.newHashSetWithExpectedSize(2) = new HashSet(3), a 4-slot table that grows 4 -> 8 -> 16 -> ... at load 0.75.  knn <= 0: every list
  is train.columns(), the items with a live entry, ascending, j itself included.  `treeified` counts the lists whose map or set would
  have treeified a bin (their order is not modelled; they come back in the order reached).
* `iterate(nbr, W, l1, l2)`: one pass of buildModel's loop body over W (one array per list, aligned with it); returns the loss.
  l1, l2 are the doubles of Java's floats (`f32`).
* `predict(nbr, W, u, j)`: SLIM.predict(u, j).
"""
import gzip
import json
import os
import struct

import numpy as np

from tests import knn_ref, nmf_ref


def f32(x):
    """a Java float widened to double"""
    return struct.unpack("f", struct.pack("f", x))[0]


class JavaIntHashSet(knn_ref.JavaIntHashMap):
    """the java.util.HashSet<Integer> of guava's HashMultimap: new HashSet(3) -> HashMap(3) -> a 4-slot table, threshold 3"""

    def __init__(self):
        super().__init__()
        self.cap, self.thr = 4, 3


def cut_neighbors(sims, knn):
    """SLIM.java:96-109 for one item: `sims` its row of the similarity matrix (NaN unset).  Raises knn_ref.Treeified."""
    nns = knn_ref.JavaIntHashMap()
    for i, s in enumerate(sims):
        if s == s and s != 0.0:
            nns.put(i, float(s))
    if knn < len(nns):
        srt = sorted(nns.items(), key=lambda kv: -kv[1])
        nns.clear()
        for k, v in srt[:knn]:
            nns.put(k, v)
    vals = JavaIntHashSet()
    for k, _ in nns.items():
        vals.put(k, 0.0)
    return [k for k, _ in vals.items()]


class Slim:
    def __init__(self, n_users, n_items, cells):
        self.nu, self.ni = n_users, n_items
        live = sorted((int(u), int(j), float(v)) for u, j, v in cells if float(v) != 0.0)
        self.rows = [[] for _ in range(n_users)]   # user -> ascending (item, value)
        self.cols = [[] for _ in range(n_items)]   # item -> ascending (user, value)
        for u, j, v in live:
            self.rows[u].append((j, v))
            self.cols[j].append((u, v))
        self.val = {(u, j): v for u, j, v in live}
        # Ru.contains(k) for the entries of every row: SparseVector.contains' whole-capacity search
        self.found = [{k: f for (k, _), f in zip(row, knn_ref.findable(row))} for row in self.rows]
        self.treeified = 0
        self._pos = {}  # the position map of the list _matches saw last

    def neighbors(self, knn, measure="pcc", shrinkage=-1, min_rate=1.0, max_rate=5.0):
        self.treeified = 0
        if knn <= 0:
            all_items = [j for j in range(self.ni) if self.cols[j]]
            return [all_items] * self.ni  # (one object: _matches keeps one position map for it)
        S = knn_ref.build_corrs(self.cols, self.nu, measure, shrinkage, min_rate, max_rate)
        out = []
        for j in range(self.ni):
            try:
                out.append(cut_neighbors(S[j], knn))
            except knn_ref.Treeified:
                self.treeified += 1
                out.append([])
        return out

    def _matches(self, u, lst):
        """the positions s of lst with Ru.contains(lst[s]), in list order, with Ru.get(lst[s])"""
        if len(lst) <= len(self.rows[u]):
            found, val = self.found[u], self.val
            return [(s, val[(u, k)]) for s, k in enumerate(lst) if found.get(k, False)]
        pos = self._pos.get(id(lst))  # a list longer than the row: from the row's side, put back into list order
        if pos is None:
            self._pos = {id(lst): {k: s for s, k in enumerate(lst)}}
            pos = self._pos[id(lst)]
        found = self.found[u]
        return sorted((pos[k], v) for k, v in self.rows[u] if found[k] and k in pos)

    def iterate(self, nbr, W, l1, l2):
        loss, nan = 0.0, float("nan")
        cols, val_get = self.cols, self.val.get
        for j in range(self.ni):
            lst, w = nbr[j], [float(x) for x in W[j]]  # plain floats: the same IEEE arithmetic, without numpy's scalar overhead
            match = {}  # per user of this column's sweep: the terms of predict(u, j, ...), which do not depend on the coordinate
            for t, i in enumerate(lst):
                grad = rate = errs = 0.0
                for u, rui in cols[i]:
                    m = match.get(u)
                    if m is None:
                        m = match[u] = self._matches(u, lst)
                    pred = 0.0
                    for s, ruk in m:
                        if s != t:
                            pred += ruk * w[s]
                    e = val_get((u, j), 0.0) - pred
                    grad += rui * e
                    rate += rui * rui
                    errs += e * e
                n = float(len(cols[i]))
                if n:
                    grad, rate, errs = grad / n, rate / n, errs / n
                else:  # 0.0 / 0
                    grad = rate = errs = nan
                wij = w[t]
                loss += errs + 0.5 * l2 * wij * wij + l1 * wij
                if l1 < abs(grad):
                    w[t] = knn_ref._div(grad - l1 if grad > 0 else grad + l1, l2 + rate)
                else:
                    w[t] = 0.0
            W[j][:] = w
        return loss

    def predict(self, nbr, W, u, j):
        pred = 0.0
        for s, ruk in self._matches(u, nbr[j]):
            if nbr[j][s] != j:
                pred += ruk * W[j][s]
        return pred

    def scores(self, nbr, W):
        return np.array([[self.predict(nbr, W, u, j) for j in range(self.ni)] for u in range(self.nu)])


def init_weights(rnd, n_users, n_items, k, nbr):
    """SLIM.initModel()'s W from a tests.hostmirror.javarand.JavaRandom stream: IterativeRecommender.initModel draws P and Q gaussian
    first (unused, but they move the stream), then W.init(): n_items^2 uniform draws, row by row; the diagonal is set to 0.  Returns the
    listed cells, one array per list: W[j][t] = W[nbr[j][t]][j]."""
    nmf_ref.skip_gaussians(rnd, (n_users + n_items) * k)
    dense = np.array(rnd.doubles(n_items * n_items)).reshape(n_items, n_items)
    np.fill_diagonal(dense, 0.0)
    return [np.array([dense[i, j] for i in nbr[j]], dtype=np.float64) for j in range(n_items)]


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INIT_FACTORS = 2  # num.factors of the minted runs (P and Q's draws)


def golden():
    return json.loads(gzip.open(os.path.join(GOLDEN, "reference_slim.json.gz"), "rb").read())


def golden_runs():
    """the runs of tests/golden/reference_slim.json.gz, decoded: cells, neighbors, W0 / W[iteration] as lists of arrays aligned with the
    neighbour lists, loss per iteration, predict (n_users x n_items)"""
    g = golden()
    knn = json.loads(gzip.open(os.path.join(GOLDEN, "reference_knn.json.gz"), "rb").read())["knn_matrix"]
    mats = {"knn_matrix": knn, "edge_matrix": g["edge_matrix"]}
    dec = lambda rows: [np.array([float.fromhex(x) for x in row], dtype=np.float64) for row in rows]  # noqa: E731
    runs = []
    for run in g["runs"]:
        m = mats[run["name"]]
        assert (run["n_users"], run["n_items"]) == (m["n_users"], m["n_items"])
        runs.append({"name": "%s knn=%d l1=%g l2=%g" % (run["name"], run["knn"], run["l1"], run["l2"]), "matrix": run["name"],
                     "n_users": run["n_users"], "n_items": run["n_items"], "knn": run["knn"], "l1": f32(run["l1"]), "l2": f32(run["l2"]),
                     "measure": run["measure"], "shrinkage": run["shrinkage"],
                     "cells": [(c[0], c[1], float.fromhex(c[2])) for c in m["cells"]], "neighbors": run["neighbors"],
                     "W0": dec(run["W0"]), "W": {int(k): dec(v) for k, v in run["W"].items()},
                     "loss": [float.fromhex(x) for x in run["loss"]],
                     "predict": np.array([[float.fromhex(x) for x in row] for row in run["predict"]])})
    return runs
