"""What the top-N tests of ItemKNN, UserKNN, SlopeOne and NMF share (test infrastructure): the decoded ranking-mode golden file, the
contextual splits over the golden matrices with their seeds, and the evaluation tuples of the kernel-edge tests."""
import functools
import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# check_rankings' three settings (tests/test_gpu_rankals.py)
SETTINGS = (dict(bin_thold=-1.0, num_recs=10), dict(bin_thold=-1.0, num_recs=5, strategy="uc"),
            dict(bin_thold=0.05, num_recs=10, num_ignore=3))
# the split's seed: with it every setting leaves at least one list for every golden model of the four baselines, on knn_matrix and on
# the handmade matrices (tests/test_knn_rank_ref.py checks that without a GPU)
SPLIT_SEED = 3


def _matrix(rows):
    return np.array([[float.fromhex(x) for x in row] for row in rows], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def knn_rank_runs():
    """the runs of tests/golden/reference_knn_rank.json.gz, decoded: name, kind, matrix (which), n_users, n_items, cells [(u, j, v)],
    u / i / r arrays, measure, shrinkage, global_mean, ranking {knn: (n_users, n_items) array}; the handmade runs also carry `corrs`
    (the upper triangle, 0.0 where nothing is stored), `means` and `witnesses`"""
    g = json.loads(gzip.open(os.path.join(GOLDEN, "reference_knn_rank.json.gz"), "rb").read())
    km = json.loads(gzip.open(os.path.join(GOLDEN, "reference_knn.json.gz"), "rb").read())["knn_matrix"]
    assert g["no_tuple_treeifies"] is True
    runs = []
    for which, mat, recs in (("knn_matrix", km, g["models"]), ("hand", g["hand_matrix"], g["hand"])):
        cells = [(int(c[0]), int(c[1]), float.fromhex(c[2])) for c in mat["cells"]]
        for rec in recs:
            run = {"name": "%s %s %s/%d" % (which, rec["model"], rec["measure"], rec["shrinkage"]), "matrix": which,
                   "kind": "item" if rec["model"] == "ItemKNN" else "user", "n_users": mat["n_users"], "n_items": mat["n_items"],
                   "cells": cells, "u": np.array([c[0] for c in cells], np.int32), "i": np.array([c[1] for c in cells], np.int32),
                   "r": np.array([c[2] for c in cells]), "measure": rec["measure"], "shrinkage": rec["shrinkage"],
                   "global_mean": float.fromhex(rec["global_mean"]),
                   "ranking": {int(k): _matrix(rows) for k, rows in rec["ranking"].items()}}
            if "corrs" in rec:
                run["corrs"] = np.array([float.fromhex(x) for x in rec["corrs"]])
                run["means"] = np.array([float.fromhex(x) for x in rec["means"]])
                run["witnesses"] = rec["witnesses"]
            runs.append(run)
    return runs


class Scored:
    """a handle as tests/test_gpu_rankals.check_rankings takes one: eval_rankings(train, test, **kw) with the model's own leading
    arguments (knn and global_mean, or global_mean) bound"""

    def __init__(self, h, *lead):
        self.h, self.lead, self.n_users, self.n_items = h, lead, h.n_users, h.n_items

    def eval_rankings(self, train, test, **kw):
        return self.h.eval_rankings(train, test, *self.lead, **kw)
