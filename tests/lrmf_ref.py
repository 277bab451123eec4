"""CPU restatement of the reference's LRMF (src/carskit/alg/baseline/ranking/LRMF.java; test infrastructure, never imported by
carskit_amd/; tools/bench_lrmf.py times it beside the device), in the reference's operation order, in IEEE doubles without FMA.  Pinned
to the reference's own source by tests/golden/reference_lrmf.json.gz (tests/test_lrmf_ref.py).

    m = LRMF(n_users, n_items, cells)  # the 2-D train matrix: m.cells (iterator order), m.columns[u] (getColumns), m.user_exp
    loss = m.epoch(P, Q, lrate, reg_u, reg_i, terms=None)   # LRMF.java:75-104 over every MatrixEntry, in place on lists of lists
    loss, terms = m.epoch_np(P, Q, lrate, reg_u, reg_i, users=None)   # the same bits on numpy arrays (numpy only across the
                                       # INDEPENDENT items of one cell's sum; every chain stays a chain)
    levels(n_users, n_items, cells)    # the level of every user's unit
    exp_vec(x)                         # fdlibm exp of an array, element for element tests/bpr_ref.fdlibm_exp

What librec's SparseMatrix makes of the cells (recorded in the golden file): the matrix iterator yields a stored 0.0 -- the cell adds
exp(0) = 1 to userExp[u] and updates P[u] and Q[j] -- but getColumns(u) leaves it out, so its exp(pred) is no part of uexp.  A user whose
only cell is a stored 0.0 has uexp = 0.0: B = +Inf and the model goes non-finite, as in the reference."""
import gzip
import json
import math
import os

import numpy as np

from tests.bpr_ref import fdlibm_exp, fdlibm_log, unhex

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def jdiv(a, b):
    """Java's double division: x / 0.0 is an infinity or NaN, never an exception"""
    if b != 0.0:
        return a / b
    if a != a or a == 0.0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def g(x):
    """Recommender.java:1140-1142: 1.0 / (1 + Math.exp(-x))"""
    return jdiv(1.0, 1 + fdlibm_exp(-x))


def gd(x):
    """Recommender.java:1147-1149: g(x) * g(-x)"""
    return g(x) * g(-x)


def exp_vec(x):
    """fdlibm __ieee754_exp of every element of an array: the branches of tests/bpr_ref.fdlibm_exp as masks; the arguments near or past
    the overflow / underflow region (|x| >= 700, infinities, NaN) go through the scalar function"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    ln2HI, ln2LO, invln2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00
    P1, P2, P3, P4, P5 = (1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05,
                          -1.65339022054652515390e-06, 4.13813679705723846039e-08)
    hx = ((x.view(np.uint64) >> np.uint64(32)) & np.uint64(0x7FFFFFFF)).astype(np.int64)
    neg = np.signbit(x)
    far = hx >= 0x4085E000                                            # |x| >= 700: the scaled-result and saturation paths
    tiny = hx < 0x3E300000
    with np.errstate(all="ignore"):
        big = hx > 0x3FD62E42
        near = big & (hx < 0x3FF0A2B2)
        k = np.where(near, np.where(neg, -1, 1), np.where(big, np.trunc(invln2 * x + np.where(neg, -0.5, 0.5)), 0.0)).astype(np.int64)
        k = np.where(far, 0, k)
        t = k.astype(np.float64)
        hi = np.where(near, x - np.where(neg, -ln2HI, ln2HI), x - t * ln2HI)
        lo = np.where(near, np.where(neg, -ln2LO, ln2LO), t * ln2LO)
        r = np.where(big, hi - lo, x)
        tt = r * r
        c = r - tt * (P1 + tt * (P2 + tt * (P3 + tt * (P4 + tt * P5))))
        y0 = 1.0 - ((r * c) / (c - 2.0) - r)
        y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi)
        scaled = (y.view(np.int64) + (k << 52)).view(np.float64)     # hy + (k << 20): k >= -1021 away from the far region
        out = np.where(k == 0, y0, scaled)
        out = np.where(tiny, 1.0 + x, out)
    for p in np.nonzero(far)[0].tolist():
        out[p] = fdlibm_exp(float(x[p]))
    return out


def _chain(v):
    """0.0 + v[0] + v[1] + ... left to right (np.add.accumulate is sequential)"""
    return float(np.add.accumulate(np.concatenate([[0.0], v]))[-1])


class LRMF:
    def __init__(self, n_users, n_items, cells):
        self.n_users, self.n_items = n_users, n_items
        self.cells = sorted((int(u), int(j), float(r)) for u, j, r in cells)          # the MatrixEntry iterator: rows, then columns
        self.columns = [[] for _ in range(n_users)]                                   # getColumns(u): without the stored zeros
        self.stored = [[] for _ in range(n_users)]                                    # every stored column of the row
        self.user_exp = [0.0] * n_users                                               # LRMF.java:59-65
        for u, j, r in self.cells:
            self.stored[u].append(j)
            if r != 0.0:
                self.columns[u].append(j)
            self.user_exp[u] += fdlibm_exp(r)

    def epoch(self, P, Q, lrate, reg_u, reg_i, terms=None, users=None):
        """LRMF.java:74-104, in place on the lists of lists P and Q; returns the loss, one chain over every cell's 1 + k terms (the first
        one negated, as `terms` receives them).  users: only these users' cells (see epoch_np)"""
        loss = 0.0
        k = len(P[0])
        only = None if users is None else set(users)
        for u, j, r in self.cells:
            if only is not None and u not in only:
                continue
            pu, qj = P[u], Q[j]
            pred = 0.0
            for f in range(k):
                pred += pu[f] * qj[f]
            uexp = 0.0
            for i in self.columns[u]:
                qi, d = Q[i], 0.0
                for f in range(k):
                    d += pu[f] * qi[f]
                uexp += fdlibm_exp(d)
            A = jdiv(fdlibm_exp(r), self.user_exp[u])
            B = jdiv(fdlibm_exp(pred), uexp)
            out = [-(A * fdlibm_log(B))]
            loss -= A * fdlibm_log(B)
            d = (A - B) * gd(pred)
            for f in range(k):
                puf, qjf = pu[f], qj[f]
                pu[f] += lrate * (d * qjf - reg_u * puf)
                qj[f] += lrate * (d * puf - reg_i * qjf)
                t = 0.5 * reg_u * puf * puf + 0.5 * reg_i * qjf * qjf
                loss += t
                out.append(t)
            if terms is not None:
                terms.extend(out)
        return loss

    def epoch_np(self, P, Q, lrate, reg_u, reg_i, users=None):
        """the same iteration on numpy arrays (in place): the dots of one cell's sum are independent of one another, so numpy forms
        them side by side, each as one chain along the factors; uexp and the loss stay chains.  users: only these users' cells (the
        rows they touch then equal a full epoch's only if no other user shares them).  Returns (loss, terms): terms in (cell, term)
        order"""
        k = P.shape[1]
        only = None if users is None else set(users)
        terms = []
        for u, j, r in self.cells:
            if only is not None and u not in only:
                continue
            pu, qj = P[u].copy(), Q[j].copy()
            pred = _chain(pu * qj)
            cols = self.columns[u]
            if cols:
                dots = np.add.accumulate(np.concatenate([np.zeros((len(cols), 1)), pu * Q[cols]], axis=1), axis=1)[:, -1]
                uexp = _chain(exp_vec(dots))
            else:
                uexp = 0.0
            A = jdiv(fdlibm_exp(r), self.user_exp[u])
            B = jdiv(fdlibm_exp(pred), uexp)
            d = (A - B) * gd(pred)
            terms.append(-(A * fdlibm_log(B)))
            with np.errstate(all="ignore"):
                P[u] = pu + lrate * (d * qj - reg_u * pu)
                Q[j] = qj + lrate * (d * pu - reg_i * qj)
                terms.extend((0.5 * reg_u * pu * pu + 0.5 * reg_i * qj * qj).tolist())
        with np.errstate(all="ignore"):
            return (_chain(np.array(terms)) if terms else 0.0), np.array(terms)


def levels(n_users, n_items, cells):
    """the level of every user's unit, 1-based (0: the user stores no cell): 1 + the largest level among the last earlier users that
    store one of its columns, stored zeros included"""
    stored = [[] for _ in range(n_users)]
    for u, j, _ in cells:
        stored[int(u)].append(int(j))
    last, out = [0] * n_items, [0] * n_users
    for u in range(n_users):
        if stored[u]:
            out[u] = 1 + max(last[j] for j in stored[u])
            for j in stored[u]:
                last[j] = out[u]
    return out


def predict(P, Q, u, j):
    s = 0.0
    for f in range(len(P[u])):
        s += P[u][f] * Q[j][f]
    return s


def scores(P, Q):
    """predict(u, j) of every cell, as an array"""
    return np.array([[predict(P, Q, u, j) for j in range(len(Q))] for u in range(len(P))])


def golden():
    return json.loads(gzip.open(os.path.join(GOLDEN, "reference_lrmf.json.gz"), "rb").read())


def golden_runs():
    """the runs of tests/golden/reference_lrmf.json.gz, decoded"""
    gd_ = golden()
    knn = None
    runs = []
    for run in gd_["runs"]:
        cells = run.get("cells")
        if cells is None:  # the matrix of the KNN golden file
            knn = knn or json.loads(gzip.open(os.path.join(GOLDEN, "reference_knn.json.gz"), "rb").read())["knn_matrix"]
            assert (run["n_users"], run["n_items"]) == (knn["n_users"], knn["n_items"])
            cells = knn["cells"]
        nu, ni, k = run["n_users"], run["n_items"], run["k"]
        runs.append({"name": "%s k=%d" % (run["name"], k), "n_users": nu, "n_items": ni, "k": k, "seed": run["seed"],
                     "lrate": float.fromhex(run["lrate"]), "reg_u": float.fromhex(run["reg_u"]), "reg_i": float.fromhex(run["reg_i"]),
                     "cells": [(c[0], c[1], float.fromhex(c[2])) for c in cells],
                     "P0": unhex(run["P0"], nu, k), "Q0": unhex(run["Q0"], ni, k),
                     "iters": [{"P": unhex(it["P"], nu, k), "Q": unhex(it["Q"], ni, k), "loss": float.fromhex(it["loss"])}
                               for it in run["iters"]],
                     "predict": np.array([[float.fromhex(x) for x in row] for row in run["predict"]]),
                     "user_exp": unhex(run["user_exp"], nu), "columns": run["columns"],
                     "entries": [(e[0], e[1], float.fromhex(e[2])) for e in run["entries"]]})
    return runs
