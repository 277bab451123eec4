"""CPU restatement of the reference's BPR (src/carskit/alg/baseline/ranking/BPR.java; test infrastructure, never imported by
carskit_amd/; tools/bench_bpr.py times it beside the device), in the reference's operation order, in IEEE doubles without FMA.  Pinned
to the reference's own source by tests/golden/reference_bpr.json.gz (tests/test_bpr_ref.py).

    rnd = JavaStream(state)            # java.util.Random from its 48-bit state: next(bits), next_int(bound) (the published algorithm)
    m = BPR(n_users, n_items, cells)   # the 2-D train matrix as train.row(u) sees it
    u, i, j = m.sample(rnd)            # BPR.java:65-80: one triple
    tri = m.sample_iteration(rnd)      # n_users * 100 of them
    loss = m.epoch(P, Q, tri, lrate, reg_u, reg_i)   # BPR.java:83-102 over the triples, in place; the loss chain
    levels(n_users, n_items, tri)      # the level of every sample: 1 + the largest level of an earlier sample on one of its three rows
    fdlibm_exp(x), fdlibm_log(x)       # StrictMath.exp / log.  Math.exp / Math.log are specified to 1 ulp only; the project defines
                                       # them as StrictMath's

What librec's SparseMatrix makes of the cells (recorded in the golden file): a stored 0.0 takes no part.  row(u) leaves it out, so
getCount() == len(getIndex()) and `is[Randoms.uniform(is.length)]` never reads a slot past the count; a user whose only cell is a stored
0.0 is drawn again like an empty one.  contains(j) binary-searches the row's WHOLE index array (capacity: the next power of two >= count,
zero tail), so it can miss an entry of the upper half: such an item can be drawn as j, and j == i can happen."""
import gzip
import json
import math
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MASK = (1 << 48) - 1
SAMPLES_PER_USER = 100


def _bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _dbl(b):
    return struct.unpack("<d", struct.pack("<q", b))[0]


def _with_high(x, hi):
    return struct.unpack("<d", struct.pack("<Q", ((hi & 0xFFFFFFFF) << 32) | (_bits(x) & 0xFFFFFFFF)))[0]


def _high(x):
    h = (_bits(x) >> 32) & 0xFFFFFFFF
    return h - (1 << 32) if h >= 1 << 31 else h


def fdlibm_log(x):
    """fdlibm __ieee754_log, every argument"""
    ln2_hi, ln2_lo, two54 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.80143985094819840000e+16
    Lg = (6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01,
          1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01)
    hx, lx, k = _high(x), _bits(x) & 0xFFFFFFFF, 0
    if hx < 0x00100000:
        if ((hx & 0x7FFFFFFF) | lx) == 0:
            return -math.inf
        if hx < 0:
            return math.nan
        k -= 54
        x *= two54
        hx = _high(x)
    if hx >= 0x7FF00000:
        return x + x
    k += (hx >> 20) - 1023
    hx &= 0x000FFFFF
    i = (hx + 0x95F64) & 0x100000
    x = _with_high(x, hx | (i ^ 0x3FF00000))
    k += i >> 20
    f = x - 1.0
    dk = float(k)
    if (0x000FFFFF & (2 + hx)) < 3:
        if f == 0.0:
            return 0.0 if k == 0 else dk * ln2_hi + dk * ln2_lo
        R = f * f * (0.5 - 0.33333333333333333 * f)
        return f - R if k == 0 else dk * ln2_hi - ((R - dk * ln2_lo) - f)
    s = f / (2.0 + f)
    z = s * s
    w = z * z
    t1 = w * (Lg[1] + w * (Lg[3] + w * Lg[5]))
    t2 = z * (Lg[0] + w * (Lg[2] + w * (Lg[4] + w * Lg[6])))
    R = t2 + t1
    i, j = hx - 0x6147A, 0x6B851 - hx
    if i >= 0 and j >= 0 and (i | j) > 0:
        hfsq = 0.5 * f * f
        if k == 0:
            return f - (hfsq - s * (hfsq + R))
        return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f)
    if k == 0:
        return f - s * (f - R)
    return dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f)


def fdlibm_exp(x):
    """fdlibm __ieee754_exp, every argument"""
    ln2HI, ln2LO, invln2 = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00
    P1, P2, P3, P4, P5 = (1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05,
                          -1.65339022054652515390e-06, 4.13813679705723846039e-08)
    twom1000 = 9.33263618503218878990e-302
    b = _bits(x)
    hx, lx = (b >> 32) & 0xFFFFFFFF, b & 0xFFFFFFFF
    xsb = hx >> 31
    hx &= 0x7FFFFFFF
    hi = lo = 0.0
    k = 0
    if hx >= 0x40862E42:
        if hx >= 0x7FF00000:
            if (hx & 0xFFFFF) | lx:
                return x + x
            return x if xsb == 0 else 0.0
        if x > 7.09782712893383973096e+02:
            return math.inf                  # huge * huge
        if x < -7.45133219101941108420e+02:
            return 0.0                       # twom1000 * twom1000
    if hx > 0x3FD62E42:
        if hx < 0x3FF0A2B2:
            hi = x - (-ln2HI if xsb else ln2HI)
            lo = -ln2LO if xsb else ln2LO
            k = 1 - xsb - xsb
        else:
            k = int(invln2 * x + (-0.5 if xsb else 0.5))
            t = float(k)
            hi = x - t * ln2HI
            lo = t * ln2LO
        x = hi - lo
    elif hx < 0x3E300000:
        return 1.0 + x
    t = x * x
    c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))))
    if k == 0:
        return 1.0 - ((x * c) / (c - 2.0) - x)
    y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi)
    if k >= -1021:
        return _with_high(y, _high(y) + (k << 20))
    return _with_high(y, _high(y) + ((k + 1000) << 20)) * twom1000


def g(x):
    """Recommender.g: 1.0 / (1.0 + Math.exp(-x))"""
    return 1.0 / (1.0 + fdlibm_exp(-x))


def random_state(seed):
    return (seed ^ 0x5DEECE66D) & MASK


class JavaStream:
    """java.util.Random from its 48-bit state; `draws` counts the calls of next()"""

    def __init__(self, state):
        self.state, self.draws = state, 0

    def next(self, bits):
        self.state = (self.state * 0x5DEECE66D + 0xB) & MASK
        self.draws += 1
        v = self.state >> (48 - bits)
        return v - (1 << 32) if v >= 1 << 31 else v

    def next_int(self, bound):
        """Random.nextInt(bound): r = next(31); a power of two takes the high bits, (int) ((bound * (long) r) >> 31); else
        `for (u = r; u - (r = u % bound) + m < 0; u = next(31))` in wrapping int arithmetic"""
        r = self.next(31)
        m = bound - 1
        if bound & m == 0:
            return (bound * r) >> 31
        u = r
        while True:
            r = u % bound
            if ((u - r + m + (1 << 31)) & 0xFFFFFFFF) - (1 << 31) >= 0:
                return r
            u = self.next(31)


def contains(idx, key):
    """SparseVector.contains(key): Arrays.binarySearch over the whole capacity"""
    n = len(idx)
    cap = 0 if n == 0 else 1 << (n - 1).bit_length()
    low, high = 0, cap - 1
    while low <= high:
        mid = (low + high) >> 1
        v = idx[mid] if mid < n else 0
        if v < key:
            low = mid + 1
        elif v > key:
            high = mid - 1
        else:
            return True
    return False


class BPR:
    def __init__(self, n_users, n_items, cells):
        self.n_users, self.n_items = n_users, n_items
        self.rows = [[] for _ in range(n_users)]
        for u, i, v in sorted((int(u), int(i), float(v)) for u, i, v in cells):
            if v != 0.0:
                self.rows[u].append(i)
        self.found = [[contains(row, j) for j in range(n_items)] for row in self.rows] if n_users * n_items <= 1 << 22 else None

    def _contains(self, u, j):
        return self.found[u][j] if self.found is not None else contains(self.rows[u], j)

    def sample(self, rnd):
        while True:
            u = rnd.next_int(self.n_users)
            row = self.rows[u]
            if not row:
                continue
            i = row[rnd.next_int(len(row))]
            while True:
                j = rnd.next_int(self.n_items)
                if not self._contains(u, j):
                    return u, i, j

    def sample_iteration(self, rnd, n=None):
        return [self.sample(rnd) for _ in range(self.n_users * SAMPLES_PER_USER if n is None else n)]


def update(P, Q, u, i, j, lrate, reg_u, reg_i, terms=None):
    """BPR.java:83-102 of one sample, in place on the lists of lists P and Q; returns the loss it adds as a list of its 1 + k terms in
    order (appended to `terms` if given)"""
    pu, qi, qj = P[u], Q[i], Q[j]
    k = len(pu)
    xui = xuj = 0.0
    for f in range(k):
        xui += pu[f] * qi[f]
    for f in range(k):
        xuj += pu[f] * qj[f]
    xuij = xui - xuj
    out = [-fdlibm_log(g(xuij))]
    cmg = g(-xuij)
    for f in range(k):
        puf, qif, qjf = pu[f], qi[f], qj[f]
        pu[f] += lrate * (cmg * (qif - qjf) - reg_u * puf)
        qi[f] += lrate * (cmg * puf - reg_i * qif)
        qj[f] += lrate * (cmg * (-puf) - reg_i * qjf)
        out.append(reg_u * puf * puf + reg_i * qif * qif + reg_i * qjf * qjf)
    if terms is not None:
        terms.extend(out)
    return out


def epoch(P, Q, triples, lrate, reg_u, reg_i, terms=None):
    """one iteration's samples in sequence; P and Q are lists of lists, updated in place.  Returns the loss: one chain from 0.0 over
    every sample's terms in order"""
    loss = 0.0
    for u, i, j in triples:
        for t in update(P, Q, u, i, j, lrate, reg_u, reg_i, terms):
            loss += t
    return loss


def epoch_by_levels(P, Q, triples, lrate, reg_u, reg_i):
    """the same iteration level by level on numpy arrays P and Q (in place): the samples of a level touch pairwise different rows, so
    a level's updates commute and the result has the sequential epoch's bits (tests/test_bpr_capi_cpu.py replays that).  numpy works
    across the INDEPENDENT samples of a level only; a dot is np.add.accumulate from 0.0 along the factors, one chain.  Returns
    (loss, terms): the reference's loss chain over the (S, 1 + k) terms in (sample, term) order, and the terms"""
    n, k = len(triples), P.shape[1]
    lv = np.array(levels(P.shape[0], Q.shape[0], triples))
    tri = np.array(triples, dtype=np.int64).reshape(n, 3)
    terms = np.empty((n, k + 1))
    zero = None
    for level in range(1, int(lv.max()) + 1 if n else 1):
        idx = np.nonzero(lv == level)[0]
        u, i, j = tri[idx, 0], tri[idx, 1], tri[idx, 2]
        pu, qi, qj = P[u], Q[i], Q[j]
        zero = np.zeros((len(idx), 1))
        xui = np.add.accumulate(np.concatenate([zero, pu * qi], axis=1), axis=1)[:, -1]
        xuj = np.add.accumulate(np.concatenate([zero, pu * qj], axis=1), axis=1)[:, -1]
        xuij = xui - xuj
        terms[idx, 0] = [-fdlibm_log(g(x)) for x in xuij.tolist()]
        cmg = np.array([g(-x) for x in xuij.tolist()])[:, None]
        P[u] = pu + lrate * (cmg * (qi - qj) - reg_u * pu)
        new_qi = qi + lrate * (cmg * pu - reg_i * qi)
        dj = lrate * (cmg * (-pu) - reg_i * qj)
        Q[i] = new_qi
        Q[j] = np.where((i == j)[:, None], new_qi + dj, qj + dj)
        terms[idx, 1:] = reg_u * pu * pu + reg_i * qi * qi + reg_i * qj * qj
    flat = terms.ravel()
    loss = float(np.add.accumulate(np.concatenate([[0.0], flat]))[-1]) if n else 0.0
    return loss, terms


def levels(n_users, n_items, triples):
    """the level of every sample (1-based)"""
    lu, li = [0] * n_users, [0] * n_items
    out = []
    for u, i, j in triples:
        lv = 1 + max(lu[u], li[i], li[j])
        lu[u] = li[i] = li[j] = lv
        out.append(lv)
    return out


def predict(P, Q, u, j):
    s = 0.0
    for f in range(len(P[u])):
        s += P[u][f] * Q[j][f]
    return s


def scores(P, Q):
    """predict(u, j) of every cell, as an array"""
    return np.array([[predict(P, Q, u, j) for j in range(len(Q))] for u in range(len(P))])


def init_model(rnd, n_users, n_items, k):
    """IterativeRecommender.initModel() with initByNorm = false from an oracle.oracle_np.JavaRandom stream: DenseMatrix.init() row by
    row, Randoms.uniform(0, 1) = 0.0 + nextDouble() * (1.0 - 0.0)"""
    d = [0.0 + rnd.next_double() * (1.0 - 0.0) for _ in range((n_users + n_items) * k)]
    return (np.array(d[:n_users * k]).reshape(n_users, k), np.array(d[n_users * k:]).reshape(n_items, k))


def unhex(xs, *shape):
    return np.array([float.fromhex(x) for x in xs], dtype=np.float64).reshape(shape)


def golden():
    return json.loads(gzip.open(os.path.join(GOLDEN, "reference_bpr.json.gz"), "rb").read())


def golden_runs():
    """the runs of tests/golden/reference_bpr.json.gz, decoded"""
    gd = golden()
    knn = None
    runs = []
    for run in gd["runs"]:
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
                     "iters": [{"P": unhex(it["P"], nu, k), "Q": unhex(it["Q"], ni, k), "loss": float.fromhex(it["loss"]),
                                "state": it["state"], "triples": [tuple(t) for t in it["triples"]]} for it in run["iters"]],
                     "predict": np.array([[float.fromhex(x) for x in row] for row in run["predict"]]),
                     "row_count": run["row_count"], "index_len": run["index_len"], "contains": run["contains"]})
    return runs
