"""CPU restatement of the reference's RankALS (src/carskit/alg/baseline/ranking/RankALS.java; test infrastructure, never imported by
carskit_amd/; tools/bench_rankals.py times it beside the device), in the reference's operation order, in IEEE doubles without FMA.  Pinned to the reference's own source by
tests/golden/reference_rankals.json.gz (tests/test_rankals_ref.py).

    m = RankALS(n_users, n_items, cells, support_weight)    # the 2-D train matrix, s and sum_s
    m.iterate_literal(P, Q)      # one pass of buildModel()'s loop body in place, every item over every user of rows(), as the source does
    m.iterate(P, Q)              # the same bits: the four item-independent sums of the Q step are formed once (what the device runs)
    inv(A)                       # librec DenseMatrix.inv()
    predict(P, Q, u, j)          # DenseMatrix.rowMult(P, u, Q, j)

What librec's SparseMatrix makes of the cells (recorded in the golden file): a stored 0.0 takes no part anywhere.  row(u) and its
getCount() leave it out, get(u, i) returns the 0.0 of an absent cell for it, rows() lists the users with a non-zero cell (a user whose
only cell is a stored 0.0 is not solved and keeps the drawn row), and columnSize(i) counts the non-zero cells.  The three rater sums of
the Q step take the cells with a value > 0 only.

Every sum is a left-to-right chain from 0.0.  numpy does the arithmetic across INDEPENDENT elements only (the k or k x k elements of a
vector or matrix at once), elementwise multiplies, adds, subtracts and divides, one rounding each."""
import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def inv(A, stopped=None):
    """DenseMatrix.inv(): Gauss-Jordan on a copy beside I = eye(n).  Column i's pivot is the first row j >= i whose |mat[j][i]| is
    strictly greater than the running maximum (0.0 at the start: a NaN never wins); if none wins, I is returned AS IT STANDS.  Rows p and
    i are swapped, row i is divided by the pivot, every other row r takes f = mat[r][i] and subtracts the rounded f * row i.
    stopped: a list that receives the column at which the early return happened."""
    mat = np.array(A, dtype=np.float64)
    n = mat.shape[0]
    if n == 1:
        with np.errstate(all="ignore"):
            return np.array([[np.float64(1.0) / mat[0, 0]]])
    eye = np.eye(n)
    with np.errstate(all="ignore"):
        for i in range(n):
            best, p = 0.0, -1
            for j in range(i, n):
                a = abs(mat[j, i])
                if a > best:
                    best, p = a, j
            if p < 0:
                if stopped is not None:
                    stopped.append(i)
                return eye
            if p != i:
                mat[[i, p]] = mat[[p, i]]
                eye[[i, p]] = eye[[p, i]]
            piv = mat[i, i]
            mat[i, i:] = mat[i, i:] / piv
            eye[i] = eye[i] / piv
            f = mat[:, i].copy()
            others = np.arange(n) != i
            mat[others, i:] = mat[others, i:] - f[others, None] * mat[i, i:][None, :]
            eye[others] = eye[others] - f[others, None] * eye[i][None, :]
    return eye


def mult(M, y):
    """DenseMatrix.mult(DenseVector): per row the chain over b"""
    out = np.zeros(M.shape[0])
    for b in range(M.shape[1]):
        out = out + M[:, b] * y[b]
    return out


def solve(M, y):
    return mult(inv(M), y)


def predict(P, Q, u, j):
    s = 0.0
    for f in range(P.shape[1]):
        s += float(P[u, f]) * float(Q[j, f])
    return s


def scores(P, Q):
    s = np.zeros((P.shape[0], Q.shape[0]))
    for f in range(P.shape[1]):
        s = s + P[:, f][:, None] * Q[:, f][None, :]
    return s


class RankALS:
    def __init__(self, n_users, n_items, cells, support_weight):
        self.nu, self.ni = n_users, n_items
        cl = sorted((int(u), int(j), float(v)) for u, j, v in cells)
        self.rows = [[] for _ in range(n_users)]   # user -> ascending (item, value), without the stored zeros
        self.cols = [[] for _ in range(n_items)]   # item -> ascending (user, value), without the stored zeros
        for u, j, v in cl:
            if v != 0.0:
                self.rows[u].append((j, v))
                self.cols[j].append((u, v))
        self.users = [u for u in range(n_users) if self.rows[u]]   # train.rows()
        self.val = {(u, j): v for u, j, v in cl}
        self.s = np.array([float(len(self.cols[j])) if support_weight else 1.0 for j in range(n_items)])
        self.sum_s = 0.0
        for x in self.s.tolist():
            self.sum_s += x

    # ---- the shared first half: item moments and the P step ----------------------------------------------------------------------
    def item_moments(self, Q):
        k = Q.shape[1]
        sum_sq, sum_sqq = np.zeros(k), np.zeros((k, k))
        for j in range(self.ni):
            qj, sj = Q[j], self.s[j]
            sum_sq = sum_sq + qj * sj
            sum_sqq = sum_sqq + np.outer(qj, qj) * sj
        return sum_sq, sum_sqq

    def user_sums(self, Q, u):
        """the P step's sums of user u, which are step 3's m_* too (Q does not change in between)"""
        k = Q.shape[1]
        cqq, cq, cqr, sqr = np.zeros((k, k)), np.zeros(k), np.zeros(k), np.zeros(k)
        sum_sr = sum_cr = 0.0
        for i, rui in self.rows[u]:
            qi, si = Q[i], float(self.s[i])
            cqq = cqq + np.outer(qi, qi)
            cq = cq + qi
            cqr = cqr + qi * rui
            sum_sr += si * rui
            sum_cr += rui
            sqr = sqr + qi * (si * rui)
        return cqq, cq, cqr, sqr, sum_sr, sum_cr, float(len(self.rows[u]))

    def solve_user(self, Q, sum_sq, sum_sqq, u):
        """(the new P[u], m_sum_sr, m_sum_cr, m_sum_c, m_sum_cq)"""
        cqq, cq, cqr, sqr, sum_sr, sum_cr, sum_c = self.user_sums(Q, u)
        M = cqq * self.sum_s - np.outer(cq, sum_sq) - np.outer(sum_sq, cq) + sum_sqq * sum_c
        y = cqr * self.sum_s - cq * sum_sr - sum_sq * sum_cr + sqr * sum_c
        return solve(M, y), sum_sr, sum_cr, sum_c, cq

    def p_step(self, P, Q, users=None):
        sum_sq, sum_sqq = self.item_moments(Q)
        m = {}
        with np.errstate(all="ignore"):
            for u in (self.users if users is None else users):
                pu, sr, cr, c, cq = self.solve_user(Q, sum_sq, sum_sqq, u)
                P[u] = pu
                m[u] = (sr, cr, c, cq)
        return sum_sq, m

    # ---- the Q step ------------------------------------------------------------------------------------------------------------------
    def _finish_item(self, i, sum_sq, cpp, ppc, ppcq, crp, cpr, csrp, prc):
        si = float(self.s[i])
        M = cpp * self.sum_s + ppc * si
        y = mult(cpp, sum_sq) + cpr * self.sum_s - csrp + ppcq * si - crp * si + prc * si
        return solve(M, y)

    def iterate_literal(self, P, Q):
        k = P.shape[1]
        sum_sq, m = self.p_step(P, Q)
        with np.errstate(all="ignore"):
            for i in range(self.ni):
                cpp, ppc = np.zeros((k, k)), np.zeros((k, k))
                ppcq, cpr, csrp, crp, prc = np.zeros(k), np.zeros(k), np.zeros(k), np.zeros(k), np.zeros(k)
                for u in self.users:
                    pu = P[u]
                    sr, cr, c, cq = m[u]
                    rui = self.val.get((u, i), 0.0)
                    pp = np.outer(pu, pu)
                    cpp = cpp + pp
                    ppcq = ppcq + mult(pp, cq)
                    ppc = ppc + pp * c
                    crp = crp + pu * cr
                    if rui > 0:
                        cpr = cpr + pu * rui
                        csrp = csrp + pu * sr
                        prc = prc + pu * (rui * c)
                Q[i] = self._finish_item(i, sum_sq, cpp, ppc, ppcq, crp, cpr, csrp, prc)

    def user_moments(self, P, m):
        """the four sums of the Q step that do not depend on the item: each element is one chain over the users of rows() in order, the
        same chain for every item, hence the same bits"""
        k = P.shape[1]
        cpp, ppc, ppcq, crp = np.zeros((k, k)), np.zeros((k, k)), np.zeros(k), np.zeros(k)
        for u in self.users:
            pu = P[u]
            sr, cr, c, cq = m[u]
            pp = np.outer(pu, pu)
            cpp = cpp + pp
            ppcq = ppcq + mult(pp, cq)
            ppc = ppc + pp * c
            crp = crp + pu * cr
        return cpp, ppc, ppcq, crp

    def solve_item(self, P, m, sum_sq, mom, i):
        k = P.shape[1]
        cpr, csrp, prc = np.zeros(k), np.zeros(k), np.zeros(k)
        for u, rui in self.cols[i]:
            if rui > 0:
                pu = P[u]
                sr, cr, c, cq = m[u]
                cpr = cpr + pu * rui
                csrp = csrp + pu * sr
                prc = prc + pu * (rui * c)
        cpp, ppc, ppcq, crp = mom
        return self._finish_item(i, sum_sq, cpp, ppc, ppcq, crp, cpr, csrp, prc)

    def iterate(self, P, Q, items=None):
        """the hoisted form.  items: restate only those rows of Q (the others keep their values), for timing samples"""
        sum_sq, m = self.p_step(P, Q)
        with np.errstate(all="ignore"):
            mom = self.user_moments(P, m)
            for i in (range(self.ni) if items is None else items):
                Q[i] = self.solve_item(P, m, sum_sq, mom, i)


class _Pairs:
    """rows of a CSR given as [(index array, value array), ...], read as lists of (index, value)"""

    def __init__(self, csr):
        self.csr = csr

    def __len__(self):
        return len(self.csr)

    def __getitem__(self, a):
        idx, val = self.csr[a]
        return list(zip(idx.tolist(), val.tolist()))


def from_csr(n_users, n_items, rows, cols, support_weight):
    """a RankALS over tests.nmf_ref.rows_of / cols_of arrays (no zero-valued cells), for matrices too large for lists of tuples; the
    literal form is not available on it"""
    m = RankALS.__new__(RankALS)
    m.nu, m.ni, m.rows, m.cols, m.val = n_users, n_items, _Pairs(rows), _Pairs(cols), None
    m.users = [u for u in range(n_users) if len(rows[u][0])]
    m.s = np.array([float(len(cols[j][0])) if support_weight else 1.0 for j in range(n_items)])
    m.sum_s = 0.0
    for x in m.s.tolist():
        m.sum_s += x
    return m


class UserSums:
    """step 3's maps of EVERY user at once, the same chains as RankALS.user_sums: the users side by side, each walking its own row in
    order (pass t adds entry t of every row that has one).  m[u] = (sum_sr, sum_cr, sum_c, sum_cq)"""

    def __init__(self, model, Q, rows):
        nu, k = len(rows), Q.shape[1]
        ln = np.array([len(r[0]) for r in rows])
        ptr = np.concatenate([[0], np.cumsum(ln)])
        idx = np.concatenate([r[0] for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
        val = np.concatenate([r[1] for r in rows] + [np.zeros(0)])
        self.sr, self.cr, self.c, self.cq = np.zeros(nu), np.zeros(nu), ln.astype(np.float64), np.zeros((nu, k))
        order = np.argsort(-ln, kind="stable")           # the users by descending length: pass t takes a prefix of them
        for t in range(int(ln.max()) if nu else 0):
            act = order[:int(np.searchsorted(-ln[order], -t, side="left"))]   # the users with more than t entries
            e = ptr[act] + t
            r, si = val[e], model.s[idx[e]]
            self.sr[act] = self.sr[act] + si * r
            self.cr[act] = self.cr[act] + r
            self.cq[act] = self.cq[act] + Q[idx[e]]

    def __getitem__(self, u):
        return float(self.sr[u]), float(self.cr[u]), float(self.c[u]), self.cq[u]


def user_moments_fast(model, P, m):
    """RankALS.user_moments with pp.mult(m_sum_cq[u]) of all users formed side by side (the chain over b per user and element); the four
    sums stay one chain over the users of rows() in order"""
    k = P.shape[1]
    T = np.zeros_like(P)
    for b in range(k):
        T = T + (P * P[:, b][:, None]) * m.cq[:, b][:, None]
    cpp, ppc, ppcq, crp = np.zeros((k, k)), np.zeros((k, k)), np.zeros(k), np.zeros(k)
    for u in model.users:
        pu = P[u]
        pp = np.outer(pu, pu)
        cpp = cpp + pp
        ppcq = ppcq + T[u]
        ppc = ppc + pp * m.c[u]
        crp = crp + pu * m.cr[u]
    return cpp, ppc, ppcq, crp


def init_model(rnd, n_users, n_items, k, mean=0.0, std=0.1):
    """IterativeRecommender.initModel()'s P and Q from an oracle.oracle_np.JavaRandom stream: DenseMatrix.init(mean, std) row by row,
    Randoms.gaussian(mean, std) = mean + std * nextGaussian()"""
    g = [mean + std * rnd.next_gaussian() for _ in range((n_users + n_items) * k)]
    return (np.array(g[:n_users * k]).reshape(n_users, k), np.array(g[n_users * k:]).reshape(n_items, k))


def unhex(xs, *shape):
    return np.array([float.fromhex(x) for x in xs], dtype=np.float64).reshape(shape)


def golden():
    return json.loads(gzip.open(os.path.join(GOLDEN, "reference_rankals.json.gz"), "rb").read())


def golden_runs():
    """the runs of tests/golden/reference_rankals.json.gz, decoded: cells, P0, Q0, per iteration P and Q, predict, and what librec made
    of the matrix (rows, row_count, column_size, s, sum_s)"""
    g = golden()
    knn = None
    runs = []
    for run in g["runs"]:
        cells = run.get("cells")
        if cells is None:  # the matrix of the KNN golden file
            knn = knn or json.loads(gzip.open(os.path.join(GOLDEN, "reference_knn.json.gz"), "rb").read())["knn_matrix"]
            assert (run["n_users"], run["n_items"]) == (knn["n_users"], knn["n_items"])
            cells = knn["cells"]
        nu, ni, k = run["n_users"], run["n_items"], run["k"]
        runs.append({"name": "%s k=%d sw=%s" % (run["name"], k, "on" if run["sw"] else "off"), "n_users": nu, "n_items": ni, "k": k,
                     "sw": run["sw"], "cells": [(c[0], c[1], float.fromhex(c[2])) for c in cells],
                     "P0": unhex(run["P0"], nu, k), "Q0": unhex(run["Q0"], ni, k),
                     "iters": [{"P": unhex(it["P"], nu, k), "Q": unhex(it["Q"], ni, k)} for it in run["iters"]],
                     "predict": np.array([[float.fromhex(x) for x in row] for row in run["predict"]]),
                     "rows": run["rows"], "row_count": run["row_count"], "column_size": run["column_size"],
                     "s": unhex(run["s"], ni), "sum_s": float.fromhex(run["sum_s"])})
    return runs


def golden_inv():
    return [{"name": c["name"], "n": c["n"], "A": unhex(c["A"], c["n"], c["n"]), "inv": unhex(c["inv"], c["n"], c["n"])}
            for c in golden()["inv"]]


def top_lists(cand, queries, score, thold, num_recs):
    """the lists Recommender.evalRankings keeps, from a score matrix: per query (user, ctx, correct items, excluded candidate positions)
    the candidates not excluded whose score is above the threshold, by descending score, ties in candidate order, the first num_recs;
    a query without a correct item or without a scored candidate has no list"""
    out = {}
    for u, c, correct, excl in queries:
        ex = set(excl)
        sc = [(j, float(score[u, j])) for p, j in enumerate(cand) if p not in ex and score[u, j] > thold]
        sc.sort(key=lambda kv: -kv[1])
        if correct and sc:
            out[(u, c)] = sc[:num_recs]
    return out
