"""CPU restatement of the reference's BPMF (src/carskit/alg/baseline/cf/BPMF.java; test infrastructure, never imported by carskit_amd/;
tools/bench_bpmf.py times it beside the device), in the reference's operation order, in IEEE doubles without FMA.  Pinned to the
reference's own source and to librec's / happy.coding's bytecode by tests/golden/reference_bpmf.json.gz (tests/test_bpmf_ref.py).

    rnd = Stream(state, have, cached)   # happy.coding.math.Randoms' java.util.Random: the 48-bit state AND nextGaussian's cached value
    rnd.gaussian(), gamma(rnd, alpha, scale), wishart(rnd, scale, df)
    cholesky(A)                         # DenseMatrix.cholesky().transpose(): the LOWER factor, or None
    column_mean(X), cov(X)              # DenseMatrix.columnMean / cov
    m = BPMF(n_users, n_items, cells, global_mean)
    hy = m.init_hyper(P, Q)             # BPMF.java:77-83
    m.hyper(rnd, P, Q, hy)              # :98-149, in place
    flags, draws = m.sample_side(rnd, side, P, Q, alpha, mu)   # one Gibbs pass of one side (:155-191 or :194-229), in place
    loss = m.iterate(rnd, P, Q, hy)     # one pass of the loop body (:97-242)

Two random streams: DenseMatrix.init draws P and Q from librec.util.Randoms; gaussian / gamma here draw from happy.coding.math.Randoms.
They are different java.util.Random objects, so P and Q are an input and `rnd` is the second stream alone.

What the bytecode does (each recorded in the golden file):
  * cholesky(): L[i][j] = (A[i][j] - sum_{k<j} L[i][k] L[j][k]) / L[j][j], the diagonal Math.sqrt(A[i][i] - sum); after row i, a NaN
    L[i][i] returns null.  A zero diagonal is NOT null (the later rows divide by it).  The upper factor is returned and BPMF transposes
    it back.
  * cov(): per column x - Stats.mean(x), where Stats.mean SKIPS NaN entries (sum and count); the inner product of two centred columns
    over (rows - 1).  columnMean() skips nothing.
  * SparseVector.inner(SparseVector), which wishart() uses for its sums over k, asks contains(idx) of the other vector: a binary search
    over the WHOLE index array (capacity the next power of two, zero tail), which misses some indices of the upper half when the
    length is no power of two.  Those terms are left out, here too.
  * Randoms.gamma(alpha, 2) for alpha >= 1 (the case alpha < 1 is never reached: alpha >= numRows / 2).
  * a stored 0.0 takes no part in row(u) / column(j) (a user whose only cell is a stored zero has count == 0); the loss walks what the
    matrix iterator gives (`loss_cells`).

numpy does the arithmetic across INDEPENDENT elements only; every sum is one left-to-right chain from 0.0."""
import gzip
import json
import math
import os

import numpy as np

from tests.bpr_ref import MASK, contains, fdlibm_exp, fdlibm_log, random_state  # noqa: F401
from tests.rankals_ref import inv, mult, unhex  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BETA = 2.0   # `int beta = 2`, scale(beta)
B0 = 2       # b0_u = b0_m


class Stream:
    """java.util.Random from its 48-bit state, with nextGaussian's cached second value"""

    def __init__(self, state, have=False, cached=0.0):
        self.state, self.have, self.cached = state, bool(have), float(cached)

    @classmethod
    def seeded(cls, seed):
        return cls(random_state(seed))

    def copy(self):
        return Stream(self.state, self.have, self.cached)

    def key(self):
        return (self.state, self.have, self.cached.hex() if self.have else None)

    def _next(self, bits):
        self.state = (self.state * 0x5DEECE66D + 0xB) & MASK
        return self.state >> (48 - bits)

    def next_double(self):
        hi = self._next(26)
        return float((hi << 27) + self._next(27)) * (1.0 / (1 << 53))

    def gaussian(self):
        """Randoms.gaussian(0, 1) = 0 + 1 * nextGaussian()"""
        if self.have:
            self.have = False
            return 0.0 + 1.0 * self.cached
        while True:
            v1 = 2.0 * self.next_double() - 1.0
            v2 = 2.0 * self.next_double() - 1.0
            s = v1 * v1 + v2 * v2
            if s < 1.0 and s != 0.0:
                break
        m = math.sqrt(-2.0 * fdlibm_log(s) / s)
        self.cached, self.have = v2 * m, True
        return 0.0 + 1.0 * (v1 * m)


def polar_attempt(state):
    """the attempt that starts at `state` (4 LCG steps): (accepted, first, second)"""
    r = Stream(state)
    v1 = 2.0 * r.next_double() - 1.0
    v2 = 2.0 * r.next_double() - 1.0
    s = v1 * v1 + v2 * v2
    if s < 1.0 and s != 0.0:
        m = math.sqrt(-2.0 * fdlibm_log(s) / s)
        return True, v1 * m, v2 * m
    return False, 0.0, 0.0


_Q = (0.000171032, -0.0004701849, 0.0006053049, 0.0003340332, -0.0003349403, 0.0015746717, 0.0079849875, 0.0208333723, 0.0416666664)
_A = (0.104089866, -0.112750886, 0.11036831, -0.124385581, 0.142873973, -0.166677482, 0.199999867, -0.249999949, 0.333333333)
_E = (0.000247453, 0.001353826, 0.008345522, 0.041664508, 0.166666848, 0.499999994, 1.0)


def gamma(rnd, alpha, lam):
    """happy.coding.math.Randoms.gamma(alpha, lambda), alpha >= 1, statement by statement from the bytecode (Math.* as StrictMath)"""
    if not alpha >= 1.0:
        raise ValueError("gamma: alpha < 1 is not restated (BPMF never reaches it)")
    inv_l = 1.0 / lam
    ss = alpha - 0.5
    s = math.sqrt(ss)
    d = 5.656854249 - 12.0 * s
    while True:
        v1 = 2.0 * rnd.next_double() - 1.0
        v2 = 2.0 * rnd.next_double() - 1.0
        v12 = v1 * v1 + v2 * v2
        if not v12 > 1.0:
            break
    t = v1 * math.sqrt(-2.0 * fdlibm_log(v12) / v12) if v12 > 0.0 else math.nan
    x = s + 0.5 * t
    gds = x * x
    if t >= 0.0:
        return gds / inv_l
    u = rnd.next_double()
    if d * u <= t * t * t:
        return gds / inv_l
    r = 1.0 / alpha
    q0 = _Q[0]
    for c in _Q[1:]:
        q0 = q0 * r + c
    q0 = q0 * r
    if alpha > 3.686:
        if alpha > 13.022:
            b, si, c = 1.77, 0.75, 0.1515 / s
        else:
            b, si, c = 1.654 + 0.0076 * ss, 1.68 / s + 0.275, 0.062 / s + 0.024
    else:
        b, si, c = 0.463 + s - 0.178 * ss, 1.235, 0.195 / s - 0.079 + 0.016 * s

    def q_of(t):
        v = t / (s + s)
        if abs(v) > 0.25:
            return q0 - s * t + 0.25 * t * t + (ss + ss) * fdlibm_log(1.0 + v)
        p = _A[0]
        for a in _A[1:]:
            p = p * v + a
        return q0 + 0.5 * t * t * p * v

    if x > 0.0:
        q = q_of(t)
        if fdlibm_log(1.0 - u) <= q:
            return gds / inv_l
    while True:
        e = -fdlibm_log(rnd.next_double())
        u = rnd.next_double()
        u = u + u - 1.0
        sign_u = 1.0 if u > 0.0 else -1.0
        t = b + e * si * sign_u
        if t <= -0.71874483771719:
            continue
        q = q_of(t)
        if q <= 0.0:
            continue
        if q > 0.5:
            w = fdlibm_exp(q) - 1.0
        else:
            w = _E[0]
            for ec in _E[1:]:
                w = w * q + ec
            w = w * q
        if not c * u * sign_u <= w * fdlibm_exp(e - 0.5 * t * t):
            continue
        x = s + 0.5 * t
        return x * x / inv_l


def cholesky(A):
    """DenseMatrix.cholesky().transpose(): the lower factor L, or None.  The partial sums of row i's later elements take their terms in
    the order of k, as each element's own chain does."""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[0]
    L = np.zeros((n, n))
    with np.errstate(all="ignore"):
        for i in range(n):
            s = np.zeros(i + 1)
            for j in range(i + 1):
                if j == i:
                    L[i, i] = np.sqrt(A[i, i] - s[i])
                else:
                    L[i, j] = (A[i, j] - s[j]) / L[j, j]
                    s[j + 1:] = s[j + 1:] + L[i, j] * L[j + 1:i + 1, j]   # the rows j + 1 .. i, row i's new element included
            if L[i, i] != L[i, i]:
                return None
    return L


def cholesky_literal(A):
    """the same, element by element as the bytecode walks it (for the small matrices of the golden file)"""
    n = len(A)
    L = [[0.0] * n for _ in range(n)]
    with np.errstate(all="ignore"):
        for i in range(n):
            for j in range(i + 1):
                s = 0.0
                for k in range(j):
                    s += L[i][k] * L[j][k]
                d = np.float64(A[i][j]) - s
                L[i][j] = float(np.sqrt(d)) if i == j else float(d / np.float64(L[j][j]))
            if L[i][i] != L[i][i]:
                return None
    return np.array(L).reshape(n, n)


def column_mean(X):
    """DenseMatrix.columnMean(f) of every f: one chain over the rows, over numRows"""
    s = np.zeros(X.shape[1])
    for r in range(X.shape[0]):
        s = s + X[r]
    with np.errstate(all="ignore"):
        return s / float(X.shape[0])


def cov(X):
    """DenseMatrix.cov()"""
    n, k = X.shape
    s, cnt = np.zeros(k), np.zeros(k)
    nan = np.isnan(X)
    for r in range(n):
        s = s + np.where(nan[r], 0.0, X[r])
        cnt = cnt + np.where(nan[r], 0.0, 1.0)
    with np.errstate(all="ignore"):
        C = X - (s / cnt)[None, :]
        acc = np.zeros((k, k))
        for r in range(n):
            acc = acc + np.outer(C[r], C[r])
        return acc / float(n - 1)


def matmul(A, B):
    """DenseMatrix.mult(DenseMatrix): per element the chain over the inner index"""
    out = np.zeros((A.shape[0], B.shape[1]))
    for m in range(A.shape[1]):
        out = out + np.outer(A[:, m], B[m, :])
    return out


def sparse_inner(a, b):
    """SparseVector.inner(SparseVector) of two vectors that hold the indices 0 .. n - 1"""
    idx = list(range(len(a)))
    s = 0.0
    for i in idx:
        if contains(idx, i):
            s += a[i] * b[i]
    return s


def wishart(rnd, scale, df):
    """BPMF.wishart (BPMF.java:258-313): None (and no draw) when the scale has no factor"""
    L = cholesky(scale)
    if L is None:
        return None
    p = scale.shape[0]
    z = [[rnd.gaussian() for _ in range(p)] for _ in range(p)]
    y = [gamma(rnd, (df - (i + 1)) / 2, 2.0) for i in range(p)]
    B = np.zeros((p, p))
    B[0, 0] = y[0]
    for j in range(1, p):
        zz = [z[k][j] for k in range(j)]
        B[j, j] = y[j] + sparse_inner(zz, zz)
    for j in range(1, p):
        B[0, j] = B[j, 0] = z[0][j] * math.sqrt(y[0])
    for j in range(2, p):
        for i in range(1, j):
            B[i, j] = B[j, i] = z[i][j] * math.sqrt(y[i]) + sparse_inner([z[k][i] for k in range(i)], [z[k][j] for k in range(i)])
    A = L.T.copy()   # scale.cholesky(): the upper factor
    return matmul(matmul(A.T.copy(), B), A)


def hyper_side(rnd, X, alpha, mu, mean=None, S=None):
    """BPMF.java:98-122 (or :125-149) of one side: (alpha, mu) after it.  mean / S: columnMean and cov() formed elsewhere"""
    M, k = X.shape
    x_bar = column_mean(X) if mean is None else mean
    S_bar = cov(X) if S is None else S
    with np.errstate(all="ignore"):
        d = np.zeros(k) - x_bar
        e = np.outer(d, d) * ((M * B0) / (B0 + M + 0.0))
        WI = inv(np.eye(k)) + S_bar * float(M) + e
        WI = inv(WI)
        WI = (WI + WI.T) * 0.5
        w = wishart(rnd, WI, float(k + M))
        if w is not None:
            alpha = w
        mu_temp = (np.zeros(k) * float(B0) + x_bar * float(M)) * (1 / (B0 + M + 0.0))
        L = cholesky(inv(alpha * float(B0 + M)))
        if L is not None:
            zs = np.array([rnd.gaussian() for _ in range(k)])
            mu = mult(L, zs) + mu_temp
    return alpha, mu


def row_posterior(other, entries, gm, alpha, mu):
    """(mean, L or None) of one row: BPMF.java:164-179"""
    k = other.shape[1]
    G, v = np.zeros((k, k)), np.zeros(k)
    with np.errstate(all="ignore"):
        for j, r in entries:
            q = other[j]
            G = G + np.outer(q, q)
            v = v + q * (r - gm)
        covar = inv(alpha + G * BETA)
        mean = mult(covar, v * BETA + mult(alpha, mu))
        return mean, cholesky(covar)


class BPMF:
    def __init__(self, n_users, n_items, cells, global_mean, loss_zeros=True):
        self.nu, self.ni, self.gm = n_users, n_items, float(global_mean)
        cl = sorted((int(u), int(j), float(v)) for u, j, v in cells)
        self.rows = [[] for _ in range(n_users)]
        self.cols = [[] for _ in range(n_items)]
        for u, j, v in cl:
            if v != 0.0:
                self.rows[u].append((j, v))
                self.cols[j].append((u, v))
        self.loss_cells = [c for c in cl if loss_zeros or c[2] != 0.0]   # the matrix iterator: CRS order

    def init_hyper(self, P, Q):
        """BPMF.java:77-83"""
        with np.errstate(all="ignore"):
            return {"mu_u": column_mean(P), "mu_m": column_mean(Q), "alpha_u": inv(cov(P)), "alpha_m": inv(cov(Q))}

    def hyper(self, rnd, P, Q, hy):
        hy["alpha_u"], hy["mu_u"] = hyper_side(rnd, P, hy["alpha_u"], hy["mu_u"])
        hy["alpha_m"], hy["mu_m"] = hyper_side(rnd, Q, hy["alpha_m"], hy["mu_m"])

    def sample_side(self, rnd, side, P, Q, alpha, mu, only=None):
        """one pass over the users (side 0, writes P) or the items (side 1, writes Q).  flags[x]: 1 where the row had entries and no
        factor (it keeps its value and takes no draw).  only: restate those rows alone, drawing for each from `rnd` as it stands"""
        own, other, lists = (P, Q, self.rows) if side == 0 else (Q, P, self.cols)
        flags, draws = [0] * len(lists), 0
        for x in (range(len(lists)) if only is None else only):
            if not lists[x]:
                continue
            mean, L = row_posterior(other, lists[x], self.gm, alpha, mu)
            if L is None:
                flags[x] = 1
                continue
            zs = np.array([rnd.gaussian() for _ in range(own.shape[1])])
            draws += own.shape[1]
            with np.errstate(all="ignore"):
                own[x] = mult(L, zs) + mean
        return flags, draws

    def loss(self, P, Q):
        s = 0.0
        with np.errstate(all="ignore"):
            for u, j, r in self.loss_cells:
                e = r - predict(P, Q, self.gm, u, j)
                s += e * e
        return s * 0.5

    def iterate(self, rnd, P, Q, hy):
        self.hyper(rnd, P, Q, hy)
        for _ in range(2):
            self.sample_side(rnd, 0, P, Q, hy["alpha_u"], hy["mu_u"])
            self.sample_side(rnd, 1, P, Q, hy["alpha_m"], hy["mu_m"])
        return self.loss(P, Q)


def predict(P, Q, gm, u, j):
    """globalMean + DenseMatrix.rowMult(P, u, Q, j)"""
    s = 0.0
    for f in range(P.shape[1]):
        s += float(P[u, f]) * float(Q[j, f])
    return gm + s


def init_model(rnd, n_users, n_items, k):
    """P.init(0, 1), Q.init(0, 1) from a stream of the OTHER Randoms class (oracle.oracle_np.JavaRandom or a Stream): row by row"""
    draw = rnd.gaussian if hasattr(rnd, "gaussian") else rnd.next_gaussian
    g = [0.0 + 1.0 * draw() for _ in range((n_users + n_items) * k)]
    return np.array(g[:n_users * k]).reshape(n_users, k), np.array(g[n_users * k:]).reshape(n_items, k)


def golden():
    return json.loads(gzip.open(os.path.join(GOLDEN, "reference_bpmf.json.gz"), "rb").read())


def golden_cells(run):
    cells = run.get("cells")
    if cells is None:
        km = json.loads(gzip.open(os.path.join(GOLDEN, "reference_knn.json.gz"), "rb").read())["knn_matrix"]
        assert (run["n_users"], run["n_items"]) == (km["n_users"], km["n_items"])
        cells = km["cells"]
    return [(c[0], c[1], float.fromhex(c[2])) for c in cells]
