"""NMF restated on the CPU (src/carskit/alg/baseline/cf/NMF.java), in the reference's operation order, in IEEE doubles without FMA.
Pinned to the reference's own source by tests/golden/reference_nmf.json.gz (tests/test_nmf_ref.py).

    rows = rows_of(u, i, r, n_users)          # user -> (items ascending, values), the 2-D train matrix V
    cols = cols_of(u, i, r, n_items)          # item -> (users ascending, values)
    W, Ht = float64 arrays (n_users, k), (n_items, k)   # H item-major: Ht[j][f] = H[f][j]
    loss = iterate(W, Ht, rows, cols)         # one pass of buildModel()'s loop, in place: W phase, H phase, loss
    predict(W, Ht, u, j)                      # DenseMatrix.product(W, u, H, j)
    loss_tree(loss_cells(W, Ht, rows))        # the loss in the DEVICE's fixed summation order (not the reference's chain), bit for bit

Every sum is a left-to-right chain from 0.0: product() over f, DenseVector.inner(SparseVector) over the vector's entries in ascending
index order (its term is sv.get(j) * dv.get(j); the product commutes).  numpy does the arithmetic across the INDEPENDENT axis only (all
entries of a row at once for the chain over f, all factors at once for the chains over the entries): elementwise multiplies and adds,
one rounding each, so every chain keeps its order.  SparseMatrix.row() / column() leave a stored 0 out, so such a cell takes no part in
either phase (and `ruj > 0` keeps it out of the loss)."""
import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-9


def rows_of(u, i, r, n_users):
    """user -> (item indices ascending, values), without the zero-valued cells"""
    u, i, r = np.asarray(u, np.int64), np.asarray(i, np.int64), np.asarray(r, np.float64)
    keep = r != 0.0
    u, i, r = u[keep], i[keep], r[keep]
    order = np.lexsort((i, u))
    u, i, r = u[order], i[order], r[order]
    ptr = np.searchsorted(u, np.arange(n_users + 1))
    return [(i[a:b], r[a:b]) for a, b in zip(ptr[:-1], ptr[1:])]


def cols_of(u, i, r, n_items):
    return rows_of(i, u, r, n_items)


def products(W, Ht, u, j):
    """product(W, u[t], H, j[t]) of every t: the chain over f, all t side by side"""
    Wu, Hj = W[u], Ht[j]
    s = np.zeros(len(u))
    for f in range(W.shape[1]):
        s = s + Wu[:, f] * Hj[:, f]
    return s


def predict(W, Ht, u, j, bound=False, lo=1.0, hi=5.0):
    s = float(products(W, Ht, np.array([u]), np.array([j]))[0])
    if bound:
        if s > hi:
            s = hi
        if s < lo:
            s = lo
    return s


def update_row(own, other, idx, val):
    """the new own-side k-row: own[f] * (real_f / (estm_f + 1e-9)) over the row's entries (partner indices ascending, values); e_t from
    the old row"""
    if len(idx) == 0:
        return own.copy()
    part = other[idx]
    e = np.zeros(len(idx))
    for f in range(len(own)):
        e = e + own[f] * part[:, f]
    real, estm = np.zeros(len(own)), np.zeros(len(own))
    for t in range(len(idx)):
        real = real + val[t] * part[t]
        estm = estm + e[t] * part[t]
    return own * (real / (estm + EPS))


def loss_terms(W, Ht, rows):
    """(predict(u, j) - r)^2 of every cell with r > 0, in CRS order"""
    u = np.concatenate([np.full(len(idx), a, np.int64) for a, (idx, _) in enumerate(rows)] + [np.zeros(0, np.int64)])
    j = np.concatenate([idx for idx, _ in rows] + [np.zeros(0, np.int64)])
    r = np.concatenate([val for _, val in rows] + [np.zeros(0)])
    e = products(W, Ht, u, j) - r
    return (e * e)[r > 0]


def loss_cells(W, Ht, rows):
    """the loss term of every stored non-zero cell in CRS order, in place: (predict(u, j) - r)^2, and 0.0 where r > 0 does not hold (the
    device gives such a cell a lane of its own that adds +0.0; loss_terms leaves it out, which moves every later cell's place)"""
    u = np.concatenate([np.full(len(idx), a, np.int64) for a, (idx, _) in enumerate(rows)] + [np.zeros(0, np.int64)])
    j = np.concatenate([idx for idx, _ in rows] + [np.zeros(0, np.int64)])
    r = np.concatenate([val for _, val in rows] + [np.zeros(0)])
    e = products(W, Ht, u, j) - r
    return np.where(r > 0, e * e, 0.0)


LOSS_BLOCK = 256  # NMF_BLOCK: cells of a loss block, four waves of 64


def loss_partials(cells):
    """the device's partial of every loss block: the cells in order, LOSS_BLOCK a block, the last block padded with 0.0.
    A wave of 64 folds its terms in halves, t[l] + t[l + 32] for l < 32, then + 16, + 8, + 4, + 2, + 1; the block is ((w0 + w1) + w2) +
    w3.  All blocks, waves and the lanes of one fold side by side: none of them feeds another."""
    cells = np.asarray(cells, np.float64)
    blocks = -(-len(cells) // LOSS_BLOCK)
    t = np.zeros(blocks * LOSS_BLOCK)
    t[:len(cells)] = cells
    t = t.reshape(blocks, LOSS_BLOCK // 64, 64)
    for half in (32, 16, 8, 4, 2, 1):
        t = t[:, :, :half] + t[:, :, half:2 * half]
    w = t[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def loss_tree(cells):
    """the loss in the device's order: the block partials of loss_cells() added in block order in one chain from 0.0, then halved"""
    s = 0.0
    for p in loss_partials(cells).tolist():
        s += p
    return s * 0.5


def loss_of(W, Ht, rows):
    s = 0.0
    for t in loss_terms(W, Ht, rows).tolist():
        s += t
    return s * 0.5


def iterate(W, Ht, rows, cols, users=None, items=None):
    """one iteration in place (W: (n_users, k), Ht: (n_items, k) float64 arrays); returns the loss.  users / items: restate only those
    rows of either phase (the others keep their values) and no loss, for timing samples"""
    for u in (range(len(rows)) if users is None else users):
        W[u] = update_row(W[u], Ht, *rows[u])
    for j in (range(len(cols)) if items is None else items):
        Ht[j] = update_row(Ht[j], W, *cols[j])
    return loss_of(W, Ht, rows) if users is None and items is None else None


def skip_gaussians(rnd, n):
    """move a tests.hostmirror.javarand.JavaRandom stream past n nextGaussian() calls: the polar method draws pairs of nextDouble() until
    the point lies inside the unit circle, and every accepted pair serves two calls"""
    for _ in range((n + 1) // 2):
        while True:
            v1 = 2 * rnd.next_double() - 1
            v2 = 2 * rnd.next_double() - 1
            s = v1 * v1 + v2 * v2
            if 0 < s < 1:
                break


def init_model(rnd, n_users, n_items, k):
    """NMF.initModel() from a tests.hostmirror.javarand.JavaRandom stream: IterativeRecommender.initModel draws P (n_users x k) and Q
    (n_items x k) gaussian first -- unused, but they move the stream --, then W.init(0.01) and H.init(0.01) (k x n_items, row-major):
    uniform(0, 0.01) = nextDouble() * 0.01.  Returns (W, Ht) as arrays."""
    skip_gaussians(rnd, (n_users + n_items) * k)     # one stream: a pair's second value is kept from P's last call to Q's first
    W = np.array([rnd.next_double() * 0.01 for _ in range(n_users * k)]).reshape(n_users, k)
    H = np.array([rnd.next_double() * 0.01 for _ in range(k * n_items)]).reshape(k, n_items)
    return W, np.ascontiguousarray(H.T)


def unhex(xs, *shape):
    return np.array([float.fromhex(x) for x in xs], dtype=np.float64).reshape(shape)


def golden():
    return json.loads(gzip.open(os.path.join(GOLDEN, "reference_nmf.json.gz"), "rb").read())


def golden_runs():
    """the runs of tests/golden/reference_nmf.json.gz, decoded: cells (u, i, r arrays), W0, H0 (k x n_items), per iteration W, H, loss,
    and predict / predict_bounded"""
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
        m = lambda rows: np.array([[float.fromhex(x) for x in row] for row in rows], dtype=np.float64)  # noqa: E731
        runs.append({"name": "%s k=%d" % (run["name"], k), "n_users": nu, "n_items": ni, "k": k,
                     "u": np.array([c[0] for c in cells], np.int32), "i": np.array([c[1] for c in cells], np.int32),
                     "r": np.array([float.fromhex(c[2]) for c in cells]), "min_rate": float.fromhex(run["min_rate"]),
                     "max_rate": float.fromhex(run["max_rate"]), "W0": unhex(run["W0"], nu, k), "H0": unhex(run["H0"], k, ni),
                     "iters": [{"W": unhex(it["W"], nu, k), "H": unhex(it["H"], k, ni), "loss": float.fromhex(it["loss"])}
                               for it in run["iters"]],
                     "predict": m(run["predict"]), "predict_bounded": m(run["predict_bounded"])})
    return runs
