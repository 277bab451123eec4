"""SlopeOne restated on the CPU (src/carskit/alg/baseline/cf/SlopeOne.java), in the reference's operation order, in Python floats
(IEEE doubles, no FMA).  Pinned to the reference's own source by tests/golden/reference_slopeone.json.gz (tests/test_slopeone_ref.py).

    rows = rows_of(u, i, r, n_users)          # user -> [(item, value)] ascending, the 2-D train matrix
    dev, card = build(rows, n_items)          # buildModel(): dense n x n
    predict(dev, card, rows, u, j, gm)        # predict(u, j); bound=True: Recommender.predict(u, j, c, true)

pair(col_a, col_b) is one cell by the per-pair walk the GPU kernel does (columns: item -> [(user, value)] ascending); build_rows() does
whole rows that way, for shapes where the reference's own O(sum of deg(u)^2) loop is too slow in Python."""
import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rows_of(u, i, r, n_users):
    rows = [[] for _ in range(n_users)]
    for a, b, v in sorted(zip(np.asarray(u).tolist(), np.asarray(i).tolist(), np.asarray(r, dtype=np.float64).tolist())):
        rows[a].append((b, v))
    return rows


def cols_of(u, i, r, n_items):
    return rows_of(i, u, r, n_items)


def build(rows, n_items):
    """buildModel(): users ascending, every ordered pair of the user's items; then the division where card > 0"""
    dev = [[0.0] * n_items for _ in range(n_items)]
    card = [[0] * n_items for _ in range(n_items)]
    for uv in rows:
        for i, rui in uv:
            di, ci = dev[i], card[i]
            for j, ruj in uv:
                if i != j:
                    di[j] += rui - ruj
                    ci[j] += 1
    for i in range(n_items):
        for j in range(n_items):
            if card[i][j] > 0:
                dev[i][j] = dev[i][j] / card[i][j]
    return np.array(dev, dtype=np.float64).reshape(n_items, n_items), np.array(card, dtype=np.int32).reshape(n_items, n_items)


def pair(col_a, col_b):
    """(dev[a][b], dev[b][a], card) of two columns by the walk over their common users, ascending: the sum of r_ua - r_ub from +0.0, one
    division, and the mirror: the negation, except that a zero sum is +0.0 on both sides (every reference sum starts at +0.0)"""
    vb = dict(col_b)
    s, k = 0.0, 0
    for x, va in col_a:
        if x in vb:
            s += va - vb[x]
            k += 1
    if k == 0:
        return 0.0, 0.0, 0
    d = s / k
    return d, (0.0 if s == 0.0 else -d), k


def build_rows(cols, anchors):
    """rows `anchors` of dev and card by the per-pair walk: {a: (dev row, card row)}"""
    n = len(cols)
    out = {}
    for a in anchors:
        d, c = np.zeros(n), np.zeros(n, np.int32)
        if cols[a]:
            for b in range(n):
                if b != a and cols[b]:
                    d[b], _, c[b] = pair(cols[a], cols[b])
        out[a] = (d, c)
    return out


def predict(dev, card, rows, u, j, gm, bound=False, lo=1.0, hi=5.0):
    preds, cards = 0.0, 0.0
    dj, cj = dev[j], card[j]
    for i, rui in rows[u]:
        if i == j:          # train.row(u, j): the user's vector without column j
            continue
        c = float(cj[i])
        if c > 0:
            preds += (float(dj[i]) + rui) * c
            cards += c
    pred = preds / cards if cards > 0 else gm
    if bound:
        if pred > hi:
            pred = hi
        if pred < lo:
            pred = lo
    return pred


def golden_runs():
    """the runs of tests/golden/reference_slopeone.json.gz, decoded: cells (u, i, r arrays), dev, card, predict, predict_bounded"""
    g = json.loads(gzip.open(os.path.join(GOLDEN, "reference_slopeone.json.gz"), "rb").read())
    knn = None
    runs = []
    for run in g["runs"]:
        cells = run.get("cells")
        if cells is None:  # the matrix of the KNN golden file
            knn = knn or json.loads(gzip.open(os.path.join(GOLDEN, "reference_knn.json.gz"), "rb").read())["knn_matrix"]
            assert (run["n_users"], run["n_items"]) == (knn["n_users"], knn["n_items"])
            cells = knn["cells"]
        unhex = lambda m: np.array([[float.fromhex(x) for x in row] for row in m], dtype=np.float64)  # noqa: E731
        runs.append({"name": run["name"], "n_users": run["n_users"], "n_items": run["n_items"],
                     "u": np.array([c[0] for c in cells], np.int32), "i": np.array([c[1] for c in cells], np.int32),
                     "r": np.array([float.fromhex(c[2]) for c in cells]), "global_mean": float.fromhex(run["global_mean"]),
                     "min_rate": float.fromhex(run["min_rate"]), "max_rate": float.fromhex(run["max_rate"]),
                     "dev": unhex(run["dev"]), "card": np.array(run["card"], np.int32), "predict": unhex(run["predict"]),
                     "predict_bounded": unhex(run["predict_bounded"])})
    return runs
