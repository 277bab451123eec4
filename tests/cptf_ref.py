"""CPTF restated in numpy and plain Python: the reference's epoch (CPTF.java:75-115) in its own order and in the device's non-strict
order, both predicts (CPTF.java:119-155), the tensor build (DataDAO.java:423-481), TensorRecommender's fold split (:62-84) over a small
model of librec's SparseTensor, getKeys (:189-205) and evalRatings (:86-164).  Every operation on a double is one IEEE operation,
written in the order the Java source has it; nothing here reads the kernels."""
import math

import numpy as np

# ---- the model ----------------------------------------------------------------------------------------------------------------------


def predict_keys(M, keys):
    """CPTF.predict(int[] keys), CPTF.java:141-155: the product from 1 over d, the sum a chain over f"""
    pred = 0.0
    for f in range(M[0].shape[1]):
        prod = 1.0
        for d, key in enumerate(keys):
            prod = prod * float(M[d][key, f])
        pred = pred + prod
    return pred


def clamp(pred, lo, hi):
    """CPTF.java:133-136 / TensorRecommender.java:169-174: a NaN passes both comparisons"""
    if pred > hi:
        pred = hi
    if pred < lo:
        pred = lo
    return pred


def predict_ujc(M, u, j, ctx_keys, lo, hi):
    """CPTF.predict(u, j, c), CPTF.java:119-139, with getKeys' keys of the context"""
    return clamp(predict_keys(M, [u, j] + [int(x) for x in ctx_keys]), lo, hi)


def score_items(M, u, ctx_keys, lo, hi):
    """predict_ujc(M, u, j, ctx_keys, lo, hi) of every item j at once: the same operations per item, in the same order"""
    with np.errstate(all="ignore"):
        prod = np.ones_like(M[1]) * M[0][u]
        prod = prod * M[1]
        for d, key in enumerate(ctx_keys):
            prod = prod * M[2 + d][int(key)]
        pred = np.zeros(M[1].shape[0])
        for f in range(M[1].shape[1]):
            pred = pred + prod[:, f]
    return [clamp(p, lo, hi) for p in pred.tolist()]


def _rows(M, keys):
    return [M[d][int(key)].copy() for d, key in enumerate(keys)]


def _update(M, keys, rows, prod, e, lrate, reg):
    """CPTF.java:93-108 for every f at once: factor f of the entry's rows is read and written at f's turn only, and the dimensions are
    different matrices, so `sgd` is the product `pred` took and `df` the value before the sweep reached it"""
    terms = []
    with np.errstate(all="ignore"):
        for d, key in enumerate(keys):
            df = rows[d]
            gdf = prod / df * e
            M[d][int(key)] = df + lrate * (gdf - reg * df)
            terms.append(reg * df * df)
    return terms


def epoch_strict(M, keys, r, lrate, reg):
    """one iteration in the reference's order, M (a list of (dims[d], k) arrays) updated in place; returns the loss after :111"""
    lrate, reg, loss = np.float64(lrate), np.float64(reg), 0.0
    for ks, rate in zip(np.asarray(keys).tolist(), np.asarray(r, dtype=np.float64).tolist()):
        if rate <= 0:
            continue
        rows = _rows(M, ks)
        with np.errstate(all="ignore"):
            prod = np.ones_like(rows[0])
            for row in rows:
                prod = prod * row
        pred = 0.0
        for p in prod.tolist():
            pred = pred + p
        e = rate - pred
        loss = loss + e * e
        terms = _update(M, ks, rows, prod, np.float64(e), lrate, reg)
        for f in range(len(prod)):
            for d in range(len(ks)):
                loss = loss + float(terms[d][f])
    return loss * 0.5


def wave_sum(x):
    """a sum over 64 lanes as a fixed tree: inside every row of 16 lanes the lanes 8, 4, 2 and 1 apart are added in turn (every lane
    then holds its row's sum), then (row 3 + row 2) + (row 1 + row 0)"""
    x = np.asarray(x, dtype=np.float64).reshape(4, 16)
    with np.errstate(all="ignore"):
        for s in (8, 4, 2, 1):
            x = x + np.roll(x, s, axis=1)
        row = x[:, 15]
        return float((row[3] + row[2]) + (row[1] + row[0]))


def epoch_tree(M, keys, r, lrate, reg):
    """one iteration in the non-strict order: the same updates, but `pred` is the tree sum over 64 lanes that own one (k <= 64) or two
    consecutive factors each, and the loss is summed by parts: the chain of e * e over the entries, then every factor's own chain of
    reg * df * df over (entry, d), added in factor order"""
    k = M[0].shape[1]
    per = 1 if k <= 64 else 2
    lrate, reg = np.float64(lrate), np.float64(reg)
    sum_e, sum_f, any_entry = 0.0, np.zeros(k), False
    for ks, rate in zip(np.asarray(keys).tolist(), np.asarray(r, dtype=np.float64).tolist()):
        if rate <= 0:
            continue
        any_entry = True
        rows = _rows(M, ks)
        with np.errstate(all="ignore"):
            prod = np.ones_like(rows[0])
            for row in rows:
                prod = prod * row
            lanes = np.zeros(64 * per)
            lanes[:k] = prod
            lanes = lanes.reshape(64, per)
            part = lanes[:, 0].copy()
            for c in range(1, per):
                part = part + lanes[:, c]
        pred = wave_sum(part)
        e = rate - pred
        sum_e = sum_e + e * e
        terms = _update(M, ks, rows, prod, np.float64(e), lrate, reg)
        with np.errstate(all="ignore"):
            for d in range(len(ks)):
                sum_f = sum_f + terms[d]
    if not any_entry:
        return 0.0
    loss = 0.0 + sum_e
    for v in sum_f.tolist():
        loss = loss + v
    return loss * 0.5


# ---- java.util.HashSet<Integer> as guava's HashMultimap keeps one per key -----------------------------------------------------------


class JavaIntHashSet:
    """insertion and iteration of a java.util.HashSet<Integer> (JDK 8) created with `slots` table slots (guava's HashMultimap:
    new HashSet(3), 4 slots; new HashSet(): 16).  Iteration is by bucket, inside a bucket by insertion; a table doubles when its size
    passes 3/4 of its slots.  Tree bins (9 colliding keys in a table of 64 slots or more) are not modelled: add() refuses them."""

    def __init__(self, slots=4):
        self.cap, self.keys = slots, []

    def _bucket(self, key, cap):
        h = key & 0xFFFFFFFF
        return (h ^ (h >> 16)) & (cap - 1)

    def add(self, key):
        if key in self.keys:
            return
        self.keys.append(key)
        same = sum(1 for x in self.keys if self._bucket(x, self.cap) == self._bucket(key, self.cap))
        if same >= 9:
            if self.cap >= 64:
                raise NotImplementedError("a tree bin")
            self.cap *= 2
        if len(self.keys) > self.cap * 3 // 4:
            self.cap *= 2

    def __iter__(self):
        return iter(sorted(self.keys, key=lambda x: self._bucket(x, self.cap)))   # (stable: insertion order inside a bucket)

    def __len__(self):
        return len(self.keys)


class SparseTensor:
    """librec.data.SparseTensor as far as TensorRecommender uses it: parallel key lists and values in insertion order, and per indexed
    dimension a HashMultimap key -> positions that getIndices and findIndex walk in HashSet order"""

    def __init__(self, n_dims, keys=(), vals=()):
        self.n_dims = n_dims
        self.keys, self.vals = [list(k) for k in keys], list(vals)
        self.index, self.indexed = {}, []

    def clone(self):
        res = SparseTensor(self.n_dims, self.keys, self.vals)
        res.indexed = list(self.indexed)
        for d, multimap in self.index.items():                       # putAll: the positions arrive in the source's iteration order
            res.index[d] = {}
            for key, positions in multimap.items():
                for p in positions:
                    res.index[d].setdefault(key, JavaIntHashSet()).add(p)
        return res

    def build_index(self, d):
        self.index[d] = {}
        for p, ks in enumerate(self.keys):
            self.index[d].setdefault(ks[d], JavaIntHashSet()).add(p)
        if d not in self.indexed:
            self.indexed.append(d)

    def get_indices(self, user, item):
        if 0 not in self.indexed:
            self.build_index(0)
        return [p for p in self.index[0].get(user, ()) if self.keys[p][1] == item]

    def find_index(self, keys):
        if not self.vals:
            return -1
        if not self.indexed:
            self.build_index(0)
        d = self.indexed[0]
        for p in self.index[d].get(keys[d], ()):
            if self.keys[p] == list(keys):
                return p
        return -1

    def set(self, val, keys):
        p = self.find_index(keys)
        if p >= 0:
            self.vals[p] = val
            return
        self.keys.append(list(keys))
        for d in self.indexed:
            self.index[d].setdefault(keys[d], JavaIntHashSet()).add(len(self.keys) - 1)
        self.vals.append(val)

    def remove(self, keys):
        p = self.find_index(keys)
        if p < 0:
            return False
        del self.keys[p]
        del self.vals[p]
        for d in list(self.indexed):
            self.build_index(d)
        return True


# ---- DataDAO.toSparseTensor, TensorRecommender ---------------------------------------------------------------------------------------

KEYS_SIZE, KEYS_INDEXOF = "size", "indexof"


def tensor_build(cells, pair_user, pair_item, ctx_conds, cond_dim, form=KEYS_SIZE):
    """DataDAO.java:423-481.  cells: (pair, context, rate) in rateMatrix order; ctx_conds[c]: the context's conditions in list order;
    cond_dim[cond]: its dimension.  form: KEYS_SIZE is the reference (:461 is not under the `if`: a condition already listed gets the
    last index of its dimension's list), KEYS_INDEXOF its evident intent.
    Returns dims, keys (one list per entry), vals, dim_lists ({dimension: its conditions in list order})"""
    n_dims = 2 + len(set(cond_dim.values() if isinstance(cond_dim, dict) else cond_dim))
    keys, vals, dim_lists = [], [], {}
    seen = [set() for _ in range(n_dims)]
    for pair, ctx, rate in cells:
        ks = [None] * n_dims
        ks[0], ks[1] = int(pair_user[pair]), int(pair_item[pair])
        for cond in ctx_conds[ctx]:
            dim = int(cond_dim[cond])
            if dim in dim_lists:
                lst = dim_lists[dim]
                index = lst.index(cond) if cond in lst else -1
                if index == -1:
                    lst.append(cond)
                if form == KEYS_SIZE or index == -1:
                    index = len(lst) - 1
            else:
                dim_lists[dim] = [cond]
                index = 0
            ks[2 + dim] = index
        for d in range(n_dims):
            seen[d].add(ks[d])
        keys.append(ks)
        vals.append(float(rate))
    return [len(s) for s in seen], keys, vals, dim_lists


def get_keys_table(ctx_conds, dim_lists):
    """TensorRecommender.getKeys (:189-205) of every context: its k-th condition is looked up in dimension k's list; -1: not there"""
    table = []
    for conds in ctx_conds:
        row = []
        for k, cond in enumerate(conds):
            lst = dim_lists.get(k, [])
            row.append(lst.index(cond) if cond in lst else -1)
        table.append(row)
    return table


def fold_split(n_dims, keys, vals, pair_user, pair_item, test_cells):
    """TensorRecommender.java:62-84.  test_cells: (pair, context, rate) of testMatrix in its order.  Returns (train keys, train vals,
    test keys, test vals), each in its tensor's iterator order"""
    rate = SparseTensor(n_dims, keys, vals)
    train, test = rate.clone(), SparseTensor(n_dims)
    for pair, _, _ in test_cells:
        for p in rate.get_indices(int(pair_user[pair]), int(pair_item[pair])):
            test.set(rate.vals[p], rate.keys[p])
            train.remove(rate.keys[p])
    return train.keys, train.vals, test.keys, test.vals


def fold_split_fast(n_dims, keys, vals, pair_user, pair_item, test_cells):
    """fold_split's result without the tensor model's quadratic bookkeeping, for files of thousands of cells: every index of a test pair
    is removed, so the train tensor is the rate tensor without the test pairs' entries, in order; the test tensor takes, per test cell,
    the pair's entries in the HashSet order of the user's positions, a key tuple already present keeping its place and taking the
    value.  Held equal to fold_split by tests/test_cptf_ref.py"""
    test_pairs = {(int(pair_user[p]), int(pair_item[p])) for p, _, _ in test_cells}
    positions, ordered = {}, {}
    for p, ks in enumerate(keys):
        positions.setdefault(ks[0], []).append(p)
    train = [(list(ks), v) for ks, v in zip(keys, vals) if (ks[0], ks[1]) not in test_pairs]
    at, test_keys, test_vals = {}, [], []
    for pair, _, _ in test_cells:
        u, i = int(pair_user[pair]), int(pair_item[pair])
        if u not in ordered:
            hs = JavaIntHashSet()
            for p in positions.get(u, []):
                hs.add(p)
            ordered[u] = list(hs)
        for p in ordered[u]:
            if keys[p][1] != i:
                continue
            kt = tuple(keys[p])
            if kt in at:
                test_vals[at[kt]] = vals[p]
            else:
                at[kt] = len(test_vals)
                test_keys.append(list(keys[p]))
                test_vals.append(vals[p])
    return [ks for ks, _ in train], [v for _, v in train], test_keys, test_vals


def java_round(x):
    """Math.round(double), JDK 8: floor(x + 1/2) computed without the addition's rounding; NaN -> 0"""
    if math.isnan(x):
        return 0
    if math.isinf(x) or abs(x) >= 2.0 ** 52:
        return max(-2 ** 63, min(2 ** 63 - 1, int(x))) if not math.isinf(x) else (2 ** 63 - 1 if x > 0 else -2 ** 63)
    fl = math.floor(x)
    return int(fl) + (1 if x - fl >= 0.5 else 0)


def eval_ratings(M, test_keys, test_vals, lo, hi):
    """TensorRecommender.evalRatings (:86-164), view "all": the bounded predict(keys) of every test entry in iterator order"""
    s_mae = s_mse = s_rmae = s_rmse = 0.0
    n = n_pe = 0
    for ks, rate in zip(test_keys, test_vals):
        pred = clamp(predict_keys(M, ks), lo, hi)
        if math.isnan(pred):
            continue
        r_pred = java_round(pred / lo) * lo
        err, r_err = abs(rate - pred), abs(rate - r_pred)
        s_mae, s_mse = s_mae + err, s_mse + err * err
        s_rmae, s_rmse = s_rmae + r_err, s_rmse + r_err * r_err
        n += 1
        if r_err > 1e-5:
            n_pe += 1
    div = lambda a: a / n if n else float("nan")   # noqa: E731  (0.0 / 0 in Java)
    mae = div(s_mae)
    return {"MAE": mae, "NMAE": mae / (hi - lo), "RMSE": math.sqrt(div(s_mse)), "rMAE": div(s_rmae), "rRMSE": math.sqrt(div(s_rmse)),
            "MPE": div(n_pe + 0.0), "n": n}
