"""CPU restatement of the reference's ItemKNN / UserKNN rating prediction (test infrastructure; never imported by carskit_amd/ or tools/).

* `correlation(iv, jv, method, shrinkage, min_rate, max_rate)`: Recommender.correlation (Recommender.java:385-432) over sparse vectors
  given as ascending (index, value) lists, with the six happy.coding.math.Sims formulas as their bytecode computes them
  (lib/happy.coding.utils-1.2.6.jar: sequential sums; Math.pow(d, 2.0) is d * d; Sims.msd turns +-Infinity into 1.0;
  Sims.pcc needs two common entries; cos-binary uses the full-vector SparseVector.inner products).
* `build_corrs(rows, n_ctr, ...)`: Recommender.buildCorrs -- the same sums, vectorised over the partners of one anchor (non-common
  entries add +0.0, which changes no bit), as a dense matrix with NaN where nothing is stored.
* `predict(...)`: ItemKNN.predict / UserKNN.predict with the java.util.HashMap (JDK 8) iteration order; `JavaIntHashMap` models the
  table's growth (size threshold, and the resize treeifyBin does on tables below 64 slots) and reports a bin that would be treeified.
"""
import math

import numpy as np

MEASURES = ("pcc", "cos", "cos-binary", "msd", "cpc", "exjaccard")


def measure_name(name):
    """Recommender.correlation's switch: case-insensitive, anything unknown is pcc"""
    n = name.lower()
    return n if n in MEASURES else "pcc"


def sims(method, a, b, median=0.0, inner=None):
    """happy.coding.math.Sims on the common lists a (of iv) and b (of jv); inner = (iv.inner(jv), iv.inner(iv), jv.inner(jv))"""
    n = len(a)
    if method == "cos-binary":
        x, na, nb = inner
        return _div(x, math.sqrt(na) * math.sqrt(nb))
    if method == "msd":
        s = 0.0
        for x, y in zip(a, b):
            d = x - y
            s += d * d
        sim = _div(float(n), s)
        return 1.0 if math.isinf(sim) else sim
    if method == "exjaccard":
        s = sa = sb = 0.0
        for x, y in zip(a, b):
            s += x * y
            sa += x * x
            sb += y * y
        return _div(s, sa + sb - s)
    if method == "pcc":
        if n < 2:
            return math.nan
        ma, mb = _mean(a), _mean(b)
        num = da = db = 0.0
        for x, y in zip(a, b):
            p, q = x - ma, y - mb
            num += p * q
            da += p * p
            db += q * q
        return _div(num, math.sqrt(da) * math.sqrt(db))
    if n == 0:
        return math.nan
    if method == "cpc":
        a = [x - median for x in a]
        b = [y - median for y in b]
    s = sa = sb = 0.0
    for x, y in zip(a, b):
        s += x * y
        sa += x * x
        sb += y * y
    return _div(s, math.sqrt(sa) * math.sqrt(sb))


def _mean(v):  # happy.coding.math.Stats.mean(Collection): sequential sum / count
    s = 0.0
    for x in v:
        s += x
    return s / len(v)


def _div(x, y):  # Java double division (IEEE): x/0 is +-Infinity or NaN
    if y == 0.0:
        if x == 0.0 or math.isnan(x):
            return math.nan
        return math.copysign(math.inf, x) * math.copysign(1.0, y)
    return x / y


def contains(v, key):
    """librec SparseVector.contains(key): Arrays.binarySearch over the WHOLE index array.  A vector built by set() grows that array to
    the next power of two (1, 2, 4, ...) and leaves the tail zero, so the search can step into the zeros and miss an entry of the upper
    half; it never finds a key the vector lacks (its first probe, index cap/2 - 1, is a real entry)."""
    n = len(v)
    cap = 0 if n == 0 else 1 << (n - 1).bit_length()
    a = [k for k, _ in v] + [0] * (cap - n)
    low, high = 0, cap - 1
    while low <= high:
        mid = (low + high) >> 1
        if a[mid] < key:
            low = mid + 1
        elif a[mid] > key:
            high = mid - 1
        else:
            return True
    return False


def findable(v):
    """per entry of v: does v.contains find its own index"""
    return [contains(v, k) for k, _ in v]


def correlation(iv, jv, method, shrinkage, min_rate=1.0, max_rate=5.0):
    """Recommender.correlation(iv, jv, method); iv, jv: ascending lists of (index, value)"""
    method = measure_name(method)
    di = dict(iv)
    a, b = [], []
    for idx, val in jv:  # for (Integer idx : jv.getIndex()) if (iv.contains(idx)) ...
        if contains(iv, idx):
            a.append(di[idx])
            b.append(val)
    inner = None
    if method == "cos-binary":
        dj = dict(jv)
        x = 0.0
        for idx, val in iv:  # SparseVector.inner: iv's indices, jv.contains
            if contains(jv, idx):
                x += val * dj[idx]
        na = nb = 0.0
        for idx, val in iv:
            if contains(iv, idx):
                na += val * val
        for idx, val in jv:
            if contains(jv, idx):
                nb += val * val
        inner = (x, na, nb)
    sim = sims(method, a, b, (min_rate + max_rate) / 2.0, inner)
    if not math.isnan(sim) and shrinkage > 0:
        n = len(a)
        sim *= n / float(n + shrinkage)
    return sim


def rows_of(u, i, r, kind, n_users, n_items):
    """the compared rows (ItemKNN: columns of the 2-D matrix, UserKNN: its rows) as ascending (index, value) lists"""
    ent, ctr = (np.asarray(i), np.asarray(u)) if kind == "item" else (np.asarray(u), np.asarray(i))
    n = n_items if kind == "item" else n_users
    rows = [[] for _ in range(n)]
    for e, c, v in sorted(zip(ent.tolist(), ctr.tolist(), np.asarray(r, dtype=np.float64).tolist())):
        rows[e].append((c, v))
    return rows


def build_corrs(rows, n_ctr, method, shrinkage, min_rate=1.0, max_rate=5.0, anchors=None):
    """Recommender.buildCorrs as a dense matrix (NaN = not stored), the sums vectorised over each anchor's partners; `anchors`: only
    those rows' pairs with larger partners (the rest stays NaN)"""
    method = measure_name(method)
    n = len(rows)
    X = np.zeros((n, n_ctr))
    P = np.zeros((n, n_ctr), dtype=bool)
    for e, row in enumerate(rows):
        for c, v in row:
            X[e, c] = v
            P[e, c] = True
    F = np.zeros((n, n_ctr), dtype=bool)  # the entries SparseVector.contains finds
    ok = [findable(row) for row in rows]
    for e, row in enumerate(rows):
        for (c, _), f in zip(row, ok[e]):
            F[e, c] = f
    norm2 = np.zeros(n)
    for e, row in enumerate(rows):
        s = 0.0
        for (_, v), f in zip(row, ok[e]):  # iv.inner(iv)
            if f:
                s += v * v
        norm2[e] = s
    med = (min_rate + max_rate) / 2.0
    S = np.full((n, n), np.nan)
    nonempty = np.array([len(r) > 0 for r in rows])
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        for a in (range(n - 1) if anchors is None else anchors):
            if a >= n - 1 or not rows[a]:
                continue
            bs = np.nonzero(nonempty[a + 1:])[0] + a + 1
            if len(bs) == 0:
                continue
            k = np.zeros(len(bs), dtype=np.int64)
            x1, x2, x3 = np.zeros(len(bs)), np.zeros(len(bs)), np.zeros(len(bs))
            for (c, va), fa in zip(rows[a], ok[a]):  # ascending contracted index
                if method == "cos-binary":  # iv.inner(jv) tests jv.contains; n = is.size() counts correlation()'s list all the same
                    if fa:
                        k += P[bs, c]
                    m = P[bs, c] & F[bs, c]
                elif not fa:  # correlation(): iv.contains misses this entry of the anchor
                    continue
                else:
                    m = P[bs, c]
                    k += m
                vb = X[bs, c]
                if method == "pcc":
                    x1 += np.where(m, va, 0.0)
                    x2 += np.where(m, vb, 0.0)
                elif method == "msd":
                    d = va - vb
                    x1 += np.where(m, d * d, 0.0)
                elif method == "cos-binary":
                    x1 += np.where(m, va * vb, 0.0)
                else:
                    p, q = (va - med, vb - med) if method == "cpc" else (va, vb)
                    x1 += np.where(m, p * q, 0.0)
                    x2 += np.where(m, p * p, 0.0)
                    x3 += np.where(m, q * q, 0.0)
            if method == "pcc":
                mua, mub = x1 / k, x2 / k
                x1, x2 = np.zeros(len(bs)), np.zeros(len(bs))
                for (c, va), fa in zip(rows[a], ok[a]):
                    if not fa:
                        continue
                    m = P[bs, c]
                    p, q = va - mua, X[bs, c] - mub
                    x1 += np.where(m, p * q, 0.0)
                    x2 += np.where(m, p * p, 0.0)
                    x3 += np.where(m, q * q, 0.0)
                sim = np.where(k >= 2, x1 / (np.sqrt(x2) * np.sqrt(x3)), np.nan)
            elif method in ("cos", "cpc"):
                sim = np.where(k > 0, x1 / (np.sqrt(x2) * np.sqrt(x3)), np.nan)
            elif method == "cos-binary":
                sim = x1 / (np.sqrt(norm2[a]) * np.sqrt(norm2[bs]))
            elif method == "msd":
                sim = k.astype(np.float64) / x1
                sim = np.where(np.isinf(sim), 1.0, sim)
            else:
                sim = x1 / (x2 + x3 - x1)
            if shrinkage > 0:
                sim = np.where(np.isnan(sim), sim, sim * (k.astype(np.float64) / (k + shrinkage).astype(np.float64)))
            S[a, bs] = sim
            S[bs, a] = sim
    return S


def row_means(rows, global_mean):
    """itemMeans / userMeans: SparseVector.mean() (sum in index order / count), globalMean for an empty row"""
    out = np.empty(len(rows))
    for e, row in enumerate(rows):
        if row:
            s = 0.0
            for _, v in row:
                s += v
            out[e] = s / len(row)
        else:
            out[e] = global_mean
    return out


class Treeified(Exception):
    """a put made a bin of 9 nodes in a table of 64 slots or more: java.util.HashMap would treeify it"""


class JavaIntHashMap:
    """java.util.HashMap<Integer, Double> of JDK 8, for its iteration order: bins are lists in insertion order (a resize keeps the
    order inside a bin); a put that makes a list of 9 nodes calls treeifyBin, which resizes a table below 64 slots and treeifies the
    bin otherwise (not modelled: raises Treeified)."""

    def __init__(self):
        self.cap, self.thr, self.keys, self.vals = 0, 0, [], {}

    @staticmethod
    def hash(k):
        k &= 0xFFFFFFFF
        return k ^ (k >> 16)

    def put(self, k, v):
        if self.cap == 0:
            self.cap, self.thr = 16, 12
        b = self.hash(k) & (self.cap - 1)
        if k not in self.vals:
            nodes = sum(1 for q in self.keys if (self.hash(q) & (self.cap - 1)) == b)
            self.keys.append(k)
            if nodes >= 8:  # binCount >= TREEIFY_THRESHOLD - 1
                if self.cap < 64:
                    self.cap, self.thr = self.cap * 2, self.thr * 2
                else:
                    raise Treeified(k)
            self.vals[k] = v
            if len(self.keys) > self.thr:
                self.cap, self.thr = self.cap * 2, self.thr * 2
        else:
            self.vals[k] = v

    def clear(self):  # keeps the table
        self.keys, self.vals = [], {}

    def items(self):
        order = sorted(range(len(self.keys)), key=lambda t: (self.hash(self.keys[t]) & (self.cap - 1), t))
        return [(self.keys[t], self.vals[self.keys[t]]) for t in order]

    def __len__(self):
        return len(self.keys)


def predict(kind, S, means, lists, u, j, knn, global_mean, bound=False, lo=1.0, hi=5.0):
    """ItemKNN.predict(u, j) (kind "item": lists[u] = the user's (item, rating) cells) or UserKNN.predict(u, j) (kind "user":
    lists[j] = the item's (user, rating) cells); S dense with NaN unset; means = itemMeans / userMeans.  Raises Treeified."""
    owner, target = (u, j) if kind == "item" else (j, u)
    nns = JavaIntHashMap()
    for e, rate in lists[owner]:  # dv.getIndex() ascending; train.get(...) > 0 only where a cell exists
        sim = S[target, e]
        if sim > 0 and rate > 0:
            nns.put(e, float(sim))
    if 0 < knn < len(nns):
        srt = sorted(nns.items(), key=lambda kv: -kv[1])  # Lists.sortMap(nns, true): stable, descending by value
        nns.clear()
        for k, v in srt[:knn]:
            nns.put(k, v)
    if len(nns) == 0:
        pred = global_mean
    else:
        rate_of = dict(lists[owner])
        s = ws = 0.0
        for e, sim in nns.items():
            s += sim * (rate_of[e] - float(means[e]))
            ws += abs(sim)
        pred = float(means[target]) + _div(s, ws) if ws > 0 else global_mean
    if bound:
        if pred > hi:
            pred = hi
        if pred < lo:
            pred = lo
    return pred


def lists_of(u, i, r, kind, n_users, n_items):
    """the prediction side's lists: ItemKNN -> per user its (item, rating) cells; UserKNN -> per item its (user, rating) cells"""
    return rows_of(u, i, r, "user" if kind == "item" else "item", n_users, n_items)


def eval_ratings(preds, truth, min_rate):
    """Recommender.evalRatings (MAE, RMSE) over bounded predictions; NaN predictions are skipped"""
    sa = ss = 0.0
    n = 0
    for p, r in zip(preds, truth):
        if math.isnan(p):
            continue
        e = abs(r - p)
        sa += e
        ss += e * e
        n += 1
    return sa / n, math.sqrt(ss / n)


# ---- the same prediction, vectorised -----------------------------------------------------------------------------------------------
# predict() puts every candidate through JavaIntHashMap, whose put scans all keys: O(m^2) Python steps a tuple, unusable near the
# 16 384-candidate limit.  predict_fast() restates it with numpy: the table's growth is a closed form of the size (plus a serial walk
# while the table is below 64 slots, where treeifyBin resizes), the treeify test is "the number of earlier keys in key i's bin at the
# capacity in force when i is put", and the iteration order is a sort by (bucket at the final capacity, insertion).  Only the weighted
# sum stays a Python loop, so its rounding is predict()'s.

def _jhash(keys):
    k = np.asarray(keys, dtype=np.int64) & 0xFFFFFFFF
    return k ^ (k >> 16)


def _earlier_in_bin(b):
    """per position i: how many positions s < i hold the same value b[s] == b[i]"""
    if len(b) == 0:
        return np.zeros(0, dtype=np.int64)
    order = np.argsort(b, kind="stable")
    sb = b[order]
    start = np.r_[0, np.nonzero(sb[1:] != sb[:-1])[0] + 1]
    first = np.repeat(start, np.diff(np.r_[start, len(sb)]))
    occ = np.empty(len(b), dtype=np.int64)
    occ[order] = np.arange(len(b)) - first
    return occ


def hashmap_grow(keys, cap=0, thr=0):
    """JavaIntHashMap's (cap, thr) after putting the distinct `keys` in order into a table of (cap, thr) that holds no keys (cap 0: a
    new map); raises Treeified as its put does"""
    h = _jhash(keys)
    n = len(h)
    if cap == 0:
        cap, thr = 16, 12
    t = 0
    while t < n and cap < 64:  # treeifyBin resizes a table below 64 slots: walk it
        nodes = int(np.count_nonzero((h[:t] & (cap - 1)) == (h[t] & (cap - 1))))
        t += 1
        if nodes >= 8:
            cap, thr = cap * 2, thr * 2
        if t > thr:
            cap, thr = cap * 2, thr * 2
    # 64 slots and more: key i is put into the table of size i, which has doubled while i > thr
    i = np.arange(t, n)
    d = np.zeros(len(i), dtype=np.int64)
    while True:
        more = i > (thr << d)
        if not more.any():
            break
        d += more
    for dd in np.unique(d).tolist():
        c = cap << dd
        sel = i[d == dd]
        hi = int(sel[-1]) + 1
        occ = _earlier_in_bin(h[:hi] & (c - 1))
        bad = sel[occ[sel] >= 8]
        if len(bad):
            raise Treeified(int(keys[int(bad[0])]))
    while n > thr:
        cap, thr = cap * 2, thr * 2
    return cap, thr


def _iteration_order(keys, cap):
    return np.lexsort((np.arange(len(keys)), _jhash(keys) & (cap - 1)))


def predict_fast(kind, S, means, lists, u, j, knn, global_mean, bound=False, lo=1.0, hi=5.0):
    """predict() with the same contract and bits (raises Treeified for the same tuples).  lists[owner] may also be an (m, 2) array of
    (id, rating) rows; S needs only S[target] (a row indexable by the candidate ids)."""
    owner, target = (u, j) if kind == "item" else (j, u)
    cells = np.asarray(lists[owner], dtype=np.float64).reshape(-1, 2)
    ids = cells[:, 0].astype(np.int64)
    rates = cells[:, 1]
    sims = np.asarray(S[target], dtype=np.float64)[ids]
    with np.errstate(invalid="ignore"):
        keep = (sims > 0) & (rates > 0)
    keys, sims, rates = ids[keep], sims[keep], rates[keep]
    m = len(keys)
    if m:
        cap, thr = hashmap_grow(keys)
        order = _iteration_order(keys, cap)
        if 0 < knn < m:
            srt = order[np.argsort(-sims[order], kind="stable")][:knn]  # Lists.sortMap(nns, true): stable, descending
            cap, thr = hashmap_grow(keys[srt], cap, thr)  # clear() keeps the table
            order = srt[_iteration_order(keys[srt], cap)]
    if m == 0:
        pred = global_mean
    else:
        s = ws = 0.0
        for t in order.tolist():
            sim = float(sims[t])
            s += sim * (float(rates[t]) - float(means[int(keys[t])]))
            ws += abs(sim)
        pred = float(means[target]) + _div(s, ws) if ws > 0 else global_mean
    if bound:
        if pred > hi:
            pred = hi
        if pred < lo:
            pred = lo
    return pred
