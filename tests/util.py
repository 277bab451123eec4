"""Shared helpers for the test-suite (problem builders, oracle adapters)."""
import os

import numpy as np

from carskit_amd import synth
from oracle import oracle_np

MODELS = ["BiasedMF", "CAMF_C", "CAMF_CI", "CAMF_CU", "CAMF_CUCI", "PMF"]
TWO_D = ("BiasedMF", "PMF")   # recommenders that iterate the 2-D (user x item) train matrix

# setting.conf defaults as the doubles the reference computes with (Java float -> double)
REG = synth.java_float(1e-4)
REGC = synth.java_float(1e-3)
LR = synth.java_float(2e-2)


def small_data(n_users=23, n_items=11, n_dims=2, conds_per_dim=3, n=300, seed=7, item_zipf=None):
    return synth.generate(n_users, n_items, n_dims, conds_per_dim, n, seed=seed, item_zipf=item_zipf)


def tuples_for(model, data):
    """(u, j, ctx, r) arrays in the order the model's buildModel iterates."""
    if model in TWO_D:
        u, j, r = synth.to_2d(data)
        return u, j, np.zeros(len(r), np.int32), r
    return data.u, data.j, data.ctx, data.r


def np_model(model, data, k, state, gm, regU=REG, regI=REG, regB=REG, regC=REGC):
    conds = [data.ctx_conds[data.ctx_ptr[c]:data.ctx_ptr[c + 1]].tolist() for c in range(data.n_ctx)]
    m = oracle_np.MODELS[model](k, data.n_users, data.n_items, data.n_conds, conds, gm, regU, regI, regB, regC)
    for name, a in state.items():
        setattr(m, name, np.asarray(a, dtype=np.float64).tolist())
    return m


def np_state(m):
    out = {}
    for name in ("P", "Q", "userBias", "itemBias", "condBias", "ucBias", "icBias"):
        v = getattr(m, name)
        if v is not None:
            out[name] = np.array(v, dtype=np.float64)
    return out


def c_oracle(model, data, k, state, gm, regU=REG, regI=REG, regB=REG, regC=REGC):
    from oracle import oracle_c
    u, j, ctx, r = tuples_for(model, data)
    st = {n: np.array(a, dtype=np.float64, copy=True) for n, a in state.items()}
    return oracle_c.Oracle(model, k, data.n_users, data.n_items, data.n_conds, u, j, ctx, r, data.ctx_ptr,
                           data.ctx_conds, st, gm, regU, regI, regB, regC)


class OracleEngine:
    """The CPU oracle behind tests.hostmirror.recommender's engine interface (tests only: the product engine is
    recommender.GpuEngine)."""

    def __init__(self, model, k, data, tuples, hp, flags=0, device=0):
        from oracle import oracle_c
        self.model, self.k, self.data, self.tuples, self.hp = model, k, data, tuples, hp
        self.oracle_c = oracle_c
        self.orc = None

    def set_states(self, st):
        u, j, ctx, r = self.tuples
        st = {n: np.array(a, dtype=np.float64, copy=True) for n, a in st.items()}
        d = self.data
        if self.model in self.oracle_c.SIM_MODEL_IDS:   # SVD++ / CAMF_ICS / CAMF_LCS / CAMF_MCS: carskit_oracle_sim.c
            self.orc = self.oracle_c.SimOracle(self.model, self.k, d.n_users, d.n_items, d.n_conds, u, j, ctx, r, d.ctx_ptr, d.ctx_conds,
                                               d.empty_conds, st, self.hp["gm"], self.hp["regU"], self.hp["regI"], self.hp["regB"],
                                               self.hp["regC"], n_ctx_dims=max(1, d.n_dims))
            return
        self.orc = self.oracle_c.Oracle(self.model, self.k, d.n_users, d.n_items, d.n_conds, u, j,
                                        ctx if ctx is not None else np.zeros(len(r), np.int32), r, d.ctx_ptr,
                                        d.ctx_conds, st, self.hp["gm"], self.hp["regU"], self.hp["regI"],
                                        self.hp["regB"], self.hp["regC"])

    def get_states(self):
        return {n: a for n, a in self.orc.state.items() if a is not None}

    def epoch(self, lr):
        return self.orc.epoch(lr)

    def eval_ratings(self, u, j, ctx, r, lo, hi):
        if self.model in self.oracle_c.SIM_MODEL_IDS:    # Recommender.evalRatings (Recommender.java:504-594) over predict()
            pred = np.array([min(max(self.orc.predict(int(a), int(b), -1 if ctx is None else int(c)), lo), hi)
                             for a, b, c in zip(u, j, ctx if ctx is not None else u)])
            err = np.abs(np.asarray(r) - pred)
            rerr = np.abs(np.asarray(r) - np.floor(pred / lo + 0.5) * lo)
            n = len(err)
            mae = float(err.sum() / n)
            return {"MAE": mae, "RMSE": float(np.sqrt((err * err).sum() / n)), "NMAE": mae / (hi - lo), "rMAE": float(rerr.sum() / n),
                    "rRMSE": float(np.sqrt((rerr * rerr).sum() / n)), "n": n}
        return self.orc.eval_ratings(u, j, ctx, r, lo, hi)

    def eval_rankings(self, train, test, bin_thold, num_recs, num_ignore, strategy):
        from oracle import rank_oracle
        tup = lambda t: list(zip(*(np.asarray(a).tolist() for a in t)))
        res, _ = rank_oracle.eval_rankings(lambda u, j, c: self.orc.predict(u, j, c), tup(train), tup(test), bin_thold,
                                           num_recs, strategy, num_ignore)
        return res


# ---- builders shared by several test modules -----------------------------------------------------------------------------------

def with_env(fn, **kv):
    """fn() with the environment variables `kv` set (None = unset), restored afterwards"""
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


SIM_NUM_F = 7


def sim_data(seed=81, n=1500):
    """every dimension's last condition plays its ':na' condition (EmptyContextConditions, DataDAO.java:213-214)"""
    d = small_data(n_users=70, n_items=30, n_dims=3, conds_per_dim=4, n=n, seed=seed)
    empty = np.array([dim * 4 + 3 for dim in range(3)], dtype=np.int32)
    return d, empty


def sim_state(model, d, k, seed=7):
    rng = np.random.default_rng(seed)
    st = {"P": rng.random((d.n_users, k)), "Q": rng.random((d.n_items, k))}      # isRankingPred: P.init(), Q.init() (CAMF_ICS.java:40-46)
    if model == "SVD++":
        st = {"P": 0.1 * rng.standard_normal((d.n_users, k)), "Q": 0.1 * rng.standard_normal((d.n_items, k)),
              "userBias": 0.1 * rng.standard_normal(d.n_users), "itemBias": 0.1 * rng.standard_normal(d.n_items),
              "Y": 0.1 * rng.standard_normal((d.n_items, k))}
    elif model == "CAMF_ICS":
        st["P"] *= 0.3
        st["ccMatrix"] = np.ones((d.n_conds, d.n_conds))
    elif model == "CAMF_LCS":
        st["P"] *= 0.3
        st["cfMatrix"] = rng.random((d.n_conds, SIM_NUM_F))
    else:
        st["P"] *= 0.02      # small e * dot; at LR the positions still reach a bound within the first epoch
        st["cVector"] = (0.2 + 0.6 * rng.random(d.n_conds)) / np.sqrt(d.n_dims)
    return st


def sim_tuples(model, d):
    if model == "SVD++":
        u, j, r = synth.to_2d(d)
        return u, j, None, r
    return d.u, d.j, d.ctx, d.r


def sim_oracle(model, d, empty, k, lr_state_seed=7, regs=None):
    from oracle import oracle_c
    regs = regs or (REG, REG, REG, REGC)
    u, j, ctx, r = sim_tuples(model, d)
    st = sim_state(model, d, k, lr_state_seed)
    return oracle_c.SimOracle(model, k, d.n_users, d.n_items, d.n_conds, u, j, ctx, r, d.ctx_ptr, d.ctx_conds, empty, st,
                              oracle_c.global_mean(d.r), *regs, n_ctx_dims=d.n_dims)


def svdpp_state(nu, ni, k, seed=3):
    rng = np.random.default_rng(seed)
    return {"P": 0.1 * rng.standard_normal((nu, k)), "Q": 0.1 * rng.standard_normal((ni, k)), "userBias": 0.1 * rng.standard_normal(nu),
            "itemBias": 0.1 * rng.standard_normal(ni), "Y": 0.1 * rng.standard_normal((ni, k))}


def svdpp_oracle(u, j, r, nu, ni, k, regs=None):
    from oracle import oracle_c
    regs = regs or (REG, REG, REG, REGC)
    z = np.zeros(1, np.int32)
    return oracle_c.SimOracle("SVD++", k, nu, ni, 1, u, j, None, r, z, np.zeros(0, np.int32), np.zeros(0, np.int32),
                              svdpp_state(nu, ni, k), float(r.mean()), *regs, n_ctx_dims=1)


def svdpp_matrix(nu, ni, per_user, seed, heavy=()):
    """a 2-D train matrix in row-major order; users in `heavy` rate `heavy[u]` items"""
    rng = np.random.default_rng(seed)
    u, j = [], []
    for x in range(nu):
        m = heavy[x] if x in heavy else int(rng.integers(1, per_user + 1))
        items = np.sort(rng.choice(ni, size=min(m, ni), replace=False))
        u += [x] * len(items)
        j += items.tolist()
    r = rng.integers(1, 6, size=len(u)).astype(np.float64)
    return np.array(u, np.int32), np.array(j, np.int32), r


# ---- ItemKNN / UserKNN / SlopeOne ------------------------------------------------------------------------------------------------

def same_bits(a, b, nan_equal=True):
    """identical doubles; nan_equal: any NaN equal to any NaN (NaN marks "unset" in both)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    same = a.view(np.int64) == b.view(np.int64)
    return bool(np.all(same | (np.isnan(a) & np.isnan(b)) if nan_equal else same))


def same_bits_exact(a, b):
    """identical doubles, NaN payloads included (SlopeOne stores no NaN)"""
    return same_bits(a, b, nan_equal=False)


def assert_same_rankings(got, want, label):
    """two results of eval_rankings(with_lists=True): every measure bit for bit (NaN = NaN), every list entry for entry"""
    (res, lists), (ref, ref_lists) = got, want
    assert res.keys() == ref.keys(), label
    for m in ref:
        assert same_bits([res[m]], [ref[m]]), (label, m, res[m], ref[m])
    assert lists.keys() == ref_lists.keys(), label
    for key, ref_l in ref_lists.items():
        assert lists[key] == ref_l, (label, key, lists[key], ref_l)


def to2d(u, j, r):
    """DataDAO.toTraditionalSparseMatrix: each (user, item) cell's mean over its tuples, summed in tuple order"""
    order = np.lexsort((np.arange(len(r)), j, u))
    cells = {}
    for t in order.tolist():
        key = (int(u[t]), int(j[t]))
        s, c = cells.get(key, (0.0, 0))
        cells[key] = (s + float(r[t]), c + 1)
    keys = sorted(cells)
    return (np.array([k[0] for k in keys], np.int32), np.array([k[1] for k in keys], np.int32),
            np.array([cells[k][0] / cells[k][1] for k in keys]))


def global_mean(r):
    """SparseMatrix.getGlobalAvg of the contextual train matrix: a sequential sum over the entries / the non-zero count"""
    s = 0.0
    for v in np.asarray(r, dtype=np.float64).tolist():
        s += v
    return s / np.count_nonzero(r)


def synth_chunks_by_tiles(seed=4, n_rows=640, n_ctr=3 * 4096 + 600):
    """640 compared rows (3 chunks of 256 partners) over a contracted dimension of 4 tiles: by row mod 8, empty rows; rows only in the
    first tile; rows only in the last tile; rows with entries in every tile; rows spread over all of it with half their entries in
    the busy ranges, so pairs share entries in every tile"""
    rng = np.random.default_rng(seed)
    busy = [np.arange(t * 4096, t * 4096 + 300) for t in range(4)]
    cells = []
    for e in range(n_rows):
        kind, cnt = e % 8, int(rng.integers(1, 60))
        if kind == 0:
            continue
        if kind == 1:
            c = rng.choice(busy[0], min(cnt, 300), replace=False)
        elif kind == 2:
            c = rng.choice(busy[3], min(cnt, 300), replace=False)
        elif kind == 3:
            c = np.concatenate([rng.choice(b, max(cnt // 4, 1), replace=False) for b in busy])
        else:
            c = np.concatenate([rng.choice(np.concatenate(busy), cnt // 2 + 1, replace=False), rng.integers(0, n_ctr, cnt // 2)])
        for x in np.unique(c).tolist():
            cells.append((e, x, float(rng.integers(1, 6)) / float(rng.integers(1, 3))))
    ent = np.array([c[0] for c in cells], np.int32)
    ctr = np.array([c[1] for c in cells], np.int32)
    r = np.array([c[2] for c in cells])
    return n_rows, n_ctr, ent, ctr, r
