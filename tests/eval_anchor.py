"""predict / evalRatings anchored on their own: states that are given, not trained, rating scales other than 1..5, and the bars the
kernels are held to, derived here and not chosen.  Shared by tests/test_eval_anchor_ref.py (CPU: this module against the oracles and the
interpreted reference source, the rounding premise, the mutants) and tests/test_gpu_eval_anchor.py (GPU: eval_kernel / ext_eval_kernel
through cmi_predict_batch, cmi_eval_ratings, cmi_eval_resident and the group calls).  Nothing here imports the GPU library.

Reference prediction: a vectorised fp64 NumPy restatement of predict(u, j, c) written from the reference's sources
(BiasedMF.java:112-114, PMF.java:94-97, dev/CAMF_C.java:66-72, CAMF_CI.java:66-72, CAMF_CU.java:63-69, CAMF_CUCI.java:70-76).  With it
come, per tuple, S = the sum of the absolute values of every addend and m = their number.

Reference evalRatings: Recommender.java:504-594 line for line; the four sums run sequentially in tuple order (np.cumsum).

Bars.  The kernels compute in fp64 over the stored state.  The product of two floats is exact in fp64, so for an fp32 state kernel and
reference differ only in the order of at most m additions: any order of m additions of terms with absolute sum S is within
(m - 1) * 2^-53 * S of the exact sum, hence the two sides within b_t = 2 * m * 2^-53 * S of each other.  An fp64 state adds
k * 2^-53 * S for the rounded products.  The similarity models multiply similarities and keep the suite's absolute 1e-10
(tests/test_gpu_sim_edges.py).  The measures' bars follow from the b_t: see measure_bars()."""
import collections
import functools

import numpy as np

from tests import util

EPS = 2.0 ** -53
MEASURES = ("MAE", "RMSE", "NMAE", "rMAE", "rRMSE")
MF_MODELS = tuple(util.MODELS)
EXT_MODELS = ("SVD++", "CAMF_ICS", "CAMF_LCS", "CAMF_MCS")
EXT_BAR = 1e-10
SCALES = ((1.0, 5.0), (0.5, 5.0), (2.0, 10.0))
HAS_BU = ("BiasedMF", "CAMF_C", "CAMF_CI")
HAS_BJ = ("BiasedMF", "CAMF_C", "CAMF_CU")
TWO_D = ("BiasedMF", "PMF", "SVD++")
NO_MEAN = ("PMF", "CAMF_ICS", "CAMF_LCS", "CAMF_MCS")      # predict() does not name globalMean

# users != items, so a swapped row index reads another row; three dimensions of four conditions, contexts with zero to three of them
N_USERS, N_ITEMS, N_DIMS, CONDS_PER_DIM = 23, 37, 3, 4
N_CONDS = N_DIMS * CONDS_PER_DIM
CTX_LISTS = ([], [0], [1, 6], [3, 5, 9], [2, 7, 11], [10], [0, 4, 8])
CTX_PTR = np.cumsum([0] + [len(c) for c in CTX_LISTS]).astype(np.int32)
CTX_CONDS = np.array([c for cl in CTX_LISTS for c in cl], dtype=np.int32)
EMPTY_CONDS = np.array([d * CONDS_PER_DIM + CONDS_PER_DIM - 1 for d in range(N_DIMS)], dtype=np.int32)   # each dimension's last
BIAS_SCALE = {"userBias": 0.5, "itemBias": 0.3, "condBias": 0.2, "ucBias": 0.7, "icBias": 0.1}       # loud and pairwise distinct


def global_mean(scale):
    """a non-round number low on the scale: with factors about N(0, 0.3) and biases of 0.1 to 0.7 some predictions then fall more than
    half a level under minRate, where bounding and rounding do not commute (on 2..10 half a level is a whole unit, hence lower still)"""
    lo, hi = scale
    return lo + (0.03137 if lo > 1.0 else 0.11372) * (hi - lo)


# ---- the reference -----------------------------------------------------------------------------------------------------------------

def _context_table(ctx_ptr, ctx_conds):
    """(conds, mask): row c holds getConditions(c), padded"""
    ctx_ptr = np.asarray(ctx_ptr, dtype=np.int64)
    lens = np.diff(ctx_ptr)
    width = max(int(lens.max()) if len(lens) else 0, 1)
    conds, mask = np.zeros((len(lens), width), np.int64), np.zeros((len(lens), width), bool)
    for c in range(len(lens)):
        conds[c, :lens[c]] = ctx_conds[ctx_ptr[c]:ctx_ptr[c + 1]]
        mask[c, :lens[c]] = True
    return conds, mask


def predict_ref(model, state, gm, u, j, ctx, ctx_ptr=CTX_PTR, ctx_conds=CTX_CONDS, mutant=None):
    """-> (pred, S, m) per tuple, all float64.  `state` is used as float64 whatever its type.  mutant: None, "no-bu", "no-bj" or
    "ic-by-user" (the reference mutants of tests/test_eval_anchor_ref.py)"""
    st = {n: np.asarray(a, dtype=np.float64) for n, a in state.items() if a is not None}
    u, j = np.asarray(u, dtype=np.int64), np.asarray(j, dtype=np.int64)
    n = len(u)
    terms = []                                                   # every addend, as (n, width) blocks
    if model != "PMF":
        terms.append(np.full((n, 1), float(gm)))
    if model in HAS_BU and mutant != "no-bu":
        terms.append(st["userBias"][u][:, None])
    if model in HAS_BJ and mutant != "no-bj":
        terms.append(st["itemBias"][j][:, None])
    terms.append(st["P"][u] * st["Q"][j])                        # DenseMatrix.rowMult
    if model not in ("BiasedMF", "PMF"):
        conds, mask = _context_table(ctx_ptr, ctx_conds)
        c = np.asarray(ctx, dtype=np.int64)
        cd, mk = conds[c], mask[c]
        if model == "CAMF_C":
            terms.append(np.where(mk, st["condBias"][cd], 0.0))
        if model in ("CAMF_CI", "CAMF_CUCI"):
            row = u if mutant == "ic-by-user" and model == "CAMF_CUCI" else j
            terms.append(np.where(mk, st["icBias"][row[:, None], cd], 0.0))
        if model in ("CAMF_CU", "CAMF_CUCI"):
            terms.append(np.where(mk, st["ucBias"][u[:, None], cd], 0.0))
        n_bias = mk.sum(axis=1) * (2 if model == "CAMF_CUCI" else 1)
    else:
        n_bias = np.zeros(n, np.int64)
    with np.errstate(invalid="ignore"):
        pred = sum(t.sum(axis=1) for t in terms)
        S = sum(np.abs(t).sum(axis=1) for t in terms)
    m = n_bias + st["P"].shape[1] + (model != "PMF") + (model in HAS_BU and mutant != "no-bu") + (model in HAS_BJ and mutant != "no-bj")
    return pred, S, m.astype(np.float64)


def predict_bar(S, m, k, f64_state):
    """b_t of the six MF models (module docstring)"""
    return 2.0 * m * EPS * S + (k * EPS * S if f64_state else 0.0)


Eval = collections.namedtuple("Eval", "measures n pred rpred err rerr keep")


def eval_ratings_ref(pred, r, min_rate, max_rate, mutant=None):
    """Recommender.evalRatings over given predictions.  -> Eval(measures {name: value}, count, bounded predictions, rounded predictions,
    |rate - pred|, |rate - rPred| (the last four over the counted tuples), the mask of the counted tuples).
    mutant: None, "round-unscaled", "round-before-clip", "nmae-over-max", "nan-counted\""""
    pred, r = np.array(pred, dtype=np.float64), np.asarray(r, dtype=np.float64)
    raw = pred.copy()
    with np.errstate(invalid="ignore"):
        pred[pred > max_rate] = max_rate                          # predict(u, j, c, true): Recommender.java:309-314
        pred[pred < min_rate] = min_rate
    keep = ~np.isnan(pred) if mutant != "nan-counted" else np.ones(len(pred), bool)     # :532
    pred, raw, rate = pred[keep], raw[keep], r[keep]
    if mutant == "round-unscaled":
        rpred = np.floor(pred + 0.5)
    elif mutant == "round-before-clip":
        rpred = np.floor(raw / min_rate + 0.5) * min_rate
    else:
        rpred = np.floor(pred / min_rate + 0.5) * min_rate        # Math.round(pred / minRate) * minRate, :540
    err, rerr = np.abs(rate - pred), np.abs(rate - rpred)

    def seq(x):                                                   # sum += x, in tuple order
        return np.float64(np.cumsum(x)[-1]) if len(x) else np.float64(0.0)
    n = len(pred)
    with np.errstate(invalid="ignore", divide="ignore"):
        cnt = np.float64(n)
        mae = seq(err) / cnt
        out = {"MAE": mae, "RMSE": np.sqrt(seq(err * err) / cnt),
               "NMAE": mae / (max_rate if mutant == "nmae-over-max" else max_rate - min_rate),
               "rMAE": seq(rerr) / cnt, "rRMSE": np.sqrt(seq(rerr * rerr) / cnt)}
    return Eval({name: float(v) for name, v in out.items()}, n, pred, rpred, err, rerr, keep)


def measure_bars(ev, bars, min_rate, max_rate):
    """{measure: bar} from the per-tuple prediction bars `bars` (over all tuples; the counted ones are used).
    A clipped prediction moves by no more than the unclipped one, so |err_t| is within b_t; the rounded prediction is the same on both
    sides (the rounding premise), so rerr_t is identical and only the summation order is left.  With U = sum b_t + n 2^-53 sum |err_t|:
      the sum of absolute errors is within U                                 -> MAE, rMAE: U / n;  NMAE: U / n / (maxRate - minRate)
      the sum of squares is within V = sum 2 |err_t| b_t + n 2^-53 sum err_t^2 -> RMSE: |d sqrt(x)| = |dx| / (2 sqrt(x)), x = sum / n
    (rRMSE with rerr_t in V; where the root is 0 the bound is sqrt(V / n), from |sqrt a - sqrt b| <= sqrt |a - b|)"""
    b = np.broadcast_to(np.asarray(bars, dtype=np.float64), ev.keep.shape)[ev.keep]
    n = ev.n
    if n == 0:
        return {name: 0.0 for name in MEASURES}
    U = float(b.sum() + n * EPS * ev.err.sum())

    def root_bar(e, root):
        V = float((2.0 * e * b).sum() + n * EPS * (e * e).sum())
        return V / n / (2.0 * root) if root > 0 else float(np.sqrt(V / n))
    return {"MAE": U / n, "NMAE": U / n / (max_rate - min_rate), "rMAE": U / n,
            "RMSE": root_bar(ev.err, ev.measures["RMSE"]), "rRMSE": root_bar(ev.rerr, ev.measures["rRMSE"])}


def rounding_margin(ev, bars, min_rate):
    """the smallest distance / b_t of a counted, bounded prediction to a rounding boundary (q + 0.5) * minRate"""
    b = np.broadcast_to(np.asarray(bars, dtype=np.float64), ev.keep.shape)[ev.keep]
    x = ev.pred / min_rate
    dist = np.abs(x - np.floor(x) - 0.5) * min_rate
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.min(dist / b)) if len(b) else np.inf


PREMISE_MARGIN = 1e3


def assert_rounding_premise(ev, bars, min_rate):
    margin = rounding_margin(ev, bars, min_rate)
    assert margin >= PREMISE_MARGIN, "a prediction lies within %g bars of a rounding boundary: pick another seed" % margin


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

def loud_state(model, k, scale, seed, num_f=0):
    """fp64 draws: factors about N(0, 0.3), every bias array at its own scale (BIAS_SCALE).  PMF and the similarity models (SVD++ apart)
    have no global mean, and N(0, 0.3) factors would leave every prediction under minRate: theirs are positive and sized so that the
    dot product lands on the rating scale."""
    from carskit_amd import capi
    rng = np.random.default_rng(seed)
    shapes = {"userBias": (N_USERS,), "itemBias": (N_ITEMS,), "condBias": (N_CONDS,), "ucBias": (N_USERS, N_CONDS), "icBias": (N_ITEMS, N_CONDS)}
    st = {"P": 0.3 * rng.standard_normal((N_USERS, k)), "Q": 0.3 * rng.standard_normal((N_ITEMS, k))}
    for name in capi.MODEL_STATES[model]:
        if name in shapes:
            st[name] = BIAS_SCALE[name] * rng.standard_normal(shapes[name])
    if model == "SVD++":
        st["Y"] = 0.1 * rng.standard_normal((N_ITEMS, k))
    elif model in NO_MEAN:
        # E[dot] = k a^2 / 4 is 60 % up the scale for the middle user; the users' rows are scaled from 0.05 to 1.95 of that, so that
        # predictions cover the scale and leave it at both ends whatever k
        a = np.sqrt(4.0 * (scale[0] + 0.6 * (scale[1] - scale[0])) / k)
        st["P"] = a * rng.random((N_USERS, k)) * np.linspace(0.05, 1.95, N_USERS)[:, None]
        st["Q"] = a * rng.random((N_ITEMS, k))
        if model == "CAMF_ICS":
            c = 1.0 + 0.1 * rng.standard_normal((N_CONDS, N_CONDS))
            st["ccMatrix"] = (c + c.T) / 2
        elif model == "CAMF_LCS":
            st["cfMatrix"] = (0.8 + 0.4 * rng.random((N_CONDS, num_f))) / np.sqrt(num_f)
        elif model == "CAMF_MCS":
            st["cVector"] = (0.2 + 0.6 * rng.random(N_CONDS)) / np.sqrt(N_DIMS)
    return st


def train_tuples(model, seed=11, n=120):
    """what cmi_set_ratings gets (the context table, SVD++'s item lists): unique (user, item) pairs, every user and item present"""
    rng = np.random.default_rng(seed)
    cells = rng.choice(N_USERS * N_ITEMS, size=n, replace=False)
    cells = np.unique(np.concatenate([cells, np.arange(N_USERS) * N_ITEMS, np.arange(N_ITEMS)]))
    u, j = (cells // N_ITEMS).astype(np.int32), (cells % N_ITEMS).astype(np.int32)
    ctx = rng.integers(0, len(CTX_LISTS), len(u)).astype(np.int32)
    r = rng.integers(1, 6, len(u)).astype(np.float64)
    return u, j, (None if model in TWO_D else ctx), r


def draw_ratings(rng, n, scale):
    """rating levels of the scale: minRate, 2 minRate, ..., maxRate"""
    lo, hi = scale
    return lo * rng.integers(1, int(round(hi / lo)) + 1, n).astype(np.float64)


Case = collections.namedtuple("Case", "model k n f64 num_f seed")


def case_id(c):
    return "%s-k%d-n%d-%s%s" % (c.model, c.k, c.n, "f64" if c.f64 else "f32", "-f%d" % c.num_f if c.num_f else "")


class Problem:
    """one case, built once: the state as the GPU will store it, the eval tuples, and per scale the ratings, the reference and its bars.

    ONE state serves all three scales.  The models with a global mean get a mean per scale (global_mean), so their predictions move
    with the scale.  PMF, CAMF_ICS, CAMF_LCS and CAMF_MCS have none: their factors are sized for the 0.5..5 scale only (loud_state:
    the users' dot products run from about 0.16 to 6.2) and are reused unchanged on 1..5 and on 2..10, where they cover the lower
    half of the scale and fall under minRate for the smallest users; the reference predictions are computed once and shared."""

    def __init__(self, case):
        self.case = case
        model, k = case.model, case.k
        rng = np.random.default_rng(case.seed + 1000)
        self.u = rng.integers(0, N_USERS, case.n).astype(np.int32)
        self.j = rng.integers(0, N_ITEMS, case.n).astype(np.int32)
        self.ctx = rng.integers(0, len(CTX_LISTS), case.n).astype(np.int32)
        self.ratings = {s: draw_ratings(rng, case.n, s) for s in SCALES}
        self.train = train_tuples(model)
        # the similarity models (SVD++ apart) have no global mean to sit on a scale: their state is sized for one scale, used on all three
        dtype = np.float64 if case.f64 else np.float32
        self.state = {n: np.ascontiguousarray(a.astype(dtype)) for n, a in loud_state(model, k, SCALES[1], case.seed, case.num_f).items()}
        for a in self.state.values():
            a.setflags(write=False)
        self.gm = {s: global_mean(s) for s in SCALES}
        self.pred, self.bar, self.evals = {}, {}, {}
        for s in SCALES:
            if s != SCALES[0] and model in NO_MEAN:
                self.pred[s], self.bar[s] = self.pred[SCALES[0]], self.bar[SCALES[0]]
            else:
                self.pred[s], self.bar[s] = reference_predictions(model, self.state, self.gm[s], self.u, self.j, self.ctx, self.train, k, case.f64)
            self.evals[s] = eval_ratings_ref(self.pred[s], self.ratings[s], *s)
            assert_rounding_premise(self.evals[s], self.bar[s], s[0])

    def ctx_arg(self):
        return None if self.case.model in TWO_D else self.ctx


def sim_oracle(model, state, gm, train, k):
    from oracle import oracle_c
    tu, tj, tc, tr = train
    return oracle_c.SimOracle(model, k, N_USERS, N_ITEMS, N_CONDS, tu, tj, tc, tr, CTX_PTR, CTX_CONDS, EMPTY_CONDS, dict(state), gm,
                              util.REG, util.REG, util.REG, util.REGC, n_ctx_dims=N_DIMS)


def reference_predictions(model, state, gm, u, j, ctx, train, k, f64_state):
    """-> (pred, per-tuple bar): the NumPy restatement for the MF models, the oracle's predict (once per distinct tuple) for the others"""
    if model in MF_MODELS:
        pred, S, m = predict_ref(model, state, gm, u, j, ctx)
        return pred, predict_bar(S, m, k, f64_state)
    orc = sim_oracle(model, state, gm, train, k)
    key = (np.asarray(u, np.int64) * N_ITEMS + j) * len(CTX_LISTS) + (0 if model == "SVD++" else ctx)
    uniq, inv = np.unique(key, return_inverse=True)
    vals = np.array([orc.predict(int(q // len(CTX_LISTS) // N_ITEMS), int(q // len(CTX_LISTS) % N_ITEMS), int(q % len(CTX_LISTS))) for q in uniq])
    return vals[inv], np.full(len(u), EXT_BAR)


@functools.lru_cache(maxsize=None)
def problem(case):
    return Problem(case)


KS = (1, 63, 64, 65, 130, 256, 300)      # one lane; a ragged last pass; one pass exactly; two passes; past the training kernels' fast range
NS = (1, 3, 4, 5, 16384, 16385, 16389)   # 16 384 = 4 096 blocks x 4 waves: the two above take the grid-stride loop, n % 4 != 0 past the cap
N_SWEEP = 501


def _cases():
    sweep = [Case(m, k, N_SWEEP, f64, 7 if m == "CAMF_LCS" else 0, 100 + i) for i, (m, k, f64) in
             enumerate((m, k, f64) for m in MF_MODELS + EXT_MODELS for k in KS for f64 in (False, True))]
    sweep += [Case("CAMF_LCS", 64, N_SWEEP, f64, f, 300 + f) for f in (1, 65) for f64 in (False, True)]
    sizes = [Case(m, 65, n, False, 0, 400 + i) for i, (m, n) in enumerate((m, n) for m in ("CAMF_CUCI", "BiasedMF", "CAMF_ICS") for n in NS)]
    return sweep, sizes


SWEEP_CASES, SIZE_CASES = _cases()
PLUMBING_CASES = [Case("CAMF_CI", 65, N_SWEEP, False, 0, 501), Case("BiasedMF", 130, N_SWEEP, True, 0, 502),     # resident set, group
                  Case("CAMF_MCS", 64, N_SWEEP, False, 0, 503)]
NAN_CASES = [Case("CAMF_CU", 65, N_SWEEP, True, 0, 511), Case("CAMF_C", 64, N_SWEEP, False, 0, 512), Case("CAMF_LCS", 63, N_SWEEP, False, 7, 513)]
ALL_CASES = SWEEP_CASES + SIZE_CASES + PLUMBING_CASES + NAN_CASES


# ---- constructed ties and edges: exactly representable numbers, so every order of additions gives the same bits ----------------------

TIE_GM = 2.0
# what an item adds to the prediction of user 0 (k = 1, P = 1): predictions 2.25 (0.5-scale tie -> 2.5, truncation 2.0), 0.75, 3.75 and
# 4.75 (ties at other levels), 2.5 and 3.5 (ties of the 1-scale), 3.0 and 7.0 (ties of the 2-scale: 1.5 and 3.5 levels), exactly 5.0, 0.5,
# 1.0, 2.0 and 10.0 (the scales' ends), 6.25 and 12.5 above, 0.125 and -3.0 below, and plain values in between
TIE_PREDS = (2.25, 0.75, 3.75, 4.75, 2.5, 3.5, 3.0, 7.0, 9.0, 5.0, 0.5, 1.0, 2.0, 10.0, 6.25, 12.5, 0.125, -3.0, 2.625, 4.125, 8.375)
TIE_USER_BIAS = (0.0, 0.5, -0.25)        # users 1 and 2 shift every prediction by a representable amount: more ties, other levels
TIE_MODELS = ("BiasedMF", "CAMF_CUCI", "PMF", "CAMF_ICS")


def tie_problem(model, f64):
    """-> (state, gm, u, j, ctx, expected raw predictions).  k = 1.  Users 0..2 have P = 1 (their bias, where the model has one, is
    TIE_USER_BIAS; CAMF_CUCI carries it as ucBias of condition 0, with context 1 = [0]); user 3 has P = +inf, which bounds to maxRate
    and is counted.  PMF and CAMF_ICS have no bias and no mean: their Q holds the prediction itself."""
    dtype = np.float64 if f64 else np.float32
    nj = len(TIE_PREDS)
    assert nj <= N_ITEMS
    base = 0.0 if model in ("PMF", "CAMF_ICS") else TIE_GM
    P, Q = np.zeros((N_USERS, 1)), np.zeros((N_ITEMS, 1))
    P[:3], P[3] = 1.0, np.inf
    Q[:nj, 0] = np.array(TIE_PREDS) - base
    st = {"P": P, "Q": Q}
    shift = np.zeros(N_USERS)
    if model == "BiasedMF":
        st["userBias"], st["itemBias"] = np.zeros(N_USERS), np.zeros(N_ITEMS)
        st["userBias"][:3] = shift[:3] = TIE_USER_BIAS
    elif model == "CAMF_CUCI":
        st["ucBias"], st["icBias"] = np.zeros((N_USERS, N_CONDS)), np.zeros((N_ITEMS, N_CONDS))
        st["ucBias"][:3, 0] = shift[:3] = TIE_USER_BIAS
    elif model == "CAMF_ICS":
        st["ccMatrix"] = np.ones((N_CONDS, N_CONDS))
    u = np.repeat(np.arange(3), nj).astype(np.int32)
    j = np.tile(np.arange(nj), 3).astype(np.int32)
    pos = np.flatnonzero(np.array(TIE_PREDS) > base)             # +inf * a positive factor only
    u = np.concatenate([u, np.full(len(pos), 3, np.int32)])
    j = np.concatenate([j, pos.astype(np.int32)])
    ctx = np.ones(len(u), np.int32)
    want = np.where(u == 3, np.inf, np.array(TIE_PREDS)[j] + shift[u])
    st = {n: a.astype(dtype) for n, a in st.items()}
    assert all(np.array_equal(a.astype(np.float64), b) for a, b in zip(st.values(), (P, Q)))       # nothing was rounded
    return st, TIE_GM, u, j, ctx, want


def tie_ratings(n, scale):
    """every level of the scale in turn"""
    lo, hi = scale
    return lo * (1 + np.arange(n) % int(round(hi / lo))).astype(np.float64)
