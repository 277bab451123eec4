"""The host path between the C ABI and eval_kernel / ext_eval_kernel, where tests/test_gpu_eval_anchor.py holds the kernels' numbers: the
lifetime of the resident test set (cmi_set_eval_ratings: replaced by a smaller and a larger one, cleared by n = 0, dropped by new
ratings; the same through a group of two shards), calls that are refused on the host (an id out of range in the LAST tuple, a missing
ctx) and leave the handle as it was, and the tuple counts on both sides of one block's four waves.

The problem is the smallest with every part: 5 users x 7 items x 3 conditions, k = 3; BiasedMF and CAMF_CI in fp32, SVD++ in fp64.
References and bars are those of tests/eval_anchor.py (predict_ref / the oracle's predict, eval_ratings_ref, predict_bar, EXT_BAR,
measure_bars).  No call here reaches the device with a bad id: every refusal happens before anything is uploaded or launched."""
import numpy as np
import pytest

from carskit_amd import capi
from tests import eval_anchor as ea
from tests import util

pytestmark = pytest.mark.gpu

NU, NI, NC, K = 5, 7, 3, 3
CTX_LISTS = ([], [0], [1, 2], [2])
CTX_PTR = np.cumsum([0] + [len(c) for c in CTX_LISTS]).astype(np.int32)
CTX_CONDS = np.array([c for cl in CTX_LISTS for c in cl], dtype=np.int32)
N_CTX = len(CTX_LISTS)
SCALE = (1.0, 5.0)
GM = 3.137
MODELS = (("BiasedMF", False), ("CAMF_CI", False), ("SVD++", True))
IDS = [m + ("-f64" if f else "-f32") for m, f in MODELS]


class Small:
    """state, training cells and test tuples of one model, drawn once"""

    def __init__(self, model, f64, seed=7):
        self.model, self.f64 = model, f64
        rng = np.random.default_rng(seed)
        dtype = np.float64 if f64 else np.float32
        shapes = {"P": (NU, K), "Q": (NI, K), "userBias": (NU,), "itemBias": (NI,), "icBias": (NI, NC), "Y": (NI, K)}
        self.state = {n: np.ascontiguousarray((0.4 * rng.standard_normal(shapes[n])).astype(dtype)) for n in capi.MODEL_STATES[model]}
        cells = np.arange(0, NU * NI, 2)                          # every other cell: each user and each item has some
        self.train = ((cells // NI).astype(np.int32), (cells % NI).astype(np.int32), rng.integers(0, N_CTX, len(cells)).astype(np.int32),
                      rng.integers(1, 6, len(cells)).astype(np.float64))
        self.contextual = model not in ea.TWO_D

    def tuples(self, n, seed):
        """n test tuples; the first users come from both ends of the user range in turn, so that three tuples already meet both shards"""
        rng = np.random.default_rng(1000 + seed)
        u = np.concatenate([[0, NU - 1, 1, NU - 2, 2], rng.integers(0, NU, n)])[:n].astype(np.int32)
        return u, rng.integers(0, NI, n).astype(np.int32), rng.integers(0, N_CTX, n).astype(np.int32), ea.draw_ratings(rng, n, SCALE)

    def ctx_arg(self, ctx):
        return ctx if self.contextual else None

    def instance(self):
        inst = capi.Instance(self.model, K, NU, NI, NC, flags=(capi.FLAG_STATE_F64 if self.f64 else 0) |
                             (capi.FLAG_SCHED_SERIAL if self.model == "SVD++" else 0))
        inst.set_hparams(util.REG, util.REG, util.REG, util.REGC, GM)
        self.set_ratings(inst)
        inst.set_states(self.state)
        return inst

    def set_ratings(self, inst):
        tu, tj, tc, tr = self.train
        if self.contextual:
            inst.set_ratings(tu, tj, tc, tr, CTX_PTR, CTX_CONDS)
        else:
            inst.set_ratings(tu, tj, None, tr)

    def group(self):
        g = capi.Group(self.model, K, NU, NI, NC, 2, devices=[0, 0])
        g.set_hparams(util.REG, util.REG, util.REG, util.REGC, GM)
        self.set_group_ratings(g)
        g.set_states(self.state)
        return g

    def set_group_ratings(self, g):
        tu, tj, tc, tr = self.train
        g.set_ratings(tu, tj, tc if self.contextual else np.zeros(len(tu), np.int32), tr, CTX_PTR, CTX_CONDS)

    def reference(self, u, j, ctx):
        """-> (predictions, per-tuple bars) as tests/eval_anchor.py defines them"""
        if self.model in ea.MF_MODELS:
            pred, S, m = ea.predict_ref(self.model, self.state, GM, u, j, ctx, CTX_PTR, CTX_CONDS)
            return pred, ea.predict_bar(S, m, K, self.f64)
        from oracle import oracle_c
        tu, tj, tc, tr = self.train
        orc = oracle_c.SimOracle(self.model, K, NU, NI, NC, tu, tj, None, tr, CTX_PTR, CTX_CONDS, np.zeros(0, np.int32),
                                 {n: a.copy() for n, a in self.state.items()}, GM, util.REG, util.REG, util.REG, util.REGC)
        return np.array([orc.predict(int(a), int(b)) for a, b in zip(u, j)]), np.full(len(u), ea.EXT_BAR)


_SMALL = {}


def small(model, f64):
    if (model, f64) not in _SMALL:
        _SMALL[(model, f64)] = Small(model, f64)
    return _SMALL[(model, f64)]


def within(what, got, want, bar):
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    assert got.shape == want.shape and np.all(np.abs(got - want) <= bar), (what, got, want, bar)


def check_against_reference(p, res, u, j, ctx, r):
    pred, bar = p.reference(u, j, ctx)
    ev = ea.eval_ratings_ref(pred, r, *SCALE)
    ea.assert_rounding_premise(ev, bar, SCALE[0])
    bars = ea.measure_bars(ev, bar, *SCALE)
    assert res["n"] == ev.n == len(u)
    for name in ea.MEASURES:
        within(name, res[name], ev.measures[name], bars[name])


def refused(call, *parts):
    """the call fails with E_INVALID and a message that holds every part"""
    with pytest.raises(capi.CmiError) as e:
        call()
    assert e.value.code == capi.E_INVALID, e.value
    for part in parts:
        assert part in str(e.value), (part, str(e.value))


NO_SET = "call cmi_set_eval_ratings first"


# ---- the resident set's lifetime -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model,f64", MODELS, ids=IDS)
def test_resident_set_replaced_cleared_and_dropped(model, f64):
    """9 tuples sit in three blocks and 3 in one: a partials buffer kept from the larger set adds stale blocks, one sized for the smaller
    is too short for the next"""
    p = small(model, f64)
    inst = p.instance()
    refused(lambda: inst.eval_resident(*SCALE), "eval_resident:", NO_SET)
    seen = []
    for n, seed in ((9, 1), (3, 2), (9, 3)):
        u, j, ctx, r = p.tuples(n, seed)
        inst.set_eval_ratings(u, j, p.ctx_arg(ctx), r)
        res = inst.eval_resident(*SCALE)
        assert res == inst.eval_ratings(u, j, p.ctx_arg(ctx), r, *SCALE) and res["n"] == n
        assert inst.eval_resident(*SCALE) == res                  # and again: nothing is used up
        check_against_reference(p, res, u, j, ctx, r)
        seen.append(res)
    assert seen[0] != seen[2]                                     # the third set is not the first one kept
    empty = np.zeros(0, np.int32)
    inst.set_eval_ratings(empty, empty, p.ctx_arg(empty), np.zeros(0))
    refused(lambda: inst.eval_resident(*SCALE), "eval_resident:", NO_SET)
    u, j, ctx, r = p.tuples(9, 1)
    inst.set_eval_ratings(u, j, p.ctx_arg(ctx), r)
    assert inst.eval_resident(*SCALE) == seen[0]
    p.set_ratings(inst)                                           # the set indexes the context table of the ratings it came with
    refused(lambda: inst.eval_resident(*SCALE), "eval_resident:", NO_SET)
    assert inst.eval_ratings(u, j, p.ctx_arg(ctx), r, *SCALE) == seen[0]


@pytest.mark.parametrize("model,f64", MODELS[:2], ids=IDS[:2])
def test_group_resident_set_replaced_cleared_and_dropped(model, f64):
    p = small(model, f64)
    g = p.group()
    no_set = "call cmi_group_set_eval_ratings first"
    refused(lambda: g.eval_resident(*SCALE), "group_eval_resident:", no_set)
    cut = g.shard_info(0)["user_hi"]
    assert 0 < cut < NU
    sets = [p.tuples(9, 1), p.tuples(3, 2), p.tuples(9, 3)]
    u, j, ctx, r = p.tuples(9, 4)
    sets.append((u % cut, j, ctx, r))                             # every user in shard 0: shard 1's set must go, not stay from before
    sets.append((cut + u % (NU - cut), j, ctx, r))                # and every user in shard 1
    assert [sorted(set((s[0] >= cut).tolist())) for s in sets] == [[False, True], [False, True], [False, True], [False], [True]]
    for u, j, ctx, r in sets:
        g.set_eval_ratings(u, j, p.ctx_arg(ctx), r)
        res = g.eval_resident(*SCALE)
        assert res == g.eval_ratings(u, j, p.ctx_arg(ctx), r, *SCALE) and res["n"] == len(u)
        check_against_reference(p, res, u, j, ctx, r)
    empty = np.zeros(0, np.int32)
    g.set_eval_ratings(empty, empty, p.ctx_arg(empty), np.zeros(0))
    refused(lambda: g.eval_resident(*SCALE), "group_eval_resident:", no_set)
    u, j, ctx, r = sets[0]
    g.set_eval_ratings(u, j, p.ctx_arg(ctx), r)
    before = g.eval_resident(*SCALE)
    p.set_group_ratings(g)
    refused(lambda: g.eval_resident(*SCALE), "group_eval_resident:", no_set)
    g.set_states(p.state)                                         # new ratings, new shards: the state goes in again
    assert g.eval_ratings(u, j, p.ctx_arg(ctx), r, *SCALE) == before


# ---- refused calls leave the handle usable ---------------------------------------------------------------------------------------------

def bad_tuples(p, u, j, ctx):
    """(name, u, j, ctx, what the message holds): one id of the LAST tuple out of range, or no ctx at all"""
    last = len(u) - 1

    def with_last(a, v):
        b = a.copy()
        b[last] = v
        return b
    out = [("user", with_last(u, NU), j, ctx, "user/item id out of range at tuple %d" % last),
           ("item", u, with_last(j, NI), ctx, "user/item id out of range at tuple %d" % last)]
    if p.contextual:
        out.append(("context", u, j, with_last(ctx, N_CTX), "context id %d out of range at tuple %d" % (N_CTX, last)))
    return out


@pytest.mark.parametrize("model,f64", MODELS, ids=IDS)
def test_refused_instance_calls_leave_the_handle_usable(model, f64):
    p = small(model, f64)
    u, j, ctx, r = p.tuples(9, 5)
    fresh = p.instance()
    want_pred = fresh.predict(u, j, p.ctx_arg(ctx), bound=SCALE)
    want_eval = fresh.eval_ratings(u, j, p.ctx_arg(ctx), r, *SCALE)
    inst = p.instance()
    cases = [(name, bu, bj, p.ctx_arg(bc), msg) for name, bu, bj, bc, msg in bad_tuples(p, u, j, ctx)]
    none_msgs = {}
    if p.contextual:
        cases.append(("no ctx", u, j, None, None))
        none_msgs = {"predict": "eval: ctx required", "eval_ratings": "eval: ctx required", "set_eval_ratings": "set_eval_ratings: null arrays"}
    for name, bu, bj, bc, msg in cases:
        calls = {"predict": lambda: inst.predict(bu, bj, bc, bound=SCALE), "eval_ratings": lambda: inst.eval_ratings(bu, bj, bc, r, *SCALE),
                 "set_eval_ratings": lambda: inst.set_eval_ratings(bu, bj, bc, r)}
        for fn, call in calls.items():
            prefix = "set_eval_ratings: " if fn == "set_eval_ratings" else "eval: "
            refused(call, *([prefix + msg] if msg else [none_msgs[fn]]))
            if fn == "set_eval_ratings":
                refused(lambda: inst.eval_resident(*SCALE), NO_SET)          # nothing half-loaded is left behind
            assert np.array_equal(inst.predict(u, j, p.ctx_arg(ctx), bound=SCALE), want_pred), (name, fn)
            assert inst.eval_ratings(u, j, p.ctx_arg(ctx), r, *SCALE) == want_eval, (name, fn)
    inst.set_eval_ratings(u, j, p.ctx_arg(ctx), r)
    assert inst.eval_resident(*SCALE) == want_eval
    for name, bu, bj, bc, msg in cases:                           # refused before anything is released: the set loaded before it stays
        refused(lambda: inst.set_eval_ratings(bu, bj, bc, r), "set_eval_ratings: ")
        assert inst.eval_resident(*SCALE) == want_eval, name


def test_refused_fm_predict_leaves_the_handle_usable():
    rng = np.random.default_rng(3)
    w0, w, V = 3.0, 0.3 * rng.standard_normal(NU + NI + NC), 0.3 * rng.standard_normal((NU + NI + NC, K))

    def make():
        g = capi.FMInstance(K, NU, NI, NC, 1)
        g.set_model(w0, w, V)
        return g
    u, j = rng.integers(0, NU, 9).astype(np.int32), rng.integers(0, NI, 9).astype(np.int32)
    ctx = rng.integers(0, NC, 9).astype(np.int32)
    want = make().predict(u, j, ctx, bound=SCALE)
    assert np.all((want >= SCALE[0]) & (want <= SCALE[1]))
    g = make()

    def with_last(a, v):
        b = a.copy()
        b[-1] = v
        return b
    for bu, bj, bc, msg in ((with_last(u, NU), j, ctx, "fm_predict: id out of range at tuple 8"), (u, with_last(j, NI), ctx, "fm_predict: id out of range at tuple 8"),
                            (u, j, with_last(ctx, -1), "fm_predict: id out of range at tuple 8"), (u, j, None, "fm_predict: null arrays")):
        refused(lambda: g.predict(bu, bj, bc, bound=SCALE), msg)
        assert np.array_equal(g.predict(u, j, ctx, bound=SCALE), want)


def test_refused_group_eval_ratings_leaves_the_handle_usable():
    p = small("CAMF_CI", False)
    u, j, ctx, r = p.tuples(9, 6)
    want = p.group().eval_ratings(u, j, ctx, r, *SCALE)
    g = p.group()
    cut = g.shard_info(0)["user_hi"]
    shard = int(u[-1] >= cut)
    local = int(np.count_nonzero((u >= cut) == bool(shard))) - 1      # the last tuple's place among its shard's tuples
    for name, bu, bj, bc, msg in bad_tuples(p, u, j, ctx):
        if name == "user":
            msg = "eval: user id %d out of range at tuple 8" % NU        # the group routes by user: its own check, its own index
        else:
            msg = "shard %d (device 0): eval: %s" % (shard, msg.replace("tuple 8", "tuple %d" % local))
        refused(lambda: g.eval_ratings(bu, bj, bc, r, *SCALE), msg)
        assert g.eval_ratings(u, j, ctx, r, *SCALE) == want, name
    refused(lambda: g.eval_ratings(u, j, None, r, *SCALE), "eval: ctx required")
    assert g.eval_ratings(u, j, ctx, r, *SCALE) == want


# ---- both sides of one block's four waves ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model,f64", MODELS, ids=IDS)
def test_one_four_and_five_tuples(model, f64):
    """n = 4 fills one block's waves, n = 5 opens a second block whose other three waves have no tuple.  The block adds its waves as
    ((w0 + w1) + w2) + w3 and the host adds the blocks in order, so from the kernel's own bounded predictions the five measures of
    n = 4 and n = 5 follow bit for bit -- and differ by the fifth tuple's terms alone."""
    p = small(model, f64)
    inst = p.instance()
    u, j, ctx, r = p.tuples(5, 8)
    pred, bar = p.reference(u, j, ctx)
    lo, hi = SCALE
    got = {}
    for n in (1, 4, 5):
        un, jn, cn, rn = u[:n], j[:n], p.ctx_arg(ctx[:n] if p.contextual else None), r[:n]
        raw, bounded = inst.predict(un, jn, cn), inst.predict(un, jn, cn, bound=SCALE)
        within("predict", raw, pred[:n], bar[:n])
        within("bounded predict", bounded, np.clip(pred[:n], lo, hi), bar[:n])
        res = inst.eval_ratings(un, jn, cn, rn, lo, hi)
        check_against_reference(p, res, un, jn, ctx[:n], rn)
        got[n] = (bounded, res)
    bounded, _ = got[5]
    assert np.array_equal(got[4][0], bounded[:4]) and np.array_equal(got[1][0], bounded[:1])
    err, rerr = np.abs(r - bounded), np.abs(r - np.floor(bounded / lo + 0.5) * lo)
    terms = np.stack([err, err * err, rerr, rerr * rerr])        # per tuple: what it adds to each of the four sums
    block0 = ((terms[:, 0] + terms[:, 1]) + terms[:, 2]) + terms[:, 3]
    for n, sums in ((1, terms[:, 0]), (4, block0), (5, block0 + terms[:, 4])):
        mae = sums[0] / n
        want = {"MAE": mae, "RMSE": np.sqrt(sums[1] / n), "NMAE": mae / (hi - lo), "rMAE": sums[2] / n, "rRMSE": np.sqrt(sums[3] / n), "n": n}
        assert got[n][1] == want, (n, got[n][1], want)
