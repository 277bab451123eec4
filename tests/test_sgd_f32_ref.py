"""tests/sgd_f32_ref.py, the fp32 restatement the GPU kernels are held to bit for bit, is itself held to the fp64 oracle here: a
restatement written beside the kernels could share their mistake.  Host only.

Both sides start from the same fp32-rounded model and run one epoch with hparam_anchor.LOUD_REGS at util.LR; every entry of the
restatement's state must lie within a DERIVED forward bound of the oracle's, for every layout, model and k.  The bound, with
u = 2^-24 and every magnitude taken from the oracle alone (the envelope max(|before|, |after|) of its state over the epochs run):

  the error of one prediction.  pred = gm (+ bu) (+ bj) + sum_f p_f q_f (+ sum_d ctx_d) and e = rr - pred are n = k + D + 3 additions
  over k + D + 4 values (D = the context-bias terms of the tuple, two per condition for CAMF_CUCI), each value the result of at most one
  more rounding (the products; gm and the rating rounded to fp32 on the way in).  In ANY order of the additions
      |e_fp32 - e| <= de = gamma_n S,    gamma_n = n u / (1 - n u),    S = |rr| + |gm| + |bu| + |bj| + sum_f |p_f| |q_f| + sum_d |ctx_d|
  (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: each value passes through at most n roundings).  S also bounds |e|.

  the error of one update.  x' = fl(x + fl(lr fl(fl(e y) - fl(reg x)))) has five roundings; the last is relative to x', the others to
  terms no larger than lr (|e y| + reg |x|).  The owner kernels' form x' = fma(fl(lr e), y, fl(keep x)), keep = fl(1 - fl(lr reg)), has
  three roundings relative to x (keep, keep x, the result) and one relative to lr e y.  The error of e enters as lr de |y|.  For both:
      |x'_fp32 - x'| <= u (3 M_x + 3 lr (S M_y + reg M_x)) + lr de M_y
  with M_x = the largest magnitude in the row of x, M_y = the largest in the other side's row (1 for a bias, whose y is 1): three
  roundings at the row's largest magnitude, the roundings inside the step, and lr de |other row|_inf.

  an entry's bound is the SUM of that over the tuples that update it (m tuples: m times the typical term), twice over for two epochs.

What the bound leaves out: the differences already present in p, q and the biases when a later tuple reads them change its e by about
k M^2 times as much and come back scaled by lr -- a second-order term ((1 + lr k M^2)^m - 1 of the bound, a few per cent here).  The
bound is a worst case over signs while the roundings behave like a random walk, so it is slack by more than that: the recorded worst
ratio |difference| / bound over every case below is 0.29 (k = 1; under 0.25 from k = 10 on and under 0.1 at k >= 130: DESIGN.md section
21).  It is not tuned.

The mutants (sgd_f32_ref.MUTANTS) are the restatement with one deliberate mistake each; every one must leave the bound by a factor of
hparam_anchor.SEPARATION at some entry while the correct restatement of the same case stays inside it."""
import functools

import numpy as np
import pytest

from oracle import oracle_c
from tests import border_data as bd
from tests import hparam_anchor as ha
from tests import sgd_f32_ref as ref
from tests import util

U = 2.0 ** -24
KS = (1, 10, 17, 63, 64, 68, 100, 130, 252, 256)
REGS = ha.LOUD_REGS


@functools.lru_cache(maxsize=None)
def data():
    """150 x 30, four context dimensions (so the 4-lane small layout carries a condition in its last lane), about 700 tuples"""
    return util.small_data(n_users=150, n_items=30, n_dims=4, conds_per_dim=3, n=700, seed=57)


@functools.lru_cache(maxsize=None)
def case(model, k, epochs=1):
    """(problem, schedule, hparams, start, the oracle's states [start, after epoch 1, ...]) -- computed once, shared read-only"""
    d = data()
    pb = ref.problem(model, d)
    gm = oracle_c.global_mean(d.r)
    start = ref.start_state(model, d, k)
    orc = util.c_oracle(model, d, k, ref.widen(start), gm, *REGS)
    states = [ref.widen(start)]
    for _ in range(epochs):
        orc.epoch(util.LR)
        states.append({n: np.array(orc.state[n], np.float64).reshape(start[n].shape) for n in start})
    for s in states:
        for a in s.values():
            a.setflags(write=False)
    return pb, ref.schedule(pb), ref.hparams(model, util.LR, REGS, gm), start, states, gm


def forward_bound(model, pb, k, states, gm, epochs):
    """the module docstring's bound, entry by entry: {name: array}"""
    parts = ref.PARTS[model]
    env = {n: np.max([np.abs(s[n]) for s in states], axis=0) for n in states[0]}
    lr = util.LR
    regU, regI, regB, regC = REGS
    u, j, cd = pb.u, pb.j, pb.conds
    present = cd >= 0
    cdc = np.where(present, cd, 0)
    S = np.abs(pb.r.astype(np.float64)) + (0.0 if model == "PMF" else abs(gm)) + np.einsum("nk,nk->n", env["P"][u], env["Q"][j])
    D = np.zeros(pb.n)
    if "bu" in parts:
        S += env["userBias"][u]
    if "bj" in parts:
        S += env["itemBias"][j]
    if "ic" in parts:
        S += np.where(present, env["icBias"][j[:, None], cdc], 0.0).sum(axis=1)
        D += present.sum(axis=1)
    if "uc" in parts:
        S += np.where(present, env["ucBias"][u[:, None], cdc], 0.0).sum(axis=1)
        D += present.sum(axis=1)
    if "bc" in parts:
        S += np.where(present, env["condBias"][cdc], 0.0).sum(axis=1)
        D += present.sum(axis=1)
    n = k + D + 3
    de = n * U / (1 - n * U) * S

    def one(mx, my, reg):
        return U * (3 * mx + 3 * lr * (S * my + reg * mx)) + lr * de * my

    mp, mq = env["P"][u].max(axis=1), env["Q"][j].max(axis=1)
    out = {name: np.zeros_like(a) for name, a in env.items()}
    np.add.at(out["P"], u, one(mp, mq, regU)[:, None])
    np.add.at(out["Q"], j, one(mq, mp, regI)[:, None])
    if "bu" in parts:
        np.add.at(out["userBias"], u, one(env["userBias"][u], 1.0, regB))
    if "bj" in parts:
        np.add.at(out["itemBias"], j, one(env["itemBias"][j], 1.0, regB))
    rows, cols = np.nonzero(present)
    for part, name, ids in (("ic", "icBias", j), ("uc", "ucBias", u)):
        if part in parts:
            cell = (ids[rows], cd[rows, cols])
            mx = env[name][cell]
            np.add.at(out[name], cell, U * (3 * mx + 3 * lr * (S[rows] + regC * mx)) + lr * de[rows])
    if "bc" in parts:
        mx = env["condBias"][cd[rows, cols]]
        np.add.at(out["condBias"], cd[rows, cols], U * (3 * mx + 3 * lr * (S[rows] + regC * mx)) + lr * de[rows])
    return {name: epochs * a for name, a in out.items()}


def worst_ratio(state, oracle_state, bound):
    """max over entries of |difference| / bound; an entry no tuple updates has bound 0 and must not differ at all"""
    worst = 0.0
    for name, b in bound.items():
        diff = np.abs(np.asarray(state[name], np.float64) - oracle_state[name])
        assert not np.any((b == 0) & (diff != 0)), name
        live = b > 0
        if np.any(live):
            worst = max(worst, float(np.max(diff[live] / b[live])))
    return worst


def run(model, k, layout, mut=None, epochs=1):
    pb, sched, hp, start, states, gm = case(model, k, epochs)
    st = {n: a.copy() for n, a in start.items()}
    losses = [ref.epoch(st, pb, hp, layout, sched, mut if e == 0 else None)[0] for e in range(epochs)]
    return st, losses


# ---- the restatement's own pieces ------------------------------------------------------------------------------------------------
def test_every_lane_of_a_group_ends_with_the_same_bits():
    """row_sum16 and group_sum<LPT> pair the same operands in every lane (the restatement reads lane 0)"""
    rng = np.random.default_rng(1)
    x = rng.standard_normal((200, 16)).astype(np.float32)
    full = ref._row_sum16(x)
    assert np.all(full.view(np.int32) == full[:, :1].view(np.int32))
    for lpt in (4, 8, 16):
        x = rng.standard_normal((200, lpt)).astype(np.float32)
        full = ref._group_sum(x, lpt)
        assert np.all(full.view(np.int32) == full[:, :1].view(np.int32))


def test_layout_rules_cover_every_kernel_shape():
    """with_fast_shape's VPL x RAGGED instances and small_lpt's three lane counts, at the k of the GPU module"""
    shapes = {ref.level_layout(k, 4) for k in (64, 128, 256, 68, 100, 124, 132, 188, 192, 200, 252)}
    assert shapes == {("fast", 1, False), ("fast", 2, False), ("fast", 4, False), ("fast", 2, True), ("fast", 3, True), ("fast", 4, True)}
    assert ref.level_layout(124, 4) == ("fast", 2, True) and ref.level_layout(132, 4) == ("fast", 3, True)
    assert ref.level_layout(188, 4) == ("fast", 3, True) and ref.level_layout(192, 4) == ("fast", 4, True)
    assert [ref.small_lpt(k, d) for k, d in ((1, 1), (16, 4), (17, 3), (10, 5), (32, 8), (33, 2), (10, 16), (63, 12))] == [4, 4, 8, 8, 8, 16, 16, 16]
    assert ref.level_layout(70, 4) == ("wave64",) and ref.level_layout(130, 3) == ("wave64",) and ref.level_layout(64, 17) == ("wave64",)
    assert ref.serial_layout(10) == ("serial_fast", 1) and ref.serial_layout(128) == ("serial_fast", 2) and ref.serial_layout(260) == ("wave64",)


@pytest.mark.parametrize("model", ref.MODELS)
@pytest.mark.parametrize("k", [10, 68])
def test_level_order_and_crs_order_give_the_same_bits(model, k):
    """the order-exactness the GPU bars rest on: a level at a time (vectorised) against the plain loop in the reference's order"""
    pb, sched, hp, start, _, _ = case(model, k)
    perm, off = sched
    assert len(off) - 1 > 1 and np.max(np.diff(off)) > 1
    for layout in ref.layouts_for(k, pb.dmax):
        a = {n: x.copy() for n, x in start.items()}
        b = {n: x.copy() for n, x in start.items()}
        la, ta = ref.epoch(a, pb, hp, layout, sched)
        lb, tb = ref.epoch_crs(b, pb, hp, layout)
        for name in a:
            assert np.array_equal(a[name].view(np.int32), b[name].view(np.int32)), (layout, name)
        assert la == lb                                                  # fsum: the exactly rounded sum of the same terms
        assert np.array_equal(ta[np.argsort(perm, kind="stable")], tb)   # ... tuple for tuple


# ---- against the oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ref.MODELS)
@pytest.mark.parametrize("k", KS)
def test_every_layout_within_the_derived_bound_of_the_oracle(model, k):
    pb, sched, hp, start, states, gm = case(model, k)
    bound = forward_bound(model, pb, k, states, gm, 1)
    layouts = ref.layouts_for(k, pb.dmax)
    assert ("wave64",) in layouts and ("sequential",) in layouts
    for layout in layouts:
        st, _ = run(model, k, layout)
        ratio = worst_ratio(st, states[1], bound)
        print("worst |difference| / bound: %-12s k=%-3d %-22r %.4f" % (model, k, layout, ratio))
        assert ratio <= 1.0, (layout, ratio)


@pytest.mark.parametrize("k", [10, 64, 130])
def test_camf_c_within_the_derived_bound_of_the_oracle(k):
    """CAMF_C through epoch_camfc, its three layouts; condBias is updated by every tuple that names the condition, and bounded so"""
    pb, _, hp, start, states, gm = case("CAMF_C", k)
    bound = forward_bound("CAMF_C", pb, k, states, gm, 1)
    d = data()
    want = util.c_oracle("CAMF_C", d, k, ref.widen(start), gm, *REGS).epoch(util.LR)
    for name, layout in sorted(ref.camfc_layouts(k).items()):
        st = {n: a.copy() for n, a in start.items()}
        loss = ref.epoch_camfc(st, pb, hp, layout, ref.camfc_blocks(pb))
        ratio = worst_ratio(st, states[1], bound)
        print("worst |difference| / bound: %-12s k=%-3d %-22r %.4f" % ("CAMF_C", k, layout, ratio))
        assert ratio <= 1.0, (layout, ratio)
        assert abs(loss - want) <= 2e-6 * abs(want), (layout, loss, want)


@pytest.mark.parametrize("n_dims,cpd,ragged,k", [c for c in bd.CAMFC_CASES if c[2] or c[0] >= 8])
def test_camf_c_border_data_within_the_derived_bound_of_the_oracle(n_dims, cpd, ragged, k):
    """epoch_camfc where tests/test_gpu_camfc_blocks_borders.py relies on it: ragged contexts (a context with no condition among them),
    8 and 16 dimensions, blocks of exactly 64 tuples one after another, 64 to 344 conditions"""
    d = bd.camfc_data(n_dims, cpd, ragged)
    pb = ref.problem("CAMF_C", d)
    blk = ref.camfc_blocks(pb)
    lens = np.diff(blk)
    assert pb.dmax == n_dims and np.any((lens[:-1] == 64) & (lens[1:] == 64)) and (np.any(pb.conds < 0) == ragged)
    gm = oracle_c.global_mean(d.r)
    hp = ref.hparams("CAMF_C", util.LR, REGS, gm)
    start = ref.start_state("CAMF_C", d, k)
    orc = util.c_oracle("CAMF_C", d, k, ref.widen(start), gm, *REGS)
    want = orc.epoch(util.LR)
    after = {n: np.array(orc.state[n], np.float64).reshape(start[n].shape) for n in start}
    bound = forward_bound("CAMF_C", pb, k, [ref.widen(start), after], gm, 1)
    for name, layout in sorted(ref.camfc_layouts(k).items()):
        st = {n: a.copy() for n, a in start.items()}
        loss = ref.epoch_camfc(st, pb, hp, layout, blk)
        ratio = worst_ratio(st, after, bound)
        print("worst |difference| / bound: %-12s k=%-3d dims=%-2d %-22r %.4f" % ("CAMF_C", k, n_dims, layout, ratio))
        assert ratio <= 1.0, (layout, ratio)
        assert abs(loss - want) <= 2e-6 * abs(want), (layout, loss, want)


def test_loss_is_the_oracles_to_fp32_accuracy():
    """the loss terms: the epoch loss of the restatement against the oracle's, to the accuracy of fp32 terms (2e-6 relative; the old fp32
    bars allow 2e-5)"""
    for model in ref.MODELS:
        for k in (10, 100):
            pb, sched, hp, start, states, gm = case(model, k)
            d = data()
            orc = util.c_oracle(model, d, k, ref.widen(start), gm, *REGS)
            want = orc.epoch(util.LR)
            for layout in ref.layouts_for(k, pb.dmax):
                _, losses = run(model, k, layout)
                assert abs(losses[0] - want) <= 2e-6 * abs(want), (model, k, layout, losses[0], want)


# ---- the mutants -----------------------------------------------------------------------------------------------------------------
def _mutant_cases():
    out = []
    for model in ("BiasedMF", "CAMF_CUCI"):
        out += [("q_from_new_p", model, 10), ("q_from_new_p", model, 100), ("reg_on_new", model, 10), ("reg_on_new", model, 64)]
    for model in ("PMF", "CAMF_CI"):
        out += [("drop_last_factor", model, 10), ("drop_last_factor", model, 100), ("slot_past_k", model, 10), ("slot_past_k", model, 100)]
    for model in ("CAMF_CI", "CAMF_CU", "CAMF_CUCI"):
        out.append(("drop_ctx_lane", model, 10))
    for model in ("CAMF_CI", "CAMF_CU"):
        out += [("bias_e_without_ctx", model, 10), ("bias_e_without_ctx", model, 64)]
    for model in ("BiasedMF", "CAMF_CU"):
        out += [("drop_tuple", model, 10), ("drop_tuple", model, 128), ("stale_user_row", model, 10), ("stale_user_row", model, 128)]
    return out


def _applicable(name, model, k, pb, layout, sched):
    """what makes the mutant a different computation on this case, read from the model's table and the data alone; -> the mutant"""
    parts = ref.PARTS[model]
    if name == "reg_on_new":
        assert REGS[0] > 0
    if name == "drop_last_factor":
        assert k not in (64, 128, 256)                                   # a ragged k
    if name == "slot_past_k":
        assert ref.width(layout, k) > k and pb.n_users > 1               # there are slots past k, and a row after the row
    if name == "drop_ctx_lane":
        assert layout[0] in ref.GROUP_KINDS and ("ic" in parts or "uc" in parts)
        assert pb.dmax == ref.lane_count(layout) and np.any(pb.conds[:, -1] >= 0)     # some tuple has a condition in the last lane
    if name == "bias_e_without_ctx":
        assert ("bu" in parts or "bj" in parts) and ("ic" in parts or "uc" in parts) and np.any(pb.conds >= 0)
    if name == "drop_tuple":
        return (name, int(sched[0][len(sched[0]) // 3]))
    if name == "stale_user_row":
        found = ref.stale_candidate(pb, sched)
        assert found is not None
        return (name, found[0])
    return (name,)


@pytest.mark.parametrize("name,model,k", _mutant_cases())
def test_each_mutant_leaves_the_bound_by_the_separation(name, model, k):
    epochs = 2 if name == "drop_tuple" else 1
    pb, sched, hp, start, states, gm = case(model, k, epochs)
    layout = ref.level_layout(k, pb.dmax)
    mut = _applicable(name, model, k, pb, layout, sched)
    bound = forward_bound(model, pb, k, states, gm, epochs)
    good, _ = run(model, k, layout, None, epochs)
    bad, _ = run(model, k, layout, mut, epochs)
    inside, outside = worst_ratio(good, states[-1], bound), worst_ratio_of_mutant(bad, states[-1], bound)
    print("mutant %-20s %-10s k=%-3d correct %.4f, mutant %.1f x the bound" % (name, model, k, inside, outside))
    assert inside <= 1.0
    assert outside >= ha.SEPARATION, (name, outside)


def worst_ratio_of_mutant(state, oracle_state, bound):
    """worst_ratio without its demand that untouched entries stay put (a mutant may write where the model does not)"""
    worst = 0.0
    for name, b in bound.items():
        diff = np.abs(np.asarray(state[name], np.float64) - oracle_state[name])
        live = b > 0
        if np.any(live):
            worst = max(worst, float(np.max(diff[live] / b[live])))
        if np.any(~live & (diff != 0)):
            worst = float("inf")
    return worst


def test_every_mutant_has_a_case():
    assert {c[0] for c in _mutant_cases()} == set(ref.MUTANTS)
