"""CAMF_ICS / CAMF_LCS / CAMF_MCS on the GPU (carskit_amd/csrc/ext_kernels.hip) where tests/test_gpu_sim_models.py does not
look: the fp32 default path, the saturated regime, and shapes that leave lanes idle or give a lane two factors.

References: the fp64 oracle (oracle/carskit_oracle_sim.c) and, for fp32 state, tests/sim_ref.py in float32 -- the kernel's
own rounding, pinned to the oracle in float64 by tests/test_sim_ref.py.  Bars:
  * STRICT (one lane, the reference's order): state and per-epoch loss bit-identical to the reference of the same type;
  * wave: fp64 state within 1e-11, loss within 1e-12 relative, predictions within 1e-10; fp32 predictions within 2e-4 of
    max(1, |pred|), loss within 2e-5 relative;
  * saturated regime (the reference's init and learning rate 2e-2): CAMF_MCS parks positions on both bounds, where a
    different rounding is a different trajectory, so the wave kernels are held to finiteness and to [0, upbound]."""
import math

import numpy as np
import pytest

from carskit_amd import capi, synth
from oracle import oracle_c, rank_oracle
from tests import sim_ref, util
from tests.test_sim_ref import SATURATED, assert_at_both_bounds, data, oracle, reference_state, restatement

pytestmark = pytest.mark.gpu
F64, SERIAL, STRICT = capi.FLAG_STATE_F64, capi.FLAG_SCHED_SERIAL, capi.FLAG_STRICT
SIM_MODELS = ["CAMF_ICS", "CAMF_LCS", "CAMF_MCS"]
LR = util.LR / 8


def rate(model):
    """CAMF_MCS moves a condition away from its ':na' partner whenever it under-predicts, so at LR every position of these
    problems runs to a bound within an epoch; at LR / 128 none reaches one in three epochs"""
    return LR / 128 if model == "CAMF_MCS" else LR


def smooth_state(model, d, k, num_f, seed=7):
    """small P and, for CAMF_LCS, vectors whose dot product (a pair's similarity) is 1 +- 0.2 whatever numF"""
    st = reference_state(model, d, k, num_f, seed)
    st["P"] *= 0.3 if model != "CAMF_MCS" else 0.02
    if model == "CAMF_LCS":
        st["cfMatrix"] = (0.8 + 0.4 * st["cfMatrix"]) / np.sqrt(num_f)
    elif model == "CAMF_MCS":
        st["cVector"] = (0.2 + 0.6 * np.sqrt(d.n_dims) * st["cVector"]) / np.sqrt(d.n_dims)
    return st


def gpu(model, d, empty, k, num_f, st, flags):
    inst = capi.Instance(model, k, d.n_users, d.n_items, d.n_conds, flags=flags | SERIAL)
    inst.set_hparams(util.REG, util.REG, util.REG, util.REGC, oracle_c.global_mean(d.r))
    inst.set_sim_params(max(num_f, 1), d.n_dims, empty)
    inst.set_ratings(d.u, d.j, d.ctx, d.r, d.ctx_ptr, d.ctx_conds)
    inst.set_states(st)
    return inst


def finite(st):
    return all(np.isfinite(a).all() for a in st.values())


def assert_state_equal(want, got):
    for name, a in got.items():
        assert np.array_equal(np.asarray(want[name], dtype=np.float64).reshape(a.shape), a), name


# ---- the saturated regime ---------------------------------------------------------------------------------------------

def test_saturated_mcs_f64_strict_bit_exact():
    d, empty = data()
    st = reference_state("CAMF_MCS", d, 10, 0)
    orc, inst = oracle("CAMF_MCS", d, empty, 10, st), gpu("CAMF_MCS", d, empty, 10, 0, st, F64 | STRICT)
    for _ in range(5):
        lo, lg = orc.epoch(util.LR), inst.train_epoch(util.LR)
        assert np.isfinite(lo) and lo == lg
    assert_state_equal(orc.state, inst.get_states())
    assert_at_both_bounds(orc.state["cVector"], d.n_dims)


@pytest.mark.parametrize("model", SIM_MODELS)
def test_saturated_f32_strict_matches_f32_restatement(model):
    """CAMF_MCS: a float position chain stores 1e-100 as 0 and turns 0/0 = NaN once two paired conditions share a bound"""
    d, empty = data()
    num_f = SATURATED[model]
    st = reference_state(model, d, 10, num_f)
    orc, ref, inst = oracle(model, d, empty, 10, st), restatement(model, np.float32, d, empty, st), gpu(model, d, empty, 10, num_f, st, STRICT)
    losses = [(orc.epoch(util.LR), ref.epoch(util.LR), inst.train_epoch(util.LR)) for _ in range(5)]
    got = inst.get_states()
    assert all(np.isfinite(lo) and np.isfinite(lg) for lo, _, lg in losses), losses
    assert finite(got)
    assert [lg for _, _, lg in losses] == [lr_ for _, lr_, _ in losses]
    assert_state_equal(ref.state, got)
    if model == "CAMF_MCS":
        cv, upbound = got["cVector"], float(np.float32(1 / np.sqrt(d.n_dims)))
        assert np.count_nonzero(cv == 0.0) >= 2 and np.count_nonzero(cv == upbound) >= 2


@pytest.mark.parametrize("model", SIM_MODELS)
@pytest.mark.parametrize("flags", [0, F64], ids=["f32", "f64"])
def test_saturated_wave_stays_finite_and_in_bounds(model, flags):
    d, empty = data()
    num_f = SATURATED[model]
    st = reference_state(model, d, 10, num_f)
    orc, inst = oracle(model, d, empty, 10, st), gpu(model, d, empty, 10, num_f, st, flags)
    for epoch in range(5):
        lo, lg = orc.epoch(util.LR), inst.train_epoch(util.LR)
        assert np.isfinite(lo) and np.isfinite(lg), epoch
    got = inst.get_states()
    assert finite(got)
    if model == "CAMF_MCS":
        assert got["cVector"].min() >= 0.0 and got["cVector"].max() <= 1 / np.sqrt(d.n_dims)


# ---- wave-kernel shapes: idle lanes, two factors per lane, numF past one wave, 1 to 16 conditions ---------------------

SHAPES = ([(m, k, 7, 3) for m in SIM_MODELS for k in (1, 5, 63, 65, 128, 130)]
          + [("CAMF_LCS", 64, f, 3) for f in (1, 64, 65, 130)]
          + [(m, 65, 7, w) for m in SIM_MODELS for w in (1, 8, 16)])


@pytest.mark.parametrize("model,k,num_f,n_dims", SHAPES)
def test_wave_shapes(model, k, num_f, n_dims):
    d, empty = data(n_dims=n_dims, conds_per_dim=3, n=2500, seed=82)
    train, test = synth.split(d, 0.2)
    st = smooth_state(model, train, k, num_f)
    tup = list(zip(test.u.tolist(), test.j.tolist(), test.ctx.tolist()))
    orc, inst = oracle(model, train, empty, k, st), gpu(model, train, empty, k, num_f, st, F64)
    for _ in range(3):
        lo, lg = orc.epoch(rate(model)), inst.train_epoch(rate(model))
        assert np.isfinite(lo) and abs(lo - lg) <= 1e-12 * abs(lo)
    for name, a in inst.get_states().items():
        assert np.max(np.abs(orc.state[name].reshape(a.shape) - a)) <= 1e-11, name
    want = np.array([orc.predict(u, j, c) for u, j, c in tup])
    assert np.max(np.abs(inst.predict(test.u, test.j, test.ctx) - want)) <= 1e-10

    ref, inst = restatement(model, np.float32, train, empty, st), gpu(model, train, empty, k, num_f, st, 0)
    for _ in range(3):
        lr_, lg = ref.epoch(rate(model)), inst.train_epoch(rate(model))
        assert abs(lr_ - lg) <= 2e-5 * abs(lr_)
    want = np.array([float(ref.predict(u, j, c)) for u, j, c in tup])
    got = inst.predict(test.u, test.j, test.ctx)
    assert np.all(np.abs(got - want) <= 2e-4 * np.maximum(1.0, np.abs(want)))


@pytest.mark.parametrize("model,num_f,n_dims", [("CAMF_ICS", 0, 16), ("CAMF_LCS", 7, 16), ("CAMF_MCS", 0, 16), ("CAMF_LCS", 130, 3)])
def test_strict_f64_bit_exact_wide(model, num_f, n_dims):
    d, empty = data(n_dims=n_dims, conds_per_dim=3, n=1500, seed=84)
    st = smooth_state(model, d, 10, num_f)
    orc, inst = oracle(model, d, empty, 10, st), gpu(model, d, empty, 10, num_f, st, F64 | STRICT)
    for _ in range(3):
        lo, lg = orc.epoch(rate(model)), inst.train_epoch(rate(model))
        assert np.isfinite(lo) and lo == lg
    assert_state_equal(orc.state, inst.get_states())


@pytest.mark.parametrize("model", SIM_MODELS)
def test_predict_and_eval_ratings_wide(model):
    """ext_eval_kernel at k = 130, numF = 130, 16 conditions per context: fp64 against the oracle's predict"""
    d, empty = data(n_dims=16, conds_per_dim=3, n=2000, seed=85)
    train, test = synth.split(d, 0.3)
    st = smooth_state(model, train, 130, 130)
    orc, inst = oracle(model, train, empty, 130, st), gpu(model, train, empty, 130, 130, st, F64)
    orc.epoch(rate(model))
    inst.train_epoch(rate(model))
    want = np.array([orc.predict(u, j, c) for u, j, c in zip(test.u.tolist(), test.j.tolist(), test.ctx.tolist())])
    assert np.isfinite(want).all() and np.ptp(want) > 0
    assert np.max(np.abs(inst.predict(test.u, test.j, test.ctx) - want)) <= 1e-10
    lo, hi = 1.0, 5.0
    bounded = np.clip(want, lo, hi)
    err, rerr = np.abs(test.r - bounded), np.abs(test.r - np.floor(bounded / lo + 0.5) * lo)
    res = inst.eval_ratings(test.u, test.j, test.ctx, test.r, lo, hi)
    assert res["n"] == len(want)
    for m, v in (("MAE", err.mean()), ("RMSE", np.sqrt((err * err).mean())), ("rMAE", rerr.mean()), ("rRMSE", np.sqrt((rerr * rerr).mean()))):
        assert abs(res[m] - v) <= 1e-10, m


@pytest.mark.parametrize("model", SIM_MODELS)
@pytest.mark.parametrize("k", [5, 70])
def test_f32_rankings_close_to_oracle(model, k):
    """ext_rank_queries<float> / ext_rank_items<float> over 200 items (four 64-candidate tiles): rank_oracle driven by the
    oracle's predict over the model the fp32 GPU trained"""
    d, empty = data(n=3000, seed=86, n_items=200)
    train, test = synth.split(d, 0.25)
    num_f = 7 if model == "CAMF_LCS" else 0
    inst = gpu(model, train, empty, k, num_f, smooth_state(model, train, k, num_f), 0)
    for _ in range(2):
        inst.train_epoch(rate(model))
    orc = oracle(model, train, empty, k, inst.get_states())
    tup = lambda t: list(zip(t.u.tolist(), t.j.tolist(), t.ctx.tolist(), t.r.tolist()))
    ref, ref_lists = rank_oracle.eval_rankings(lambda u, j, c: orc.predict(u, j, c), tup(train), tup(test), bin_thold=-1.0,
                                               num_recs=10, strategy="ucu", num_ignore=-1)
    res, lists = inst.eval_rankings((train.u, train.j, train.ctx, train.r), (test.u, test.j, test.ctx, test.r), bin_thold=-1.0,
                                    num_recs=10, num_ignore=-1, strategy="ucu", with_lists=True)
    assert res.pop("n_queries") == len(ref_lists) > 50
    assert set(lists) == set(ref_lists)
    same = 0
    for key, want in ref_lists.items():
        got = lists[key]
        assert len(got) == len(want), key
        same += [i for i, _ in got] == [i for i, _ in want]
        for (_, a), (_, b) in zip(got, want):
            assert abs(a - b) <= 1e-4 * max(1.0, abs(b)), (key, a, b)
    assert same >= 0.9 * len(ref_lists)
    for m in rank_oracle.MEASURES:
        a, b = res[m], ref[m]
        assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 0.02, (m, a, b)


def test_seventeen_conditions_are_refused():
    d, empty = data(n_dims=17, conds_per_dim=2, n=200, seed=87)
    inst = capi.Instance("CAMF_MCS", 8, d.n_users, d.n_items, d.n_conds, flags=SERIAL)
    inst.set_sim_params(1, d.n_dims, empty)
    with pytest.raises(capi.CmiError) as ei:
        inst.set_ratings(d.u, d.j, d.ctx, d.r, d.ctx_ptr, d.ctx_conds)
    assert ei.value.code == capi.E_UNSUPPORTED
