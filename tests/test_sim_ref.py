"""tests/sim_ref.py (the dtype-parameterised restatement of ext_serial_strict) against oracle/carskit_oracle_sim.c: with
float64 it must be the oracle bit for bit, in the state and in every epoch's loss, so that with float32 it is the reference
the fp32 kernels are held to (tests/test_gpu_sim_edges.py).  Run in the saturated regime -- the reference's init and its
learning rate 2e-2 -- where CAMF_MCS parks positions on both bounds and the clipping branches are exercised."""
import numpy as np
import pytest

from oracle import oracle_c
from tests import sim_ref, util

N_USERS, N_ITEMS = 70, 30


def data(n_dims=3, conds_per_dim=4, n=1500, seed=81, n_items=N_ITEMS):
    """every dimension's last condition plays its ':na' condition (EmptyContextConditions, DataDAO.java:213-214)"""
    d = util.small_data(n_users=N_USERS, n_items=n_items, n_dims=n_dims, conds_per_dim=conds_per_dim, n=n, seed=seed)
    return d, np.array([dim * conds_per_dim + conds_per_dim - 1 for dim in range(n_dims)], dtype=np.int32)


def reference_state(model, d, k, num_f, seed=7):
    """initModel of the reference: P.init(), Q.init() (U(0,1)), ccMatrix = 1, cfMatrix.init(), cVector.init(upbound)"""
    rng = np.random.default_rng(seed)
    st = {"P": rng.random((d.n_users, k)), "Q": rng.random((d.n_items, k))}
    if model == "CAMF_ICS":
        st["ccMatrix"] = np.ones((d.n_conds, d.n_conds))
    elif model == "CAMF_LCS":
        st["cfMatrix"] = rng.random((d.n_conds, num_f))
    else:
        st["cVector"] = rng.random(d.n_conds) / np.sqrt(d.n_dims)
    return st


def oracle(model, d, empty, k, st):
    return oracle_c.SimOracle(model, k, d.n_users, d.n_items, d.n_conds, d.u, d.j, d.ctx, d.r, d.ctx_ptr, d.ctx_conds, empty,
                              {n: a.copy() for n, a in st.items()}, oracle_c.global_mean(d.r), util.REG, util.REG, util.REG,
                              util.REGC, n_ctx_dims=d.n_dims)


def restatement(model, dtype, d, empty, st):
    return sim_ref.SimRef(model, dtype, d.u, d.j, d.ctx, d.r, d.ctx_ptr, d.ctx_conds, empty, st, util.REG, util.REG, util.REGC, d.n_dims)


# CAMF_LCS: numF = 4 (the driver's default numF = 7 diverges to NaN in fp64 on this data at k = 10 and rate 2e-2)
SATURATED = {"CAMF_ICS": 0, "CAMF_LCS": 4, "CAMF_MCS": 0}


def assert_at_both_bounds(cv, n_dims):
    upbound = 1.0 / np.sqrt(n_dims)
    assert np.count_nonzero(cv == sim_ref.LOWBOUND) >= 2, cv
    assert np.count_nonzero(cv == upbound - sim_ref.LOWBOUND) >= 2, cv


@pytest.mark.parametrize("model", sorted(SATURATED))
def test_f64_restatement_is_the_oracle_in_the_saturated_regime(model):
    d, empty = data()
    st = reference_state(model, d, 10, SATURATED[model])
    orc, ref = oracle(model, d, empty, 10, st), restatement(model, np.float64, d, empty, st)
    for _ in range(5):
        lo, lr_ = orc.epoch(util.LR), ref.epoch(util.LR)
        assert np.isfinite(lo) and lo == lr_
    for name, a in ref.state.items():
        assert np.array_equal(orc.state[name].reshape(a.shape), a), name
    if model == "CAMF_MCS":
        assert_at_both_bounds(orc.state["cVector"], d.n_dims)
    for u, j, c in zip(d.u[:50].tolist(), d.j[:50].tolist(), d.ctx[:50].tolist()):
        assert ref.predict(u, j, c) == orc.predict(u, j, c)


@pytest.mark.parametrize("model,num_f,n_dims,k", [("CAMF_ICS", 0, 16, 3), ("CAMF_LCS", 65, 8, 5), ("CAMF_MCS", 0, 16, 3),
                                                   ("CAMF_MCS", 0, 1, 70)])
def test_f64_restatement_is_the_oracle_at_wide_shapes(model, num_f, n_dims, k):
    """contexts of 1 to 16 conditions, numF past one wave, k past one wave; smooth-regime state (small P)"""
    d, empty = data(n_dims=n_dims, conds_per_dim=3, n=600, seed=5)
    st = reference_state(model, d, k, num_f, seed=11)
    st["P"] *= 0.02
    if model == "CAMF_LCS":
        st["cfMatrix"] *= 1.0 / np.sqrt(num_f)
    orc, ref = oracle(model, d, empty, k, st), restatement(model, np.float64, d, empty, st)
    for _ in range(2):
        lo, lr_ = orc.epoch(util.LR / 8), ref.epoch(util.LR / 8)
        assert np.isfinite(lo) and lo == lr_
    for name, a in ref.state.items():
        assert np.array_equal(orc.state[name].reshape(a.shape), a), name


def test_f32_mcs_stays_finite_where_a_float_position_chain_turns_nan():
    """the saturated CAMF_MCS run in float32: finite, positions in [0, upbound] and on both bounds (stored 1e-100 is 0 in
    float).  The float32 restatement differs from the float64 one only in rounding, so its loss stays near the oracle's."""
    d, empty = data()
    st = reference_state("CAMF_MCS", d, 10, 0)
    r32, r64 = restatement("CAMF_MCS", np.float32, d, empty, st), restatement("CAMF_MCS", np.float64, d, empty, st)
    for epoch in range(5):
        l32, l64 = r32.epoch(util.LR), r64.epoch(util.LR)
        assert np.isfinite(l32), epoch
        if epoch < 2:      # before the trajectories part at a clipping decision
            assert abs(l32 - l64) <= 1e-6 * l64
    assert all(np.isfinite(a).all() for a in r32.state.values())
    cv = r32.state["cVector"]
    upbound = np.float32(1.0 / np.sqrt(d.n_dims))
    assert cv.min() >= 0 and cv.max() <= upbound
    assert np.count_nonzero(cv == 0) >= 2 and np.count_nonzero(cv == upbound) >= 2


def test_sequential_sums_add_left_to_right():
    rng = np.random.default_rng(3)
    for dtype in (np.float32, np.float64):
        for n in (1, 2, 63, 64, 65, 130):
            a = (rng.random(n) * rng.choice([1e-4, 1.0, 1e4], n)).astype(dtype)
            s = dtype(0)
            for x in a:
                s = dtype(s + x)
            assert sim_ref._seq_sum(a) == s
