"""The CMI_E_NUMERIC exit of cmi_bpr_iterate, cmi_ranksgd_iterate and cmi_nmf_iterate: a start that drives the loss to +Inf or NaN in
one iteration.  The call fails with the entry point's name in the message, but the iteration has run: the model equals the
restatement's bit for bit where it is a number and is NaN where the restatement's is, the random stream has advanced as the
restatement's, the handle still works (a finite model and one more iteration give a fresh handle's bits), and the top-N evaluation of
the diverged model gives the lists the reference's rule selects from the restatement's scores of it (tests/test_gpu_rank_nonfinite.py
holds that rule on planted models; here the non-finite scores come out of an iteration).
(The loss check of the CAMF epoch, cmi_train, is reached by tests/test_gpu_parity.py::test_nan_loss_is_an_error; LRMF and SLIM have
their own such tests.)"""
import math

import numpy as np
import pytest

from carskit_amd import capi
from oracle import rank_oracle
from tests import bpr_ref as bref
from tests import nmf_ref as nref
from tests import rankals_ref as rref
from tests import ranksgd_ref as rr
from tests import test_gpu_bpr as tbpr
from tests import test_gpu_nmf as tnmf
from tests import test_gpu_ranksgd as tsgd
from tests.test_bpr_capi_cpu import cols
from tests.test_gpu_rankals import contextual_split, edge_matrix
from tests.util import same_bits, same_bits_exact

pytestmark = pytest.mark.gpu

K = 4


def rankings_follow_the_rule(h, P, Q, cells, thold=-1.0, seed=11):
    """eval_rankings of the handle's model against the oracle over the restatement's scores of (P, Q); returns
    (lists, non-finite scores among them)"""
    with np.errstate(invalid="ignore", over="ignore"):
        scores = rref.scores(P, Q)
    train, test = contextual_split(cells, 4, seed)
    tup = lambda d: list(zip(*[np.asarray(a).tolist() for a in d]))  # noqa: E731
    out = None
    for num_recs in (10, 70):
        ref, want = rank_oracle.eval_rankings(lambda u, j, c: float(scores[u, j]), tup(train), tup(test), bin_thold=thold, num_recs=num_recs)
        res, lists = h.eval_rankings(train, test, bin_thold=thold, num_recs=num_recs, with_lists=True)
        assert set(lists) == set(want)
        for key, ref_l in want.items():
            assert [i for i, _ in lists[key]] == [i for i, _ in ref_l], key
            assert same_bits_exact([s for _, s in lists[key]], [s for _, s in ref_l]), key
        for m in rank_oracle.MEASURES:
            assert (math.isnan(res[m]) and math.isnan(ref[m])) or abs(res[m] - ref[m]) <= 1e-12, (m, res[m], ref[m])
        out = out or (want, res["n_queries"])
    return scores, out[0], out[1]


def bpr_start(kind):
    nu, ni, cells = edge_matrix()
    rated = np.zeros(ni, bool)
    rated[[j for _, j, v in cells if v != 0.0]] = True
    if kind == "inf_loss":
        # x_uij = <P[u], Q[i] - Q[j]> = 4 * 20 * (-10 - 10) = -1600 for a rated i and an unrated j: g = 1 / (1 + exp(1600)) = 0, -log(0) = +Inf,
        # while every update stays finite
        P0 = np.full((nu, K), 20.0)
        Q0 = np.where(rated[:, None], -10.0, 10.0) * np.ones((ni, K))
    else:
        # <P[u], Q[i]> and <P[u], Q[j]> both overflow to +Inf for every second user: x_uij = Inf - Inf = NaN, and the sample's three rows with it
        P0 = np.where((np.arange(nu) % 2 == 0)[:, None], 1e200, 1.0) * np.ones((nu, K))
        Q0 = np.full((ni, K), 1e200)
    return nu, ni, cells, P0, Q0


@pytest.mark.parametrize("kind", ["inf_loss", "nan_factors"])
def test_bpr_iteration_that_diverges(kind):
    nu, ni, cells, P0, Q0 = bpr_start(kind)
    st = bref.random_state(20270111)
    u, i, j, after = capi.bpr_sample_host(nu, ni, *cols(cells), st, nu * 100)
    P, Q = P0.copy(), Q0.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        loss, _ = bref.epoch_by_levels(P, Q, list(zip(u.tolist(), i.tolist(), j.tolist())), tbpr.LR, tbpr.REG_U, tbpr.REG_I)
    if kind == "inf_loss":
        assert loss == np.inf and np.isfinite(P).all() and np.isfinite(Q).all()
    else:
        assert math.isnan(loss) and np.isnan(P).any() and np.isnan(Q).any() and np.isfinite(P).any()
    h = tbpr.instance(K, nu, ni, cells, P0, Q0, state=st)
    with pytest.raises(capi.CmiError) as e:
        h.iterate(tbpr.LR, tbpr.REG_U, tbpr.REG_I)
    assert e.value.code == capi.E_NUMERIC and "cmi_bpr_iterate" in str(e.value), str(e.value)
    gP, gQ = h.model()
    assert same_bits(gP, P) and same_bits(gQ, Q), (np.argwhere(gP != P)[:5], np.argwhere(gQ != Q)[:5])
    assert h.random_state() == after
    # (inf_loss: the candidates are the rated items, whose scores are near -800: a threshold below them)
    scores, lists, nq = rankings_follow_the_rule(h, P, Q, cells, -1.0 if kind == "nan_factors" else -1e9)
    if kind == "nan_factors":
        assert np.isnan(scores).any() and nq > len(lists)             # queries whose every score is NaN have no list
    else:
        assert len(lists) == nq > 20
    # the handle still works: a finite model and one more iteration, as on a handle that has seen nothing
    rng = np.random.default_rng(7)
    P1, Q1 = rng.random((nu, K)), rng.random((ni, K))
    fresh = tbpr.instance(K, nu, ni, cells, P1, Q1, state=st)
    h.set_model(P1, Q1)
    h.set_random_state(st)
    assert same_bits_exact([h.iterate(tbpr.LR, tbpr.REG_U, tbpr.REG_I)], [fresh.iterate(tbpr.LR, tbpr.REG_U, tbpr.REG_I)])
    for a, b in zip(h.model(), fresh.model()):
        assert same_bits_exact(a, b) and np.isfinite(a).all()
    assert h.random_state() == fresh.random_state()
    h.close()
    fresh.close()


def test_ranksgd_iteration_that_diverges():
    """every thirtieth user's row is 1e200 against item rows of 1e200: pui and puj both overflow to +Inf and e = Inf - Inf = NaN.  The
    loss is NaN, and so is every row a diverged sample touched and every row a later sample reached from one; the few that stay numbers
    leave a few one-item lists"""
    nu, ni, cells = tsgd.epoch_matrix()
    (samples, after), _ = tsgd.epoch_samples()
    P0 = np.where((np.arange(nu) % 30 == 0)[:, None], 1e200, 0.125) * np.ones((nu, K))
    Q0 = np.full((ni, K), 1e200)
    P, Q = P0.copy(), Q0.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        loss, _ = rr.epoch_by_levels(P, Q, samples, tsgd.LR)
    assert math.isnan(loss) and np.isnan(P).any() and np.isnan(Q).any() and np.isfinite(P).any() and np.isfinite(Q).any()
    h = tsgd.instance(K, nu, ni, cells, P0, Q0, state=tsgd.EPOCH_STATE)
    with pytest.raises(capi.CmiError) as e:
        h.iterate(tsgd.LR)
    assert e.value.code == capi.E_NUMERIC and "cmi_ranksgd_iterate" in str(e.value), str(e.value)
    gP, gQ = h.model()
    assert same_bits(gP, P) and same_bits(gQ, Q), (np.argwhere(gP != P)[:5], np.argwhere(gQ != Q)[:5])
    assert h.random_state() == after
    scores, lists, nq = rankings_follow_the_rule(h, P, Q, [c for c in cells if c[2] != 0.0])
    assert np.isnan(scores).any() and np.isfinite(scores).any() and 0 < len(lists) < nq
    rng = np.random.default_rng(8)
    P1, Q1 = 0.1 * rng.standard_normal((nu, K)), 0.1 * rng.standard_normal((ni, K))
    fresh = tsgd.instance(K, nu, ni, cells, P1, Q1, state=tsgd.EPOCH_STATE)
    h.set_model(P1, Q1)
    h.set_random_state(tsgd.EPOCH_STATE)
    assert same_bits_exact([h.iterate(tsgd.LR)], [fresh.iterate(tsgd.LR)])
    for a, b in zip(h.model(), fresh.model()):
        assert same_bits_exact(a, b) and np.isfinite(a).all()
    assert h.random_state() == fresh.random_state()
    h.close()
    fresh.close()


def test_nmf_iteration_from_an_infinite_weight():
    """W0[5][0] = +Inf: user 5's estimates are +Inf, its row's update divides by them, and the loss is no number"""
    nu, ni, u, i, r, rows, cols_ = tnmf.edge_matrix()
    rng = np.random.default_rng(9)
    W0, H0 = rng.random((nu, K)), rng.random((K, ni))
    W0[5, 0] = np.inf
    assert len(rows[5][0]) > 0
    W, Ht = W0.copy(), np.ascontiguousarray(H0.T)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        loss = nref.iterate(W, Ht, rows, cols_)
    assert not math.isfinite(loss)
    h = capi.NMFInstance(K, nu, ni)
    h.set_ratings(u, i, r)
    h.set_model(W0, H0)
    with pytest.raises(capi.CmiError) as e:
        h.iterate()
    assert e.value.code == capi.E_NUMERIC and "cmi_nmf_iterate" in str(e.value), str(e.value)
    gW, gH = h.model()
    assert same_bits(gW, W) and same_bits(gH, Ht.T), (np.argwhere(gW != W)[:5], np.argwhere(gH != Ht.T)[:5])
    W1, H1 = rng.random((nu, K)), rng.random((K, ni))
    fresh = capi.NMFInstance(K, nu, ni)
    fresh.set_ratings(u, i, r)
    fresh.set_model(W1, H1)
    h.set_model(W1, H1)
    assert same_bits_exact([h.iterate()], [fresh.iterate()])
    for a, b in zip(h.model(), fresh.model()):
        assert same_bits_exact(a, b) and np.isfinite(a).all()
    h.close()
    fresh.close()
