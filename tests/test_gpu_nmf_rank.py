"""Top-N evaluation of NMF on the GPU: the golden predict matrices (tests/golden/reference_nmf.json.gz; NMF has no ranking branch, so
the unbounded product(W, u, H, j) is the score) through eval_rankings on the golden models, the shared score kernel's and the
selection's edges at k in {1, 10, 128} (tests/test_gpu_rankals.check_score_kernel_and_selection_edges with W = P, H = Q^T), and the
refusals: a model wider than the kernel's LDS row, and an evaluation before a model is set."""
import numpy as np
import pytest

from carskit_amd import capi
from tests import nmf_ref as nref, topn_baselines as tb
from tests.test_gpu_rankals import check_rankings, check_score_kernel_and_selection_edges, contextual_split, score_split

pytestmark = pytest.mark.gpu


def instance(k, nu, ni, cells, P, Q):
    h = capi.NMFInstance(k, nu, ni)
    h.set_ratings(np.array([c[0] for c in cells], np.int32), np.array([c[1] for c in cells], np.int32), np.array([c[2] for c in cells]))
    h.set_model(P, np.ascontiguousarray(Q.T))
    return h


@pytest.mark.parametrize("run", nref.golden_runs(), ids=lambda r: r["name"])
def test_eval_rankings_on_golden_models(run):
    h = capi.NMFInstance(run["k"], run["n_users"], run["n_items"])
    h.set_ratings(run["u"], run["i"], run["r"])
    h.set_model(run["iters"][-1]["W"], run["iters"][-1]["H"])   # the golden scores belong to the last iteration's model
    with pytest.raises(capi.CmiError) as e:
        h.last_rank_ms()                                        # no evaluation yet
    assert e.value.code == capi.E_INVALID
    cells = list(zip(run["u"].tolist(), run["i"].tolist(), run["r"].tolist()))
    train, test = contextual_split(cells, 4, tb.SPLIT_SEED)
    for kw in tb.SETTINGS:
        check_rankings(h, run["predict"], train, test, **kw)
    assert h.last_rank_ms() > 0.0
    h.close()


@pytest.mark.parametrize("k,n_cand,num_recs", [(1, 65, 10), (1, 513, 70), (10, 63, 10), (10, 64, 70), (10, 65, 10), (10, 513, 70), (10, 513, 10),
                                               (128, 65, 10), (128, 513, 70)])
def test_score_kernel_and_selection_edges(k, n_cand, num_recs):
    check_score_kernel_and_selection_edges(instance, k, n_cand, num_recs)


def test_refusals():
    train, test, cells = score_split(65)
    rng = np.random.default_rng(3)
    h = capi.NMFInstance(129, 8, 520)                           # trains, but is wider than the score kernel's row of 128
    h.set_ratings(np.array([c[0] for c in cells], np.int32), np.array([c[1] for c in cells], np.int32), np.array([c[2] for c in cells]))
    with pytest.raises(capi.CmiError) as e:
        h.eval_rankings(train, test)
    assert e.value.code == capi.E_INVALID                       # no model yet
    h.set_model(rng.random((8, 129)), rng.random((129, 520)))
    with pytest.raises(capi.CmiError) as e:
        h.eval_rankings(train, test)
    assert e.value.code == capi.E_UNSUPPORTED and "129" in str(e.value) and "128" in str(e.value), str(e.value)
    assert np.isfinite(h.predict([0, 1], [2, 3])).all()         # rating prediction is unaffected
    h.close()
