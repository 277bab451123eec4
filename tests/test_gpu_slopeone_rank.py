"""Top-N evaluation of SlopeOne on the GPU: the golden predict matrices (tests/golden/reference_slopeone.json.gz; SlopeOne has no ranking
branch, so the unbounded predict is the score) through eval_rankings, and the score kernel's edges -- rows of 0, 1, 64, 65 entries and
one more than the LDS tile holds, 65 and 513 candidates, lists of 10 and 70, a user with four contexts, batches of 3 queries -- against
the chain of tests/slopeone_ref.py over the deviations the device built."""
import functools

import numpy as np
import pytest

from carskit_amd import capi
from tests import slopeone_ref as sref, topn_baselines as tb
from tests.test_gpu_rankals import check_rankings, contextual_split, score_split
from tests.util import same_bits_exact, with_env

pytestmark = pytest.mark.gpu

SLOPE_RTILE = 1024  # slopeone_kernels.hpp: the entries of a user's row the score kernel stages in LDS
ROW_LENGTHS = (1, 64, 65, SLOPE_RTILE + 1, 130, 30, 40, 0)  # of the query users 0 .. 7 (score_split's)
GM = 3.125


def built(nu, ni, u, i, r):
    h = capi.SlopeOneInstance(nu, ni)
    h.set_ratings(u, i, r)
    h.build()
    return h


@pytest.mark.parametrize("run", sref.golden_runs(), ids=lambda r: r["name"])
def test_eval_rankings_on_golden_models(run):
    h = built(run["n_users"], run["n_items"], run["u"], run["i"], run["r"])
    with pytest.raises(capi.CmiError) as e:
        h.last_rank_ms()                                        # no evaluation yet
    assert e.value.code == capi.E_INVALID
    cells = list(zip(run["u"].tolist(), run["i"].tolist(), run["r"].tolist()))
    train, test = contextual_split(cells, 4, tb.SPLIT_SEED)
    for kw in tb.SETTINGS:
        check_rankings(tb.Scored(h, run["global_mean"]), run["predict"], train, test, **kw)
    assert h.last_rank_ms() > 0.0
    h.close()


@functools.lru_cache(maxsize=None)
def edge_matrix():
    """12 users x 1100 items: user q < 8 has ROW_LENGTHS[q] items (user 7 none: every score is the global mean), the others 100 to 300"""
    rng = np.random.default_rng(20261021)
    nu, ni = 12, 1100
    cells = {}
    for u in range(nu):
        n = ROW_LENGTHS[u] if u < 8 else int(rng.integers(100, 300))
        for j in rng.choice(ni, n, replace=False).tolist():
            cells[(u, j)] = float(rng.integers(1, 6)) / (3.0 if rng.random() < 0.2 else 1.0)
    cl = sorted(cells.items())
    return nu, ni, np.array([k[0] for k, _ in cl], np.int32), np.array([k[1] for k, _ in cl], np.int32), np.array([v for _, v in cl])


@functools.lru_cache(maxsize=None)
def edge_handle():
    return built(*edge_matrix())


@functools.lru_cache(maxsize=None)
def edge_scores():
    """SlopeOne.predict(u, j), unbounded, of the query users 0 .. 7 over the items below 520 (the candidates of score_split), from the
    device's dev / card: slopeone_ref.predict's chain, the valid terms added in ascending item order (np.cumsum is that serial sum)"""
    nu, ni, u, i, r = edge_matrix()
    dev, card = edge_handle().deviation()
    rows = sref.rows_of(u, i, r, nu)
    sc = np.full((nu, ni), np.nan)
    for a in range(8):
        idx = np.array([j for j, _ in rows[a]], np.int64)
        val = np.array([v for _, v in rows[a]])
        for j in range(520):
            c = card[j, idx].astype(np.float64) if len(idx) else np.zeros(0)
            ok = (idx != j) & (c > 0)
            if ok.any():
                sc[a, j] = np.cumsum(((dev[j, idx] + val) * c)[ok])[-1] / np.cumsum(c[ok])[-1]
            else:
                sc[a, j] = GM
    return sc


def test_edge_matrix_has_the_edges():
    nu, ni, u, i, r = edge_matrix()
    rows = sref.rows_of(u, i, r, nu)
    assert [len(rows[q]) for q in range(8)] == list(ROW_LENGTHS)
    sc = edge_scores()
    assert np.all(sc[7, :520] == GM)
    dev, card = edge_handle().deviation()
    tu = np.repeat(np.arange(8, dtype=np.int32), 40)
    tj = np.tile(np.arange(0, 520, 13, dtype=np.int32), 8)
    want = np.array([sref.predict(dev, card, rows, int(a), int(b), GM) for a, b in zip(tu, tj)])  # the scalar chain agrees
    assert same_bits_exact(sc[tu, tj], want)
    assert same_bits_exact(edge_handle().predict(tu, tj, GM), want)


@pytest.mark.parametrize("n_cand,num_recs", [(63, 10), (64, 70), (65, 10), (513, 70), (513, 10)])
def test_score_kernel_and_selection_edges(n_cand, num_recs):
    h = tb.Scored(edge_handle(), GM)
    train, test, _ = score_split(n_cand)
    lists = check_rankings(h, edge_scores(), train, test, bin_thold=-1e9, num_recs=num_recs)
    plan_cand, queries = capi.rank_plan(h.n_users, h.n_items, train, test, -1e9, 0)
    assert len(plan_cand) == n_cand
    ex4 = {c: tuple(e) for u, c, _, e in queries if u == 4}
    assert len(ex4) == 4 and len(set(ex4.values())) == 4           # one group of four queries, four exclusion lists
    seven = [v for key, v in lists.items() if key[0] == 7]
    assert seven and all([i for i, _ in v] == plan_cand[:len(v)] for v in seven)   # every score the global mean: candidate order
    batched = with_env(lambda: h.eval_rankings(train, test, bin_thold=-1e9, num_recs=num_recs, with_lists=True), CMI_RANK_BATCH=3)
    assert batched[1] == lists


def test_evaluating_before_build_is_invalid():
    nu, ni, u, i, r = edge_matrix()
    train, test, _ = score_split(65)
    h = capi.SlopeOneInstance(nu, ni)
    for step in (lambda: None, lambda: h.set_ratings(u, i, r)):
        step()
        with pytest.raises(capi.CmiError) as e:
            h.eval_rankings(train, test, GM)
        assert e.value.code == capi.E_INVALID
    h.close()
