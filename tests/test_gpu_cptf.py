"""CPTF on the GPU: the golden runs of the reference through the C ABI, the one-wave epoch against tests/cptf_ref.py in both summation
forms and both context-row forms (factor counts at the lane borders, 2 to 10 dimensions, entry counts at the read-ahead's borders, rows
that repeat at every short distance), the rating <= 0 skip, the unguarded division, prediction and the top-N evaluation."""
import functools
import math

import numpy as np
import pytest

from carskit_amd import capi
from oracle import rank_oracle
from tests import cptf_ref as cref
from tests.test_cptf_ref import RUNS
from tests.test_gpu_rankals import contextual_split
from tests.util import same_bits, same_bits_exact

pytestmark = pytest.mark.gpu

LRATE, REG = 0.013, 0.027                    # distinct, loud
CTX_FORMS = [("lds", 0), ("global", capi.CPTF_FLAG_GLOBAL_CTX)]
SUM_FORMS = [("strict", capi.CPTF_FLAG_STRICT, cref.epoch_strict), ("tree", 0, cref.epoch_tree)]
ITERS = 3


@pytest.mark.parametrize("cname,cflag", CTX_FORMS, ids=[c[0] for c in CTX_FORMS])
@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_golden_runs_match_the_reference_run(run, cname, cflag):
    """the reference's own run (CPTF.java executed from source) through the C ABI in the strict form: M, the loss and predict(keys),
    NaN where the reference has NaN, else bit for bit"""
    h = capi.CPTFInstance(run["k"], run["dims"], flags=capi.CPTF_FLAG_STRICT | cflag)
    h.set_entries(run["keys"], run["r"])
    h.set_model(run["M0"])
    for n, it in enumerate(run["iters"]):
        if math.isfinite(it["loss"]):
            loss = h.iterate(run["lrate"], run["reg"])
        else:                                                        # where the reference's isConverged ends the program
            with pytest.raises(capi.CmiError) as e:
                h.iterate(run["lrate"], run["reg"])
            assert e.value.code == capi.E_NUMERIC
            loss = e.value.loss
        assert same_bits([loss], [it["loss"]]), (n, loss, it["loss"])
        for d, m in enumerate(h.model()):
            assert same_bits(m, it["M"][d]), (n, d, np.argwhere(m != it["M"][d])[:5])
    assert h.ctx_in_lds() == (cname == "lds")
    assert same_bits(h.predict(run["predict_keys"]), run["predict"])
    assert same_bits(h.predict(run["predict_keys"], True, run["min_rate"], run["max_rate"]), run["predict_bounded"])
    ms = h.last_iter_ms()
    assert len(ms) == 3 and ms[0] > 0.0 and ms[1] > 0.0 and ms[2] == 0.0
    h.close()


def test_tree_form_rating_measures_within_the_parity_bound_of_the_reference_pinned_values():
    """evalRatings' RMSE and MAE of the non-strict form's model against those of the reference's own model (the golden M after three
    iterations, not the strict kernel's), within the project's parity bound of 1e-5; the golden tensors' entries serve as test entries"""
    for run in RUNS:
        if len(run["iters"]) < ITERS:
            continue
        h = capi.CPTFInstance(run["k"], run["dims"])
        h.set_entries(run["keys"], run["r"])
        h.set_model(run["M0"])
        for _ in range(ITERS):
            h.iterate(run["lrate"], run["reg"])
        keys, rates = run["keys"].tolist(), run["r"].tolist()
        pred = h.predict(run["keys"], True, run["min_rate"], run["max_rate"])
        h.close()
        want = cref.eval_ratings(run["iters"][-1]["M"], keys, rates, run["min_rate"], run["max_rate"])
        err = np.abs(np.array(rates) - pred)
        mae, rmse = float(err.sum() / len(err)), math.sqrt(float((err * err).sum() / len(err)))
        print(run["name"], "MAE", mae, want["MAE"], "RMSE", rmse, want["RMSE"])
        assert abs(mae - want["MAE"]) <= 1e-5 and abs(rmse - want["RMSE"]) <= 1e-5, run["name"]


def draw_model(rng, dims, k, total=None, spread=0.1):
    """CPTF.initModel's draw, elements around 1; total: scaled so that a prediction lies around `total`"""
    scale = 1.0 if total is None else (total / k) ** (1.0 / len(dims))
    return [scale * (1.0 + spread * rng.standard_normal((n, k))) for n in dims]


def draw_entries(rng, dims, n):
    """n entries over small dimensions, so every row repeats at every short distance; the first entries walk the distances on purpose:
    the same user and item twice running (both sides stale at once), the same user at distance 2, the same item at distance 3"""
    keys = np.stack([rng.integers(0, d, n) for d in dims], axis=1).astype(np.int32)
    lead = [(0, 0), (0, 0), (1, 0), (0, 1), (1, 1), (2, 1), (0, 2)]
    for t, (u, j) in enumerate(lead[:n]):
        keys[t, 0], keys[t, 1] = u % dims[0], j % dims[1]
    if n > 2 and len(dims) > 2:
        keys[1, 2:] = keys[0, 2:]                                    # and the same context rows twice running
    r = rng.integers(1, 6, n).astype(np.float64)
    return keys, r


def dims_for(n_dims):
    return [3, 4] + [2, 3, 2, 3, 2, 3, 2, 3][:n_dims - 2]


def run_forms(dims, k, keys, r, seed, sum_forms=SUM_FORMS, ctx_forms=CTX_FORMS, iters=ITERS, M0=None):
    rng = np.random.default_rng(seed)
    if M0 is None:
        M0 = draw_model(rng, dims, k, total=3.0)                     # inside the ratings' range: the run stays finite at every k
    for sname, sflag, ref_epoch in sum_forms:
        want_M, want_loss = [m.copy() for m in M0], []
        for _ in range(iters):
            want_loss.append(ref_epoch(want_M, keys, r, LRATE, REG))
        assert np.all(np.isfinite(want_loss)), (sname, want_loss)
        for cname, cflag in (ctx_forms if len(dims) > 2 else ctx_forms[1:]):
            h = capi.CPTFInstance(k, dims, flags=sflag | cflag)
            h.set_entries(keys, r)
            h.set_model(M0)
            losses = [h.iterate(LRATE, REG) for _ in range(iters)]           # several iterations on one handle
            assert h.ctx_in_lds() == (cname == "lds"), (sname, cname)
            got = h.model()
            h.close()
            assert same_bits_exact(losses, want_loss), (sname, cname, losses, want_loss)
            for d in range(len(dims)):
                assert same_bits_exact(got[d], want_M[d]), (sname, cname, d, np.argwhere(got[d] != want_M[d])[:5])


@pytest.mark.parametrize("n_dims", [2, 3, 5, 10])
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 128])
def test_epoch_matches_the_restatement(k, n_dims):
    dims = dims_for(n_dims)
    keys, r = draw_entries(np.random.default_rng(100 * k + n_dims), dims, 129)
    run_forms(dims, k, keys, r, seed=7 * k + n_dims)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65])
@pytest.mark.parametrize("k,n_dims", [(2, 3), (65, 5)])
def test_entry_counts_at_the_read_ahead_borders(k, n_dims, n):
    """the rows of entry t + 1 and the offsets of entry t + 2 are requested ahead: one, two and three entries, and longer streams"""
    dims = dims_for(n_dims)
    keys, r = draw_entries(np.random.default_rng(n), dims, n)
    run_forms(dims, k, keys, r, seed=n)


def test_one_row_per_dimension_every_entry_stale():
    """every dimension has one row: each entry's requested rows are all stale"""
    dims = [1, 1, 1, 1]
    keys, r = np.zeros((17, 4), np.int32), np.arange(1, 18) % 5 + 1.0
    run_forms(dims, 10, keys, r, seed=3)


def test_entries_with_a_rate_of_zero_or_less_take_no_part():
    dims = dims_for(4)
    keys, r = draw_entries(np.random.default_rng(5), dims, 40)
    r[[0, 7, 8, 39]] = [0.0, -1.0, 0.0, -0.5]
    run_forms(dims, 10, keys, r, seed=5)
    h = capi.CPTFInstance(3, dims)
    h.set_entries(keys[:1], [0.0])                                   # nothing to visit: the loss is 0
    h.set_model(draw_model(np.random.default_rng(1), dims, 3))
    assert h.iterate(LRATE, REG) == 0.0
    h.close()


def test_context_rows_past_the_lds_budget_travel_through_memory():
    """3 context dimensions of 30 conditions at k = 128: 92160 bytes of context rows, past the 64 KiB kept in LDS"""
    dims = [3, 4, 30, 30, 30]
    keys, r = draw_entries(np.random.default_rng(9), dims, 64)
    run_forms(dims, 128, keys, r, seed=9, sum_forms=SUM_FORMS[1:], ctx_forms=[("global", 0)], iters=2)


@pytest.mark.parametrize("cname,cflag", CTX_FORMS, ids=[c[0] for c in CTX_FORMS])
def test_a_zero_element_gives_e_numeric_and_the_restatements_nan_pattern(cname, cflag):
    """CPTF.java:103 divides by the element: 0 / 0 leaves a NaN in the row, and the row's next visit a NaN loss"""
    dims = dims_for(3)
    keys, r = draw_entries(np.random.default_rng(11), dims, 30)
    M0 = draw_model(np.random.default_rng(12), dims, 5)
    M0[1][int(keys[0, 1]), 2] = 0.0                                  # item 0 is trained by the entries 0, 1 and 2
    want = [m.copy() for m in M0]
    want_loss = cref.epoch_strict(want, keys, r, LRATE, REG)
    assert not math.isfinite(want_loss)                              # the restatement alone says so
    h = capi.CPTFInstance(5, dims, flags=capi.CPTF_FLAG_STRICT | cflag)
    h.set_entries(keys, r)
    h.set_model(M0)
    with pytest.raises(capi.CmiError) as e:
        h.iterate(LRATE, REG)
    assert e.value.code == capi.E_NUMERIC and same_bits([e.value.loss], [want_loss])
    got = h.model()
    h.close()
    assert any(np.isnan(m).any() for m in want)
    for d in range(len(dims)):
        assert same_bits(got[d], want[d]), d                         # NaN where the restatement has NaN, else bit for bit


@pytest.mark.parametrize("n_dims", [2, 3, 5, 10])
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 128])
def test_predict_matches_the_restatement(k, n_dims):
    dims = dims_for(n_dims)
    rng = np.random.default_rng(k + n_dims)
    M = draw_model(rng, dims, k)
    keys = np.stack([rng.integers(0, d, 300) for d in dims], axis=1).astype(np.int32)       # more than one block
    free = [cref.predict_keys(M, ks) for ks in keys.tolist()]
    lo, hi = np.percentile(free, [30, 70]).tolist()                  # of the restatement's sums: some below, some inside, some above
    h = capi.CPTFInstance(k, dims)
    h.set_model(M)
    assert same_bits_exact(h.predict(keys), free)
    assert same_bits_exact(h.predict(keys, True, lo, hi), [cref.clamp(p, lo, hi) for p in free])
    assert len({cref.clamp(p, lo, hi) == p for p in free}) == 2      # both clamped and unclamped values occur
    h.close()


# ---- top-N ---------------------------------------------------------------------------------------------------------------------------
def rank_case(n_cand, seed, n_users=6, n_ctx=4, ids=None):
    """train tuples that make the items 0 .. n_cand - 1 the candidates, and test tuples of some users in some contexts: a 2-D matrix
    in which every item has a cell, spread over contexts and split by the helper the other top-N tests use; ids: the item id that
    stands for item j in the tuples (a catalogue larger than the candidate set)"""
    rng = np.random.default_rng(seed)
    cells = {(int(rng.integers(0, n_users)), j): float(rng.integers(1, 6)) for j in range(n_cand)}
    for u in range(n_users):
        for j in rng.integers(0, n_cand, 4).tolist():
            cells.setdefault((u, j), float(rng.integers(1, 6)))
    tr, te = contextual_split([(u, j, v) for (u, j), v in sorted(cells.items())], n_ctx, seed, test_share=0.4)
    tup = lambda d: list(zip(*[np.asarray(a).tolist() for a in d]))  # noqa: E731
    tr, te = tup(tr), tup(te)
    have = {j for _, j, _, _ in tr}
    tr += [(0, j, 0, 3.0) for j in range(n_cand) if j not in have]                   # (an item whose every tuple went to the test side)
    if ids is not None:
        tr, te = ([(u, int(ids[j]), c, v) for u, j, c, v in d] for d in (tr, te))
    return sorted(tr), [t for t in te if (t[0], t[1], t[2]) not in {(a, b, c) for a, b, c, _ in tr}]


def cols(tuples):
    return (np.array([t[0] for t in tuples], np.int32), np.array([t[1] for t in tuples], np.int32), np.array([t[2] for t in tuples], np.int32),
            np.array([t[3] for t in tuples]))


def check_rankings(M, dims, k, ctx_keys, lo, hi, tr, te, h=None, got=None, **kw):
    """the lists entry for entry and score for score, the measures within the tolerance the other fp64 top-N tests use, against the
    ranking restatement fed with cptf_ref's scores; h: a handle that holds M, ctx_keys and the range already, and stays open; got: a
    list that takes the device's (measures, lists)"""
    own = h is None
    if own:
        h = capi.CPTFInstance(k, dims)
        h.set_model(M)
        h.set_context_keys(ctx_keys)
        h.set_rating_range(lo, hi)
    res, lists = h.eval_rankings(cols(tr), cols(te), with_lists=True, **kw)
    assert h.last_iter_ms()[2] > 0.0
    if own:
        h.close()
    if got is not None:
        got.append((res, lists))
    score = functools.lru_cache(maxsize=None)(lambda u, c: cref.score_items(M, u, ctx_keys[c], lo, hi))
    ref, ref_lists = rank_oracle.eval_rankings(lambda u, j, c: score(u, c)[j], tr, te, **kw)
    assert len(ref_lists) > 0 and set(lists) == set(ref_lists)
    for key, want in ref_lists.items():
        assert [i for i, _ in lists[key]] == [i for i, _ in want], key
        assert same_bits_exact([s for _, s in lists[key]], [s for _, s in want]), key
    for m in rank_oracle.MEASURES:
        a, b = res[m], ref[m]
        assert (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 1e-12, (m, a, b)
    return ref_lists


@pytest.mark.parametrize("n_cand", [1, 63, 64, 65, 257])
def test_eval_rankings_at_the_candidate_counts(n_cand):
    """a mixed model (scores below, inside and above the rating range), ranking keys that are not the training keys' table, lists
    shorter and longer than the candidate count"""
    dims, k = [6, n_cand, 3, 2], 10
    rng = np.random.default_rng(n_cand)
    M = [0.85 + 0.12 * rng.standard_normal((n, k)) for n in dims]
    ctx_keys = [[2, 1], [0, 0], [1, 1], [2, 0]]                      # getKeys' table: by context id, not the keys a tensor entry carries
    tr, te = rank_case(n_cand, n_cand)
    for kw in (dict(num_recs=10), dict(num_recs=5, strategy="uc", bin_thold=1.5), dict(num_recs=300, num_ignore=0 if n_cand < 4 else 2)):
        lists = check_rankings(M, dims, k, ctx_keys, 1.0, 5.0, tr, te, **kw)
    scores = [s for lst in lists.values() for _, s in lst]
    if n_cand > 1:
        assert min(scores) < 5.0 and max(scores) == 5.0              # clamped and unclamped scores in one list


def test_eval_rankings_all_scores_clamp_to_max_rate():
    """every score is maxRate: the lists are the ties in the order the reference's stable sort leaves them"""
    dims, k = [6, 65, 2], 10
    M = draw_model(np.random.default_rng(2), dims, k)                # sums around 10
    tr, te = rank_case(65, 2, n_ctx=3)
    lists = check_rankings(M, dims, k, [[1], [0], [1]], 1.0, 5.0, tr, te, num_recs=10)
    assert {s for lst in lists.values() for _, s in lst} == {5.0}


def test_eval_rankings_drops_nan_scores():
    dims, k = [6, 65, 2], 3
    rng = np.random.default_rng(4)
    M = [0.9 + 0.2 * rng.standard_normal((n, k)) for n in dims]
    M[1][5, 1] = M[1][40, 0] = float("nan")
    tr, te = rank_case(65, 4, n_ctx=3)
    lists = check_rankings(M, dims, k, [[0], [1], [0]], 1.0, 5.0, tr, te, num_recs=70)
    assert all(i not in (5, 40) for lst in lists.values() for i, _ in lst)


def test_eval_rankings_without_context_dimensions():
    dims, k = [6, 64], 4
    rng = np.random.default_rng(6)
    M = [0.9 + 0.2 * rng.standard_normal((n, k)) for n in dims]
    tr, te = rank_case(64, 6, n_ctx=3)
    check_rankings(M, dims, k, [[], [], []], 1.0, 5.0, tr, te, num_recs=10)


def test_refusals():
    h = capi.CPTFInstance(4, [3, 4, 2])
    with pytest.raises(capi.CmiError) as e:
        h.iterate(0.1, 0.1)
    assert e.value.code == capi.E_INVALID and "no entries" in str(e.value)
    for bad in ([[3, 0, 0]], [[0, 4, 0]], [[0, 0, 2]], [[0, -1, 0]]):
        with pytest.raises(capi.CmiError) as e:
            h.set_entries(bad, [1.0])
        assert e.value.code == capi.E_INVALID and "out of range" in str(e.value)
    h.set_entries([[0, 0, 0]], [1.0])
    with pytest.raises(capi.CmiError) as e:
        h.iterate(0.1, 0.1)
    assert e.value.code == capi.E_INVALID and "no model" in str(e.value)
    s = capi.CPTFInstance(128, [2] * 10, flags=capi.CPTF_FLAG_STRICT)    # the strict form keeps a slot per loss term: 2^27 at the most
    n = (1 << 27) // (1 + 128 * 10) + 1
    with pytest.raises(capi.CmiError) as e:
        s.set_entries(np.zeros((n, 10), np.int32), np.ones(n))
    assert e.value.code == capi.E_UNSUPPORTED and "loss slots" in str(e.value)
    s.set_entries(np.zeros((2, 10), np.int32), np.ones(2))
    s.close()
    with pytest.raises(capi.CmiError) as e:
        h.last_iter_ms()
    assert e.value.code == capi.E_INVALID
    h.set_model([np.ones((3, 4)), np.ones((4, 4)), np.ones((2, 4))])
    with pytest.raises(capi.CmiError) as e:
        h.predict([[0, 0, 2]])
    assert e.value.code == capi.E_INVALID and "out of range" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        h.set_context_keys([[2]])
    assert e.value.code == capi.E_INVALID and "out of range" in str(e.value)
    tr, te = cols([(0, 0, 0, 1.0)]), cols([(0, 1, 0, 1.0)])
    with pytest.raises(capi.CmiError) as e:
        h.eval_rankings(tr, te)
    assert e.value.code == capi.E_INVALID and "set_rating_range" in str(e.value)
    h.set_rating_range(1.0, 5.0)
    with pytest.raises(capi.CmiError) as e:
        h.eval_rankings(tr, te)
    assert e.value.code == capi.E_INVALID and "set_context_keys" in str(e.value)
    h.set_context_keys([[1]])
    with pytest.raises(capi.CmiError) as e:
        h.eval_rankings(tr, cols([(0, 1, 1, 1.0)]))                  # a context id without keys
    assert e.value.code == capi.E_INVALID and "context id" in str(e.value)
    h.close()


# ---- the driver ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def depaul_reference(tmp, form, iters=3, k=10):
    """tests/cptf_ref.py over the DePaul file, cv -k 2 --rand-seed 1: per fold the tensors, M after `iters` iterations with the bold
    driver from the Randoms.seed(1) draw, and the fold's tuples"""
    from carskit_amd import dao
    from oracle import oracle_np
    from tests.hostmirror import splitter
    d0 = dao.DataDAO(tmp)
    d = d0.rating_data()
    cells = list(zip(d0.ui.tolist(), d0.ctx.tolist(), d0.r.tolist()))
    ctx_conds = [d0.ctx_conds[d0.ctx_ptr[c]:d0.ctx_ptr[c + 1]].tolist() for c in range(len(d0.ctx_ptr) - 1)]
    labels, nf = splitter.split_folds(d.n, 2, 1)
    lr0, reg = float(np.float32(2e-2)), float(np.float32(1e-4))
    folds = []
    for f in range(1, nf + 1):
        tr, te = splitter.kth_fold(d, labels, f)
        dims, keys, vals, lists = cref.tensor_build(cells, d0.ui_user, d0.ui_item, ctx_conds, d0.cond_dim.tolist(), form)
        trk, trv, tek, tev = cref.fold_split_fast(len(dims), keys, vals, d0.ui_user, d0.ui_item, [cells[t] for t in np.flatnonzero(labels == f)])
        rnd = oracle_np.JavaRandom(1)
        M = [np.array([[1.0 + 0.1 * rnd.next_gaussian() for _ in range(k)] for _ in range(n)]) for n in dims]
        lrate, last = lr0, 0.0
        for it in range(1, iters + 1):
            loss = cref.epoch_strict(M, trk, trv, lrate, reg)
            assert abs(loss) >= 1e-5
            if it > 1:
                lrate = lrate * 1.05 if abs(last) > abs(loss) else lrate * 0.5
            last = loss
        folds.append({"M": M, "test_keys": tek, "test_vals": tev, "ctx_keys": cref.get_keys_table(ctx_conds, lists), "train": tr, "test": te})
    return folds, (d.min_rate, d.max_rate)


def run_driver(tmp_path, extra_conf, ranking):
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shutil.copyfile(os.path.join(root, "tests", "golden", "depaul_ratings_compact.csv"), tmp_path / "ratings.txt")
    conf = open(os.path.join(root, "tests", "golden", "depaul_setting.conf")).read().replace("PLACEHOLDER_SET_BY_TEST", str(tmp_path / "ratings.txt"))
    assert "num.max.iter=100" in conf and "num.factors=10" in conf and "cv -k 5 -p off --rand-seed 1" in conf and "-threshold -1" in conf
    assert "learn.rate=2e-2 -max -1 -bold-driver" in conf and "reg.lambda=0.0001 -c 0.001" in conf and "item.ranking=off -topN 10" in conf
    conf = conf.replace("recommender=biasedmf", "recommender=cptf").replace("num.max.iter=100", "num.max.iter=3").replace("cv -k 5", "cv -k 2")
    if ranking:
        conf = conf.replace("item.ranking=off", "item.ranking=on").replace("-threshold -1", "-threshold 0")
    (tmp_path / "cptf.conf").write_text(conf + "\n" + extra_conf + "\n")
    p = subprocess.run([os.path.join(root, "carskit_amd", "bin", "carskit-mi355x"), "-c", str(tmp_path / "cptf.conf"), "--precise"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return p.stdout


@pytest.mark.parametrize("form,extra", [(cref.KEYS_SIZE, ""), (cref.KEYS_INDEXOF, "CPTF=-keys indexof")], ids=["reference", "indexof"])
def test_driver_parity_depaul_rating_and_ranking(tmp_path, form, extra):
    """recommender=cptf from a setting.conf, cv -k 2 --rand-seed 1, three iterations with the bold driver, in rating and in ranking
    mode and in both key forms: the printed measures equal those of tests/cptf_ref.py run on the same folds from the same draw"""
    import re

    from carskit_amd import dao
    out = run_driver(tmp_path, extra, ranking=False)
    m = re.search(r"PRECISE CPTF folds=2 MAE=(\S+) RMSE=(\S+)", out)
    assert m and "Final Results by CPTF, MAE: " in out, out[-500:]
    dao.transform(str(tmp_path / "ratings.txt"), str(tmp_path / "train.csv"))
    folds, (lo, hi) = depaul_reference(str(tmp_path / "train.csv"), form)
    want = [cref.eval_ratings(f["M"], f["test_keys"], f["test_vals"], lo, hi) for f in folds]
    for g, name in zip(m.groups(), ("MAE", "RMSE")):
        w = sum(x[name] / len(want) for x in want)
        print(form, name, g, w)
        assert abs(float(g) - w) <= 1e-12, (name, g, w)
    out = run_driver(tmp_path, extra, ranking=True)
    m = re.search(r"PRECISE CPTF folds=2 Pre10=(\S+) Rec10=(\S+) AUC10=(\S+) MAP10=(\S+) NDCG10=(\S+) MRR10=(\S+)", out)
    assert m and "Final Results by CPTF, Pre5: " in out, out[-500:]
    names, want = ("Pre10", "Rec10", "AUC10", "MAP10", "NDCG10", "MRR10"), {}
    tup = lambda d: list(zip(d.u.tolist(), d.j.tolist(), d.ctx.tolist(), d.r.tolist()))  # noqa: E731
    for f in folds:
        score = functools.lru_cache(maxsize=None)(lambda u, c, f=f: cref.score_items(f["M"], u, f["ctx_keys"][c], lo, hi))
        res, _ = rank_oracle.eval_rankings(lambda u, j, c: score(u, c)[j], tup(f["train"]), tup(f["test"]), bin_thold=0.0, num_recs=10)
        for name in names:
            want[name] = want.get(name, 0.0) + res[name] / len(folds)
    for g, name in zip(m.groups(), names):
        print(form, name, g, want[name])
        assert abs(float(g) - want[name]) <= 1e-12, (name, g, want[name])
