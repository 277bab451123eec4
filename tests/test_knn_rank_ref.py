"""The ranking-mode restatement (tests/knn_rank_ref.py) against tests/golden/reference_knn_rank.json.gz, which the reference's own
ItemKNN / UserKNN source computed with isRankingPred = true (tests/tools/mint_reference_knn_rank.py), bit for bit; the facts the mint
recorded about the handmade matrix; and the splits the GPU tests evaluate.  No GPU."""
import gzip
import json
import os

import numpy as np
import pytest

from carskit_amd import capi
from tests import knn_rank_ref, knn_ref, nmf_ref, rankals_ref, slopeone_ref, topn_baselines as tb
from tests.test_gpu_rankals import contextual_split
from tests.util import same_bits_exact

RUNS = tb.knn_rank_runs()


def restated(run):
    """(S, means, lists) of a golden run from tests/knn_ref.py"""
    kind, nu, ni = run["kind"], run["n_users"], run["n_items"]
    rows = knn_ref.rows_of(run["u"], run["i"], run["r"], kind, nu, ni)
    S = knn_ref.build_corrs(rows, nu if kind == "item" else ni, run["measure"], run["shrinkage"])
    return S, knn_ref.row_means(rows, run["global_mean"]), knn_ref.lists_of(run["u"], run["i"], run["r"], kind, nu, ni)


def test_golden_file_covers_what_was_asked():
    assert os.path.getsize(os.path.join(tb.GOLDEN, "reference_knn_rank.json.gz")) <= os.path.getsize(os.path.join(tb.GOLDEN, "reference_knn.json.gz"))
    big = [r for r in RUNS if r["matrix"] == "knn_matrix"]
    assert sorted((r["kind"], r["measure"], r["shrinkage"]) for r in big) == [("item", "PCC", -1), ("item", "cos", 30), ("user", "PCC", -1),
                                                                               ("user", "cos", 30)]
    assert all(sorted(r["ranking"]) == [0, 1, 5, 12, 1000] and (r["n_users"], r["n_items"]) == (26, 42) for r in big)
    hand = [r for r in RUNS if r["matrix"] == "hand"]
    assert sorted(r["kind"] for r in hand) == ["item", "user"] and all(r["n_users"] <= 8 and r["n_items"] <= 10 for r in hand)


@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_restatement_equals_the_reference_run(run):
    S, means, lists = restated(run)
    for knn, want in run["ranking"].items():
        for fast in (False, True):
            got = knn_rank_ref.ranking_matrix(run["kind"], S, means, lists, run["n_users"], run["n_items"], knn, run["global_mean"], fast)
            assert same_bits_exact(got, want), (run["name"], knn, fast, np.argwhere(got != want)[:5])


@pytest.mark.parametrize("kind", ["item", "user"])
def test_ranking_mode_differs_from_rating_mode(kind):
    """some score of the PCC run lies elsewhere than the rating-mode golden's, after the bound; cos of positive ratings keeps the same
    neighbours in both modes"""
    rating = json.loads(gzip.open(os.path.join(tb.GOLDEN, "reference_knn.json.gz"), "rb").read())["models"]
    model = "ItemKNN" if kind == "item" else "UserKNN"
    for run in (r for r in RUNS if r["matrix"] == "knn_matrix" and r["kind"] == kind):
        old = next(m for m in rating if (m["model"], m["measure"], m["shrinkage"]) == (model, run["measure"], run["shrinkage"]))
        differs = 0
        for knn, got in run["ranking"].items():
            want = np.array([[float.fromhex(x) for x in row] for row in old["predict"][str(knn)]])
            differs += int(np.count_nonzero(np.clip(got, 1.0, 5.0) != want))
        assert (differs > 0) == (run["measure"] == "PCC"), (run["name"], differs)


@pytest.mark.parametrize("run", [r for r in RUNS if r["matrix"] == "hand"], ids=lambda r: r["name"])
def test_handmade_witnesses(run):
    """(a) a zero similarity between non-empty vectors, (b) a negative one that survives a cut, (c) one that is cut; and a score that
    keeping the zero entry would change"""
    kind, gm = run["kind"], run["global_mean"]
    S, means, lists = restated(run)
    n = len(S)
    assert same_bits_exact(np.array([np.nan_to_num(S[a, b], nan=0.0) for a in range(n) for b in range(a + 1, n)]), run["corrs"])
    w = run["witnesses"]
    a, b = w["zero_pair"]
    rows = knn_ref.rows_of(run["u"], run["i"], run["r"], kind, run["n_users"], run["n_items"])
    assert S[a, b] == 0.0 and rows[a] and rows[b]

    def kept(u, j):
        owner, target = (u, j) if kind == "item" else (j, u)
        return sorted(((e, float(S[target, e])) for e, rate in lists[owner] if knn_rank_ref.keeps(float(S[target, e]), rate)),
                      key=lambda kv: -kv[1])

    u, j, knn = w["negative_survives_cut"]
    assert 0 < knn < len(kept(u, j)) and any(v < 0 for _, v in kept(u, j)[:knn])
    u, j, knn = w["negative_cut"]
    assert 0 < knn < len(kept(u, j)) and any(v < 0 for _, v in kept(u, j)[knn:])
    u, j, knn = w["zero_kept_would_differ"]
    owner, target = (u, j) if kind == "item" else (j, u)
    assert any(S[target, e] == 0.0 and rate > 0 for e, rate in lists[owner])
    Z = np.where(S == 0.0, 5e-324, S)  # the zero entries kept (as the smallest positive weight): another neighbourhood
    assert knn_rank_ref.ranking(kind, Z, means, lists, u, j, knn, gm) != run["ranking"][knn][u, j]


def test_keep_rule():
    nan = float("nan")
    assert [knn_rank_ref.keeps(s, 2.0) for s in (0.5, -0.25, 0.0, -0.0, nan)] == [True, True, False, False, False]
    assert not knn_rank_ref.keeps(0.5, 0.0) and not knn_rank_ref.keeps(-0.5, -1.0)


def test_every_setting_of_the_gpu_evaluations_leaves_a_list():
    groups = [(r["name"], r["n_users"], r["n_items"], r["cells"], list(r["ranking"].values())) for r in RUNS]
    for mod, ref in (("slopeone", slopeone_ref), ("nmf", nmf_ref)):
        for r in ref.golden_runs():
            groups.append((mod + " " + r["name"], r["n_users"], r["n_items"], list(zip(r["u"].tolist(), r["i"].tolist(), r["r"].tolist())),
                           [r["predict"]]))
    for name, nu, ni, cells, scores in groups:
        train, test = contextual_split(cells, 4, tb.SPLIT_SEED)
        for kw in tb.SETTINGS:
            cand, queries = capi.rank_plan(nu, ni, train, test, kw["bin_thold"], kw.get("num_ignore", 0))
            for sc in scores:
                assert len(rankals_ref.top_lists(cand, queries, sc, kw["bin_thold"], kw["num_recs"])) > 0, (name, kw)
