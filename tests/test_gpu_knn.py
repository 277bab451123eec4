"""ItemKNN / UserKNN on the GPU against the CPU restatement (tests/knn_ref.py), bit for bit: similarity matrices for every measure x
shrinkage in {-1, 30} x kind on DePaul, one Frappe fold, a synthetic shape whose contracted dimension spans several LDS tiles, one
that adds several 256-partner chunks per anchor, and hand-made edge cases; predictions for knn in {0, 1, 20, more than any candidate count}; two handles built from two host threads;
argument checks; and the driver's MAE / RMSE on DePaul (cv -k 5) against the restatement averaged over the same folds."""
import json
import math
import os
import re
import shutil
import subprocess
import threading

import numpy as np
import pytest

from carskit_amd import capi, dao
from tests import knn_ref
from tests.frappe import write_ratings
from tests.util import global_mean, same_bits, synth_chunks_by_tiles, to2d

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carskit_amd", "bin", "carskit-mi355x")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def read(tmp_path, src):
    dao.transform(src, str(tmp_path / "train.csv"))
    return dao.DataDAO(str(tmp_path / "train.csv")).rating_data()


def depaul(tmp_path):
    shutil.copyfile(os.path.join(GOLDEN, "depaul_ratings_compact.csv"), tmp_path / "ratings.txt")
    return read(tmp_path, str(tmp_path / "ratings.txt"))


def folds(n, k=5, seed=1):
    out = subprocess.run([EXE, "--print-folds", str(n), str(k), str(seed)], capture_output=True, text=True, timeout=60).stdout.split()
    return int(out[0]), np.array([int(x) for x in out[1:]])


def fold(d, labels, f):
    nz = d.r != 0.0
    idx = np.arange(d.n)
    return d.subset(idx[(labels != f) & nz]), d.subset(idx[(labels == f) & nz])


def synth_multitile(seed=3, n_items=90, n_users=3 * 4096 + 500, cells=9000):
    """heavy-tailed item popularity over more users than one LDS tile holds"""
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, n_items + 1) ** 0.9
    it = rng.choice(n_items, size=cells, p=w / w.sum())
    us = rng.integers(0, n_users, size=cells)
    uniq = sorted(set(zip(us.tolist(), it.tolist())))
    u = np.array([c[0] for c in uniq], np.int32)
    i = np.array([c[1] for c in uniq], np.int32)
    r = rng.integers(1, 6, len(uniq)) / rng.integers(1, 4, len(uniq))
    return n_users, n_items, u, i, r


def handmade():
    """constant common values, single common entry, no overlap, identical vectors, anti-correlation, +-Infinity (cos / cpc), a user and
    an item with no ratings"""
    cells = [(0, 0, 3.0), (1, 0, 3.0), (2, 0, 4.0), (0, 1, 3.0), (1, 1, 3.0), (3, 1, 1.0),   # items 0, 1: constant common values
             (4, 2, 5.0), (4, 3, 2.0),                                                      # single common entry
             (5, 4, 2.0), (6, 5, 2.0),                                                      # no overlap
             (0, 6, 1.0), (1, 6, 2.0), (2, 6, 5.0), (0, 7, 1.0), (1, 7, 2.0), (2, 7, 5.0),  # identical vectors
             (3, 8, 1.0), (4, 8, 5.0), (3, 9, 5.0), (4, 9, 1.0),                            # anti-correlated
             (7, 10, 1e-170), (7, 11, 1e140), (8, 11, 3.0), (7, 12, -1e-170)]                # cos: +-Infinity
    u = np.array([c[0] for c in cells], np.int32)
    i = np.array([c[1] for c in cells], np.int32)
    r = np.array([c[2] for c in cells])
    return 11, 14, u, i, r  # users 9, 10 and item 13 have no ratings


def gpu_sim(kind, nu, ni, u, i, r, measure, shr, lo=1.0, hi=5.0):
    h = capi.KNNInstance(kind, nu, ni)
    h.set_ratings(u, i, r)
    h.build(measure, shr, lo, hi)
    S = h.similarity()
    h.close()
    return S


def check_sims(nu, ni, u, i, r, lo=1.0, hi=5.0, anchors=None):
    for kind in ("item", "user"):
        rows = knn_ref.rows_of(u, i, r, kind, nu, ni)
        n_ctr = nu if kind == "item" else ni
        for m in knn_ref.MEASURES:
            for shr in (-1, 30):
                want = knn_ref.build_corrs(rows, n_ctr, m, shr, lo, hi, anchors=anchors)
                got = gpu_sim(kind, nu, ni, u, i, r, m.upper() if shr > 0 else m, shr, lo, hi)
                if anchors is not None:  # only the restated rows (upper triangle)
                    for a in anchors:
                        assert same_bits(got[a, a + 1:], want[a, a + 1:]), (kind, m, shr, a)
                else:
                    assert same_bits(got, want), (kind, m, shr, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5])


def test_similarity_depaul(tmp_path):
    d = depaul(tmp_path)
    u, i, r = to2d(d.u, d.j, d.r)
    check_sims(d.n_users, d.n_items, u, i, r, d.min_rate, d.max_rate)


def test_similarity_frappe_fold(tmp_path):
    d = read(tmp_path, write_ratings(tmp_path))
    _, labels = folds(d.n)
    tr, _ = fold(d, labels, 1)
    u, i, r = to2d(tr.u, tr.j, tr.r)
    rng = np.random.default_rng(0)
    for kind, n in (("item", d.n_items), ("user", d.n_users)):
        anchors = sorted(set(rng.integers(0, n - 1, 40).tolist()) | {0, 1})
        rows = knn_ref.rows_of(u, i, r, kind, d.n_users, d.n_items)
        n_ctr = d.n_users if kind == "item" else d.n_items
        for m in knn_ref.MEASURES:
            for shr in (-1, 30):
                want = knn_ref.build_corrs(rows, n_ctr, m, shr, d.min_rate, d.max_rate, anchors=anchors)
                got = gpu_sim(kind, d.n_users, d.n_items, u, i, r, m, shr, d.min_rate, d.max_rate)
                for a in anchors:
                    assert same_bits(got[a, a + 1:], want[a, a + 1:]), (kind, m, shr, a)
                assert same_bits(got, got.T)


def test_similarity_multitile_synthetic():
    nu, ni, u, i, r = synth_multitile()
    check_sims(nu, ni, u, i, r)


def test_similarity_partner_chunks_by_tiles():
    """several 256-partner chunks of one anchor, each sweeping several 4 096-index tiles (twice for pcc), with empty partners between:
    the per-chunk tile generations; both kinds (the matrix and its transpose); the CPU restates a subsample of anchors that holds the
    first and last rows, empty rows and rows of every pattern"""
    n, n_ctr, ent, ctr, r = synth_chunks_by_tiles()
    anchors = sorted({0, 1, 2, 3, 4, 8, 11, 255, 256, 257, 511, 512, n - 9, n - 3, n - 2, n - 1} |
                     set(np.random.default_rng(1).integers(0, n, 24).tolist()))
    assert any(a % 8 == 0 for a in anchors) and {a % 8 for a in anchors} >= set(range(8))
    for kind in ("item", "user"):
        nu, ni, u, i = (n_ctr, n, ctr, ent) if kind == "item" else (n, n_ctr, ent, ctr)
        rows = knn_ref.rows_of(u, i, r, kind, nu, ni)
        assert len(rows) == n and any(row and row[0][0] < 4096 and row[-1][0] >= 3 * 4096 for row in rows)
        for m in knn_ref.MEASURES:
            for shr in (-1, 30):
                want = knn_ref.build_corrs(rows, n_ctr, m, shr, anchors=anchors)
                got = gpu_sim(kind, nu, ni, u, i, r, m, shr)
                for a in anchors:
                    assert same_bits(got[a, a + 1:], want[a, a + 1:]), (kind, m, shr, a)
                assert same_bits(got, got.T)


def test_similarity_handmade():
    nu, ni, u, i, r = handmade()
    check_sims(nu, ni, u, i, r)
    S = gpu_sim("item", nu, ni, u, i, r, "cos", -1)
    assert (S == math.inf).any() and (S == -math.inf).any()  # Java stores +-Infinity
    assert np.isnan(np.diag(S)).all()


def predict_case(kind, nu, ni, u, i, r, tu, tj, measure, gm, lo, hi):
    rows = knn_ref.rows_of(u, i, r, kind, nu, ni)
    S = knn_ref.build_corrs(rows, nu if kind == "item" else ni, measure, -1, lo, hi)
    means = knn_ref.row_means(rows, gm)
    lists = knn_ref.lists_of(u, i, r, kind, nu, ni)
    h = capi.KNNInstance(kind, nu, ni)
    h.set_ratings(u, i, r)
    h.build(measure, -1, lo, hi)
    assert same_bits(h.similarity(), S)
    wants, trees = {}, {}
    for knn in (0, 1, 20, 10 ** 6):
        wants[knn], trees[knn] = [], 0
        for a, b in zip(tu.tolist(), tj.tolist()):
            try:
                wants[knn].append(knn_ref.predict(kind, S, means, lists, a, b, knn, gm, True, lo, hi))
            except knn_ref.Treeified:
                trees[knn] += 1
                wants[knn].append(math.nan)
    print("%s %s: tuples whose HashMap would treeify a bin, per knn: %s (of %d)" % (kind, measure, trees, len(tu)))
    assert not any(trees.values()), "the tree-bin order is not modelled: these tuples would need it"
    for knn, want in wants.items():
        got = h.predict(tu, tj, knn, gm, True, lo, hi)
        assert same_bits(got, want), (kind, knn, np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0][:5])
    h.close()


def test_predictions_match_the_reference_run():
    """the matrix, similarities and predictions of tests/golden/reference_knn.json.gz, which the reference's own ItemKNN / UserKNN /
    Recommender source computed (tests/tools/mint_reference_knn.py): ties at the knn cut, a cut re-put into the 64-slot table clear()
    kept, empty rows"""
    import gzip
    g = json.loads(gzip.open(os.path.join(GOLDEN, "reference_knn.json.gz"), "rb").read())
    km = g["knn_matrix"]
    nu, ni = km["n_users"], km["n_items"]
    u = np.array([c[0] for c in km["cells"]], np.int32)
    i = np.array([c[1] for c in km["cells"]], np.int32)
    r = np.array([float.fromhex(c[2]) for c in km["cells"]])
    for run in g["models"]:
        kind = "item" if run["model"] == "ItemKNN" else "user"
        n = ni if kind == "item" else nu
        h = capi.KNNInstance(kind, nu, ni)
        h.set_ratings(u, i, r)
        h.build(run["measure"], run["shrinkage"], 1.0, 5.0)
        S = np.nan_to_num(h.similarity(), nan=0.0)  # SymmMatrix.get: 0 where nothing is stored
        want = np.array([float.fromhex(x) for x in run["corrs"]])
        got = np.array([S[a, b] for a in range(n) for b in range(a + 1, n)])
        assert same_bits(got, want), (run["model"], run["measure"], run["shrinkage"])
        for knn, rows in run.get("predict", {}).items():
            gm = float.fromhex(run["global_mean"])
            tu = np.repeat(np.arange(nu, dtype=np.int32), ni)
            tj = np.tile(np.arange(ni, dtype=np.int32), nu)
            got = h.predict(tu, tj, int(knn), gm, True, 1.0, 5.0)
            want = np.array([float.fromhex(x) for row in rows for x in row])
            assert same_bits(got, want), (run["model"], run["measure"], knn)
        h.close()


def test_predictions_depaul_folds(tmp_path):
    d = depaul(tmp_path)
    _, labels = folds(d.n)
    for f in (1, 2):
        tr, te = fold(d, labels, f)
        u, i, r = to2d(tr.u, tr.j, tr.r)
        gm = global_mean(tr.r)
        own = set(zip(u.tolist(), i.tolist()))
        assert any((a, b) in own for a, b in zip(te.u.tolist(), te.j.tolist()))  # j among the user's own train items
        tu = np.concatenate([te.u, np.arange(d.n_users, dtype=np.int32) % d.n_users])
        tj = np.concatenate([te.j, np.arange(d.n_users, dtype=np.int32) % d.n_items])
        for kind in ("item", "user"):
            for m in ("pcc", "cos"):  # cos on cell means gives ties at the cut
                predict_case(kind, d.n_users, d.n_items, u, i, r, tu, tj, m, gm, d.min_rate, d.max_rate)


def test_predictions_handmade_infinite_weights_and_empty_rows():
    nu, ni, u, i, r = handmade()
    tu = np.array([a for a in range(nu) for _ in range(ni)], np.int32)
    tj = np.array([b for _ in range(nu) for b in range(ni)], np.int32)
    gm = float(r.sum() / len(r))
    for kind in ("item", "user"):
        predict_case(kind, nu, ni, u, i, r, tu, tj, "cos", gm, 1.0, 5.0)
    h = capi.KNNInstance("item", nu, ni)
    h.set_ratings(u, i, r)
    h.build("cos", -1)
    assert np.isnan(h.predict(tu, tj, 0, gm)).any()  # an infinite weight makes the prediction NaN


def test_two_handles_from_two_threads(tmp_path):
    d = depaul(tmp_path)
    u, i, r = to2d(d.u, d.j, d.r)
    alone = {k: gpu_sim(k, d.n_users, d.n_items, u, i, r, "pcc", 30) for k in ("item", "user")}
    got, errs = {}, []

    def run(k):
        try:
            got[k] = gpu_sim(k, d.n_users, d.n_items, u, i, r, "pcc", 30)
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    ts = [threading.Thread(target=run, args=(k,)) for k in ("item", "user")]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not errs and all(same_bits(got[k], alone[k]) for k in alone)


def test_argument_checks():
    with pytest.raises(capi.CmiError) as e:
        capi.KNNInstance(7, 3, 3)
    assert e.value.code == capi.E_INVALID
    h = capi.KNNInstance("item", 3, 3)
    with pytest.raises(capi.CmiError) as e:
        h.set_ratings([0, 3], [0, 1], [1.0, 2.0])
    assert e.value.code == capi.E_INVALID
    with pytest.raises(capi.CmiError) as e:
        h.set_ratings([0, 0], [1, 1], [1.0, 2.0])
    assert e.value.code == capi.E_INVALID and "duplicate" in str(e.value)
    h.set_ratings([0, 1], [1, 1], [1.0, 2.0])
    h.build("pcc", -1)
    with pytest.raises(capi.CmiError) as e:
        h.predict([0], [3], 20, 3.0)
    assert e.value.code == capi.E_INVALID
    assert h.last_build_ms() >= 0.0


def test_driver_parity_depaul(tmp_path):
    d = depaul(tmp_path)
    nf, labels = folds(d.n)
    conf = open(os.path.join(GOLDEN, "depaul_setting.conf")).read().replace("PLACEHOLDER_SET_BY_TEST", str(tmp_path / "ratings.txt"))
    for algo, name, kind in (("itemknn", "ItemKNN", "item"), ("userknn", "UserKNN", "user")):
        txt = conf.replace("recommender=biasedmf", "recommender=" + algo) + "num.neighbors=20\nsimilarity=PCC\nnum.shrinkage=-1\n"
        (tmp_path / "knn.conf").write_text(txt)
        p = subprocess.run([EXE, "-c", str(tmp_path / "knn.conf"), "--precise"], capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        m = re.search(r"PRECISE %s folds=5 MAE=(\S+) RMSE=(\S+)" % name, p.stdout)
        assert m, p.stdout
        mae = rmse = 0.0
        for f in range(1, nf + 1):
            tr, te = fold(d, labels, f)
            u, i, r = to2d(tr.u, tr.j, tr.r)
            gm = global_mean(tr.r)
            rows = knn_ref.rows_of(u, i, r, kind, d.n_users, d.n_items)
            S = knn_ref.build_corrs(rows, d.n_users if kind == "item" else d.n_items, "pcc", -1, d.min_rate, d.max_rate)
            means = knn_ref.row_means(rows, gm)
            lists = knn_ref.lists_of(u, i, r, kind, d.n_users, d.n_items)
            preds = [knn_ref.predict(kind, S, means, lists, a, b, 20, gm, True, d.min_rate, d.max_rate)
                     for a, b in zip(te.u.tolist(), te.j.tolist())]
            fm, fr = knn_ref.eval_ratings(preds, te.r.tolist(), d.min_rate)
            mae += fm / nf
            rmse += fr / nf
        assert float(m.group(1)) == mae and float(m.group(2)) == rmse, (m.groups(), repr(mae), repr(rmse))


def test_driver_frappe_itemknn_parallel_folds(tmp_path):
    path = write_ratings(tmp_path)
    conf = ("dataset.ratings.lins=%s\nratings.setup=-threshold -1 -datatransformation 1 -fullstat -1\nrecommender=itemknn\n"
            "evaluation.setup=cv -k 5 -p on --rand-seed 1\nitem.ranking=off\noutput.setup=-folder CARSKit.Workspace -verbose off\n"
            "num.neighbors=20\nsimilarity=pcc\nnum.shrinkage=-1\n") % path
    (tmp_path / "frappe.conf").write_text(conf)
    p = subprocess.run([EXE, "-c", str(tmp_path / "frappe.conf"), "--precise"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    m = re.search(r"PRECISE ItemKNN folds=5 MAE=(\S+) RMSE=(\S+)", p.stdout)
    assert m and math.isfinite(float(m.group(1))), p.stdout
    print(m.group(0))
