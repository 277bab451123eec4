"""NMF on the GPU through the C ABI: W, H and the predictions bit for bit against the run of the reference's own source
(tests/golden/reference_nmf.json.gz) and, on a matrix that takes every path of the row kernel at six factor counts, against the CPU
restatement (tests/nmf_ref.py); the loss within the bound its fixed summation order allows; run-to-run reproducibility; the argument
checks; and the driver's MAE / RMSE on DePaul (cv -k 5) against the restatement over the same folds."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from carskit_amd import capi, dao
from tests import nmf_ref as nref
from tests.hostmirror import splitter
from tests.hostmirror.javarand import JavaRandom
from tests.knn_ref import eval_ratings
from tests.util import same_bits_exact, to2d

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carskit_amd", "bin", "carskit-mi355x")
GOLDEN = os.path.join(ROOT, "tests", "golden")

CHUNK = 64  # NMF_CHUNK: entries of a row per pass of the row kernel, one per lane


def all_tuples(nu, ni):
    return np.repeat(np.arange(nu, dtype=np.int32), ni), np.tile(np.arange(ni, dtype=np.int32), nu)


def loss_close(got, want, n):
    """The per-cell terms are bit-identical; only the order of a sum of n non-negative doubles differs.  Each order is within a relative
    (n - 1) * 2^-53 of the exact sum, to first order, so two orders are within 2 n 2^-53 of each other."""
    print("loss gpu %r ref %r |diff| %r bound %r" % (got, want, abs(got - want), 2 * n * 2.0 ** -53 * want))
    return abs(got - want) <= 2 * n * 2.0 ** -53 * want


def test_golden_runs_match_the_reference_run():
    for run in nref.golden_runs():
        nu, ni, k = run["n_users"], run["n_items"], run["k"]
        n = int(np.count_nonzero(run["r"] > 0))
        assert n < 10 ** 4
        h = capi.NMFInstance(k, nu, ni)
        h.set_ratings(run["u"], run["i"], run["r"])
        h.set_model(run["W0"], run["H0"])
        for it, want in enumerate(run["iters"]):
            loss = h.iterate()
            W, H = h.model()
            assert same_bits_exact(W, want["W"]), (run["name"], it, np.argwhere(W != want["W"])[:5])
            assert same_bits_exact(H, want["H"]), (run["name"], it, np.argwhere(H != want["H"])[:5])
            assert loss_close(loss, want["loss"], n), (run["name"], it, loss, want["loss"])
        tu, tj = all_tuples(nu, ni)
        lo, hi = run["min_rate"], run["max_rate"]
        assert same_bits_exact(h.predict(tu, tj).reshape(nu, ni), run["predict"]), run["name"]
        assert same_bits_exact(h.predict(tu, tj, True, lo, hi).reshape(nu, ni), run["predict_bounded"]), run["name"]
        assert all(ms >= 0.0 for ms in h.last_iter_ms()) and sum(h.last_iter_ms()) > 0.0
        h.close()


@functools.lru_cache(maxsize=None)
def edge_matrix():
    """300 users x 200 items, values m / 3.  User 0 and item 0 are empty; user 1 and item 1 have one entry; user 2 / item 2 exactly CHUNK;
    user 3 / item 3 CHUNK + 1; user 4 rates items 1..199 and item 4 has 250 users (three chunks and a part); the others 5..20 entries."""
    rng = np.random.default_rng(20261019)
    nu, ni = 300, 200
    val = lambda: float(rng.integers(3, 16)) / 3.0  # noqa: E731
    cells = {}
    for u in range(5, nu):
        for j in rng.choice(np.arange(5, ni), int(rng.integers(5, 21)), replace=False).tolist():
            cells[(u, j)] = val()
    for j in range(1, ni):
        cells[(4, j)] = val()
    for j, cnt in ((2, CHUNK - 1), (3, CHUNK), (4, 249)):
        for u in rng.choice(np.arange(5, nu), cnt, replace=False).tolist():
            cells[(u, j)] = val()
    for u, cnt in ((1, 1), (2, CHUNK), (3, CHUNK + 1)):
        for j in rng.choice(np.arange(5, ni), cnt, replace=False).tolist():
            cells[(u, j)] = val()
    keys = sorted(cells)
    u, i = np.array([c[0] for c in keys], np.int32), np.array([c[1] for c in keys], np.int32)
    r = np.array([cells[c] for c in keys])
    return nu, ni, u, i, r, nref.rows_of(u, i, r, nu), nref.cols_of(u, i, r, ni)


def test_edge_matrix_has_the_edges():
    nu, ni, u, i, r, rows, cols = edge_matrix()
    ul, il = [len(x[0]) for x in rows], [len(x[0]) for x in cols]
    assert ul[:5] == [0, 1, CHUNK, CHUNK + 1, ni - 1] and ul[4] >= 3 * CHUNK
    assert il[:5] == [0, 1, CHUNK, CHUNK + 1, 250] and il[4] >= 3 * CHUNK
    assert 3000 <= len(r) <= 6000 and min(ul[5:]) >= 5


@pytest.mark.parametrize("k", [1, 10, 64, 65, 128, 256])
def test_row_kernel_edges(k):
    nu, ni, u, i, r, rows, cols = edge_matrix()
    rng = np.random.default_rng(k)
    W0, H0 = rng.random((nu, k)), rng.random((k, ni))
    W0[6] = 0.0                                     # real = 0 for every factor; the 1e-9 keeps 0 / estm finite
    assert len(rows[6][0]) > 0
    W, Ht = W0.copy(), np.ascontiguousarray(H0.T)
    h = capi.NMFInstance(k, nu, ni)
    h.set_ratings(u, i, r)
    h.set_model(W0, H0)
    for it in range(2):
        want = nref.iterate(W, Ht, rows, cols)
        loss = h.iterate()
        gW, gH = h.model()
        assert same_bits_exact(gW, W), (k, it, np.argwhere(gW != W)[:5])
        assert same_bits_exact(gH, Ht.T), (k, it, np.argwhere(gH != Ht.T)[:5])
        assert loss_close(loss, want, len(r)), (k, it, loss, want)
    assert same_bits_exact(gW[0], W0[0]) and same_bits_exact(gH[:, 0], H0[:, 0])          # the empty user and item: untouched
    assert not gW[6].any() and np.isfinite(gW).all() and np.isfinite(gH).all()
    assert not same_bits_exact(gW[1], W0[1])                                              # one entry is enough to move a row
    tu, tj = rng.integers(0, nu, 500).astype(np.int32), rng.integers(0, ni, 500).astype(np.int32)
    want = nref.products(W, Ht, tu, tj)
    assert same_bits_exact(h.predict(tu, tj), want)
    assert same_bits_exact(h.predict(tu, tj, True, 1.0, 5.0), np.where(want > 5.0, 5.0, np.where(want < 1.0, 1.0, want)))
    h.close()


def test_same_model_same_bits():
    nu, ni, u, i, r, _, _ = edge_matrix()
    k = 10
    rng = np.random.default_rng(3)
    W0, H0 = 0.01 * rng.random((nu, k)), 0.01 * rng.random((k, ni))
    h = capi.NMFInstance(k, nu, ni)
    h.set_ratings(u, i, r)
    out = []
    for _ in range(2):
        h.set_model(W0, H0)
        losses = [h.iterate(), h.iterate()]
        out.append((losses, *h.model()))
    assert same_bits_exact(out[0][0], out[1][0]) and same_bits_exact(out[0][1], out[1][1]) and same_bits_exact(out[0][2], out[1][2])
    h.set_model(H=H0)                                # one side only: W stays
    assert same_bits_exact(h.model()[0], out[1][1]) and same_bits_exact(h.model()[1], H0)
    h.close()


def test_zero_cells_take_no_part_and_no_cells_at_all():
    u, i, r = [0, 0, 1, 2], [0, 1, 1, 0], [4.0, 2.0, 5.0 / 3.0, 3.0]
    rng = np.random.default_rng(5)
    W0, H0 = rng.random((3, 2)), rng.random((2, 2))
    res = []
    for extra in ([], [(1, 0, 0.0)]):
        h = capi.NMFInstance(2, 3, 2)
        h.set_ratings(u + [c[0] for c in extra], i + [c[1] for c in extra], r + [c[2] for c in extra])
        h.set_model(W0, H0)
        res.append((h.iterate(), *h.model()))
        h.close()
    assert res[0][0] == res[1][0] and same_bits_exact(res[0][1], res[1][1]) and same_bits_exact(res[0][2], res[1][2])
    h = capi.NMFInstance(2, 3, 2)
    h.set_ratings([], [], [])
    h.set_model(W0, H0)
    assert h.iterate() == 0.0 and same_bits_exact(h.model()[0], W0) and same_bits_exact(h.model()[1], H0)
    assert len(h.predict([], [])) == 0
    h.close()


def test_refusals():
    h = capi.NMFInstance(2, 3, 3)
    with pytest.raises(capi.CmiError) as e:
        h.set_ratings([0, 0], [1, 1], [1.0, 2.0])
    assert e.value.code == capi.E_INVALID and "duplicate" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        h.set_ratings([0, 3], [0, 1], [1.0, 2.0])
    assert e.value.code == capi.E_INVALID and "out of range" in str(e.value)
    W0, H0 = np.full((3, 2), 0.5), np.full((2, 3), 0.25)
    for call in (h.iterate, lambda: h.predict([0], [1]), h.model, h.last_iter_ms):      # nothing set yet
        with pytest.raises(capi.CmiError) as e:
            call()
        assert e.value.code == capi.E_INVALID
    h.set_model(W0, H0)
    with pytest.raises(capi.CmiError) as e:
        h.iterate()                                                                     # a model, but no ratings
    assert e.value.code == capi.E_INVALID and "cmi_nmf_set_ratings first" in str(e.value)
    h.close()
    h = capi.NMFInstance(2, 3, 3)
    h.set_ratings([0, 1, 2], [1, 1, 0], [1.0, 2.0, 3.0])
    with pytest.raises(capi.CmiError) as e:
        h.iterate()                                                                     # ratings, but no model
    assert e.value.code == capi.E_INVALID and "cmi_nmf_set_model first" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        h.set_model(W=W0)                                                               # the first call sets both sides
    assert e.value.code == capi.E_INVALID
    for W, H in ((W0.T, H0), (W0, H0.T), (W0[:2], H0), (W0, H0[:, :2])):                # wrong shapes
        with pytest.raises(capi.CmiError) as e:
            h.set_model(W, H)
        assert e.value.code == capi.E_INVALID and "shape" in str(e.value)
    h.set_model(W0, H0)
    with pytest.raises(capi.CmiError) as e:
        h.predict([0], [3])
    assert e.value.code == capi.E_INVALID
    Wn = W0.copy()
    Wn[1, 0] = np.nan
    h.set_model(Wn, H0)
    with pytest.raises(capi.CmiError) as e:
        h.iterate()
    assert e.value.code == capi.E_NUMERIC and "NaN" in str(e.value)
    h.close()
    for k in (0, 257, -1):
        with pytest.raises(capi.CmiError) as e:
            capi.NMFInstance(k, 3, 3)
        assert e.value.code == capi.E_INVALID
    capi.NMFInstance(256, 3, 3).close()
    with pytest.raises(capi.CmiError) as e:
        capi.NMFInstance(2, 0, 3)
    assert e.value.code == capi.E_INVALID


def test_driver_parity_depaul(tmp_path):
    iters, k = 3, 10
    shutil.copyfile(os.path.join(GOLDEN, "depaul_ratings_compact.csv"), tmp_path / "ratings.txt")
    dao.transform(str(tmp_path / "ratings.txt"), str(tmp_path / "train.csv"))
    d = dao.DataDAO(str(tmp_path / "train.csv")).rating_data()
    labels, nf = splitter.split_folds(d.n, 5, 1)
    conf = open(os.path.join(GOLDEN, "depaul_setting.conf")).read().replace("PLACEHOLDER_SET_BY_TEST", str(tmp_path / "ratings.txt"))
    assert "num.max.iter=100" in conf and "num.factors=%d" % k in conf and "--rand-seed 1" in conf
    (tmp_path / "nmf.conf").write_text(conf.replace("recommender=biasedmf", "recommender=nmf").replace("num.max.iter=100",
                                                                                                      "num.max.iter=%d" % iters))
    p = subprocess.run([EXE, "-c", str(tmp_path / "nmf.conf")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    m = re.search(r"Final Results by NMF, MAE: (\S+), RMSE: (\S+),", p.stdout)
    assert m, p.stdout
    mae = rmse = 0.0
    for f in range(1, nf + 1):
        tr, te = splitter.kth_fold(d, labels, f)
        u, i, r = to2d(tr.u, tr.j, tr.r)
        rows, cols = nref.rows_of(u, i, r, d.n_users), nref.cols_of(u, i, r, d.n_items)
        W, Ht = nref.init_model(JavaRandom(1), d.n_users, d.n_items, k)      # P and Q drawn (and dropped) first
        for _ in range(iters):
            nref.iterate(W, Ht, rows, cols)
        pred = nref.products(W, Ht, te.u, te.j)
        pred = np.where(pred > d.max_rate, d.max_rate, np.where(pred < d.min_rate, d.min_rate, pred))
        fm, fr = eval_ratings(pred.tolist(), te.r.tolist(), d.min_rate)
        mae += fm / nf
        rmse += fr / nf
    assert (m.group(1), m.group(2)) == ("%.6f" % mae, "%.6f" % rmse), (m.groups(), repr(mae), repr(rmse))
