"""SlopeOne on the GPU through the C ABI, bit for bit: against the run of the reference's own source
(tests/golden/reference_slopeone.json.gz) and, on shapes that take every path of the two kernels, against the CPU restatement
(tests/slopeone_ref.py); the argument checks; and the driver's MAE / RMSE on DePaul (cv -k 5) against the restatement over the same
folds."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from carskit_amd import capi, dao
from tests import slopeone_ref as sref
from tests.hostmirror import splitter
from tests.knn_ref import eval_ratings
from tests.util import global_mean, same_bits_exact, synth_chunks_by_tiles, to2d

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carskit_amd", "bin", "carskit-mi355x")
GOLDEN = os.path.join(ROOT, "tests", "golden")

TILE = 4096  # PAIR_TILE: users per LDS tile of the anchor's column


def all_tuples(nu, ni):
    return np.repeat(np.arange(nu, dtype=np.int32), ni), np.tile(np.arange(ni, dtype=np.int32), nu)


def built(nu, ni, u, i, r):
    h = capi.SlopeOneInstance(nu, ni)
    h.set_ratings(u, i, r)
    h.build()
    return h


def test_golden_matrices_match_the_reference_run():
    for run in sref.golden_runs():
        nu, ni = run["n_users"], run["n_items"]
        h = built(nu, ni, run["u"], run["i"], run["r"])
        dev, card = h.deviation()
        assert np.array_equal(card, run["card"]), run["name"]
        assert same_bits_exact(dev, run["dev"]), (run["name"], np.argwhere(dev.view(np.int64) != run["dev"].view(np.int64))[:5])
        tu, tj = all_tuples(nu, ni)
        gm, lo, hi = run["global_mean"], run["min_rate"], run["max_rate"]
        assert same_bits_exact(h.predict(tu, tj, gm).reshape(nu, ni), run["predict"]), run["name"]
        assert same_bits_exact(h.predict(tu, tj, gm, True, lo, hi).reshape(nu, ni), run["predict_bounded"]), run["name"]
        d1, c1 = h.deviation(1, 2)                                       # a row range; one destination only
        assert same_bits_exact(d1, run["dev"][1:3]) and np.array_equal(c1, run["card"][1:3])
        out = np.empty((2, ni))
        h._chk(h.L.cmi_slope_get_deviation(h.h, 1, 2, capi._p(out), None))
        assert same_bits_exact(out, run["dev"][1:3])
        outc = np.empty((2, ni), np.int32)
        h._chk(h.L.cmi_slope_get_deviation(h.h, 1, 2, None, capi._p(outc)))
        assert np.array_equal(outc, run["card"][1:3])
        h.close()


def two_tile_matrix():
    """4 100 users x 300 items, ~20 K cells, values k/3.  Users 4 096..4 099 (the second LDS tile) rate most items, so most anchor columns
    have entries on both sides of user 4 096; 299 partners for anchor 0 make a second chunk of 256 lanes.  Column 8 duplicates column 7,
    column 20 has users of the second tile only, column 30 is empty, columns 40 / 41 have even / odd users only (disjoint)."""
    rng = np.random.default_rng(20261018)
    nu, ni = TILE + 4, 300
    cells = {}
    for j in range(ni):
        for u in rng.choice(TILE, int(rng.integers(40, 90)), replace=False).tolist():
            cells[(u, j)] = float(rng.integers(3, 16)) / 3.0
        for u in range(TILE, nu):
            if rng.random() < 0.7:
                cells[(u, j)] = float(rng.integers(3, 16)) / 3.0
    for (u, j) in [k for k in cells if k[1] in (8, 30) or (k[1] == 20 and k[0] < TILE) or (k[1] == 40 and k[0] % 2) or
                   (k[1] == 41 and k[0] % 2 == 0)]:
        del cells[(u, j)]
    for (u, j), v in list(cells.items()):
        if j == 7:
            cells[(u, 8)] = v
    cells[(TILE, 20)] = 5.0 / 3.0
    cells[(TILE + 3, 20)] = 4.0
    keys = sorted(cells)
    return nu, ni, np.array([k[0] for k in keys], np.int32), np.array([k[1] for k in keys], np.int32), np.array([cells[k] for k in keys])


def test_build_two_lds_tiles_and_two_partner_chunks():
    nu, ni, u, i, r = two_tile_matrix()
    cols = sref.cols_of(u, i, r, ni)
    assert 19000 <= len(r) <= 23000 and ni - 1 > 256
    assert sum(1 for c in cols if c and c[0][0] < TILE <= c[-1][0]) > 250          # columns on both sides of user 4 096
    assert cols[7] == cols[8] and cols[20][0][0] >= TILE and not cols[30]
    assert not {x for x, _ in cols[40]} & {x for x, _ in cols[41]} and cols[40] and cols[41]
    rows = sref.rows_of(u, i, r, nu)
    want_dev, want_card = sref.build(rows, ni)
    h = built(nu, ni, u, i, r)
    dev, card = h.deviation()
    assert np.array_equal(card, want_card)
    assert same_bits_exact(dev, want_dev), np.argwhere(dev.view(np.int64) != want_dev.view(np.int64))[:5]
    assert card[7, 8] == len(cols[7]) and dev[7, 8] == 0 and not np.signbit(dev[7, 8]) and not np.signbit(dev[8, 7])
    assert card[40, 41] == 0 and not card[30].any() and not card[:, 30].any()
    assert card[20, 0] > 0 and card[20].max() <= 4
    rng = np.random.default_rng(1)
    tu = np.concatenate([rng.integers(0, nu, 600), np.arange(TILE, nu).repeat(4)]).astype(np.int32)
    tj = np.concatenate([rng.integers(0, ni, 600), np.tile([7, 20, 30, 41], 4)]).astype(np.int32)
    gm = 3.125
    for bound in (False, True):
        want = [sref.predict(want_dev, want_card, rows, a, b, gm, bound, 1.0, 5.0) for a, b in zip(tu.tolist(), tj.tolist())]
        assert same_bits_exact(h.predict(tu, tj, gm, bound, 1.0, 5.0), want), bound
    assert h.last_build_ms() > 0.0
    h.close()


def test_build_partner_chunks_by_tiles():
    """the matrix of test_gpu_knn's test of the same name, its 640 compared rows as items and its 12 888 contracted indices as users:
    three 256-partner chunks of one anchor, each sweeping up to four 4 096-user tiles, anchors with nothing in the middle tiles (a tile
    is skipped, the generation runs on into the next chunk) and empty columns between; the CPU restates the same subsample of anchors"""
    ni, nu, i, u, r = synth_chunks_by_tiles()
    anchors = sorted({0, 1, 2, 3, 4, 8, 11, 255, 256, 257, 511, 512, ni - 9, ni - 3, ni - 2, ni - 1} |
                     set(np.random.default_rng(1).integers(0, ni, 24).tolist()))
    cols = sref.cols_of(u, i, r, ni)
    assert (ni, nu) == (640, 3 * TILE + 600) and 16000 <= len(r) <= 18000 and ni - 1 > 2 * 256
    assert not any(cols[a] for a in range(0, ni, 8)) and {a % 8 for a in anchors} >= set(range(8))
    tiles = [{x // TILE for x, _ in cols[a]} for a in anchors]
    assert any(t == {0, 1, 2, 3} for t in tiles) and any(min(t) == 0 and max(t) == 3 and len(t) < 4 for t in tiles if t)
    want = sref.build_rows(cols, anchors)
    h = built(nu, ni, u, i, r)
    dev, card = h.deviation()
    h.close()
    for a in anchors:
        assert np.array_equal(card[a], want[a][1]), a
        assert same_bits_exact(dev[a], want[a][0]), (a, np.nonzero(dev[a].view(np.int64) != want[a][0].view(np.int64))[0][:5])
    assert np.array_equal(card, card.T) and card.any()


def long_lists_matrix():
    """6 users x 200 items, values k/3: user 0 rates 150 items (three chunks of 64 in the prediction, the last partial), user 1 exactly
    64 (one full chunk), user 2 65, user 3 three, user 4 one, user 5 none"""
    rng = np.random.default_rng(7)
    nu, ni = 6, 200
    cells = {}
    for u, cnt in ((0, 150), (1, 64), (2, 65), (3, 3), (4, 1)):
        for j in rng.choice(ni, cnt, replace=False).tolist():
            cells[(u, j)] = float(rng.integers(3, 16)) / 3.0
    keys = sorted(cells)
    return nu, ni, np.array([k[0] for k in keys], np.int32), np.array([k[1] for k in keys], np.int32), np.array([cells[k] for k in keys])


def test_predict_chunks_of_64_carry_the_sum():
    nu, ni, u, i, r = long_lists_matrix()
    rows = sref.rows_of(u, i, r, nu)
    assert [len(x) for x in rows] == [150, 64, 65, 3, 1, 0]
    want_dev, want_card = sref.build(rows, ni)
    h = built(nu, ni, u, i, r)
    dev, card = h.deviation()
    assert np.array_equal(card, want_card) and same_bits_exact(dev, want_dev)
    tu, tj = all_tuples(nu, ni)   # every j: the user's own items of every chunk (i == j at positions 0..149) and the unrated ones
    own0 = [j for j, _ in rows[0]]
    assert set(own0[64:]) and len(set(range(ni)) - set(own0)) == 50
    gm = 10.0 / 3.0
    for bound in (False, True):
        want = [sref.predict(want_dev, want_card, rows, a, b, gm, bound, 1.0, 5.0) for a, b in zip(tu.tolist(), tj.tolist())]
        got = h.predict(tu, tj, gm, bound, 1.0, 5.0)
        assert same_bits_exact(got, want), (bound, np.nonzero(got != np.array(want))[0][:5])
    assert (h.predict(tu, tj, gm).reshape(nu, ni)[5] == gm).all()
    h.close()


def test_one_item_and_no_tuples():
    h = built(3, 1, [0, 2], [0, 0], [4.0, 2.0])
    dev, card = h.deviation()
    assert dev.tolist() == [[0.0]] and card.tolist() == [[0]]
    assert h.predict([0, 1, 2], [0, 0, 0], 3.0).tolist() == [3.0, 3.0, 3.0]
    assert len(h.predict([], [], 3.0)) == 0
    h.close()
    h = capi.SlopeOneInstance(4, 5)
    h.set_ratings([], [], [])     # no cells at all
    h.build()
    dev, card = h.deviation()
    assert not dev.any() and not card.any() and not np.signbit(dev).any()
    assert h.predict([1], [2], 2.5).tolist() == [2.5]
    h.close()


def test_refusals():
    h = capi.SlopeOneInstance(3, 3)
    with pytest.raises(capi.CmiError) as e:
        h.set_ratings([0, 0], [1, 1], [1.0, 2.0])
    assert e.value.code == capi.E_INVALID and "duplicate" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        h.set_ratings([0, 3], [0, 1], [1.0, 2.0])
    assert e.value.code == capi.E_INVALID
    with pytest.raises(capi.CmiError) as e:
        h.build()                                                         # no ratings yet
    assert e.value.code == capi.E_INVALID
    h.set_ratings([0, 1], [1, 1], [1.0, 2.0])
    with pytest.raises(capi.CmiError) as e:
        h.predict([0], [1], 3.0)                                          # predict before build
    assert e.value.code == capi.E_INVALID and "cmi_slope_build first" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        h.deviation()
    assert e.value.code == capi.E_INVALID
    h.build()
    for row0, nrows in ((2, 2), (-1, 1), (0, 4), (3, 1)):
        with pytest.raises(capi.CmiError) as e:
            h.deviation(row0, nrows)
        assert e.value.code == capi.E_INVALID and "out of range" in str(e.value)
    assert h.deviation(3, 0)[0].shape == (0, 3)
    with pytest.raises(capi.CmiError) as e:
        h.predict([0], [3], 3.0)
    assert e.value.code == capi.E_INVALID
    with pytest.raises(capi.CmiError) as e:
        capi.SlopeOneInstance(0, 3)
    assert e.value.code == capi.E_INVALID
    h.close()


def test_driver_parity_depaul(tmp_path):
    shutil.copyfile(os.path.join(GOLDEN, "depaul_ratings_compact.csv"), tmp_path / "ratings.txt")
    dao.transform(str(tmp_path / "ratings.txt"), str(tmp_path / "train.csv"))
    d = dao.DataDAO(str(tmp_path / "train.csv")).rating_data()
    labels, nf = splitter.split_folds(d.n, 5, 1)
    conf = open(os.path.join(GOLDEN, "depaul_setting.conf")).read().replace("PLACEHOLDER_SET_BY_TEST", str(tmp_path / "ratings.txt"))
    (tmp_path / "slope.conf").write_text(conf.replace("recommender=biasedmf", "recommender=slopeone"))
    p = subprocess.run([EXE, "-c", str(tmp_path / "slope.conf")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    m = re.search(r"Final Results by SlopeOne, MAE: (\S+), RMSE: (\S+),", p.stdout)
    assert m, p.stdout
    mae = rmse = 0.0
    for f in range(1, nf + 1):
        tr, te = splitter.kth_fold(d, labels, f)
        u, i, r = to2d(tr.u, tr.j, tr.r)
        rows = sref.rows_of(u, i, r, d.n_users)
        dev, card = sref.build(rows, d.n_items)
        gm = global_mean(tr.r)
        preds = [sref.predict(dev, card, rows, a, b, gm, True, d.min_rate, d.max_rate) for a, b in zip(te.u.tolist(), te.j.tolist())]
        fm, fr = eval_ratings(preds, te.r.tolist(), d.min_rate)
        mae += fm / nf
        rmse += fr / nf
    assert (m.group(1), m.group(2)) == ("%.6f" % mae, "%.6f" % rmse), (m.groups(), repr(mae), repr(rmse))
