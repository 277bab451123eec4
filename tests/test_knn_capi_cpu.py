"""ItemKNN / UserKNN without a GPU: the C ABI symbols, the no-device refusal, the measure names, the driver's refusals (decided before any
device work), and the CPU restatement (tests/knn_ref.py) against itself and hand-derived answers."""
import math
import os
import subprocess

import numpy as np
import pytest

from carskit_amd import capi
from tests import knn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carskit_amd", "bin", "carskit-mi355x")
GOLDEN = os.path.join(ROOT, "tests", "golden")

KNN_SYMBOLS = ("cmi_knn_measure", "cmi_knn_create", "cmi_knn_destroy", "cmi_knn_last_error", "cmi_knn_set_ratings", "cmi_knn_build",
               "cmi_knn_get_similarity", "cmi_knn_predict_batch", "cmi_knn_last_build_ms")


def test_knn_symbols_load():
    L = capi.lib()
    bound = {name for name, _, _ in capi.SYMBOLS}
    for s in KNN_SYMBOLS:
        assert s in bound and getattr(L, s) is not None
    assert L.cmi_abi_version() == 5


def test_measure_names_case_insensitive_unknown_is_pcc():
    assert [capi.knn_measure(n) for n in ("pcc", "COS", "Cos-Binary", "msd", "CPC", "exJaccard")] == list(range(6))
    for n in ("", "pearson", "jaccard", "dice"):
        assert capi.knn_measure(n) == capi.SIM_PCC
        assert knn_ref.measure_name(n) == "pcc"


def test_knn_instance_without_device():
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(capi.CmiError) as e:
        capi.KNNInstance("item", 10, 10)
    assert e.value.code == capi.E_NO_DEVICE and "no CPU fallback" in str(e.value)


def _conf(tmp_path, extra):
    import shutil
    shutil.copyfile(os.path.join(GOLDEN, "depaul_ratings_compact.csv"), tmp_path / "ratings.txt")
    conf = open(os.path.join(GOLDEN, "depaul_setting.conf")).read().replace("PLACEHOLDER_SET_BY_TEST", str(tmp_path / "ratings.txt"))
    lines = [ln for ln in conf.splitlines() if not ln.startswith(("recommender", "item.ranking"))]
    (tmp_path / "setting.conf").write_text("\n".join(lines + extra) + "\n")
    return str(tmp_path / "setting.conf")


@pytest.mark.parametrize("algo", ["itemknn", "UserKNN"])
def test_driver_refuses_knn_top_n(tmp_path, algo):
    conf = _conf(tmp_path, ["recommender=" + algo, "item.ranking=on -topN 10"])
    p = subprocess.run([EXE, "-c", conf], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "top-N" in p.stderr and "not accelerated yet" in p.stderr, p.stderr
    assert "Rating data set has been successfully loaded." not in p.stdout


def test_driver_refuses_knn_shards(tmp_path):
    conf = _conf(tmp_path, ["recommender=itemknn", "item.ranking=off"])
    p = subprocess.run([EXE, "-c", conf, "--shards", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "--shards 2" in p.stderr, p.stderr


def test_restatement_vectorised_equals_scalar():
    """build_corrs (vectorised over partners) is the scalar correlation() bit for bit, every measure, with and without shrinkage"""
    rng = np.random.default_rng(5)
    n_u, n_i = 30, 9
    cells = sorted({(int(rng.integers(n_u)), int(rng.integers(n_i))) for _ in range(140)})
    u = np.array([c[0] for c in cells])
    i = np.array([c[1] for c in cells])
    r = rng.integers(1, 6, len(cells)) / rng.integers(1, 4, len(cells))  # cell means: 5/3 and the like
    r[:6] = 3.0
    for kind in ("item", "user"):
        rows = knn_ref.rows_of(u, i, r, kind, n_u, n_i)
        n_ctr = n_u if kind == "item" else n_i
        for m in knn_ref.MEASURES:
            for shr in (-1, 30):
                S = knn_ref.build_corrs(rows, n_ctr, m, shr)
                for a in range(len(rows)):
                    for b in range(a + 1, len(rows)):
                        if not rows[a] or not rows[b]:
                            assert math.isnan(S[a, b])
                            continue
                        want = knn_ref.correlation(rows[a], rows[b], m, shr)
                        got = S[a, b]
                        assert (math.isnan(want) and math.isnan(got)) or want.hex() == float(got).hex(), (kind, m, shr, a, b)


def test_sims_known_answers():
    iv, jv = [(0, 2.0), (3, 2.0), (5, 4.0)], [(0, 2.0), (3, 2.0), (7, 1.0)]
    assert math.isnan(knn_ref.correlation(iv, jv, "pcc", -1))           # constant common values: 0/0
    assert knn_ref.correlation(iv, jv, "msd", -1) == 1.0                  # identical common values: n/0 = Infinity -> 1.0
    cos = 8.0 / (math.sqrt(8.0) * math.sqrt(8.0))
    assert knn_ref.correlation(iv, jv, "cos", -1) == cos == 0.9999999999999998
    assert knn_ref.correlation(iv, jv, "exjaccard", -1) == 1.0
    assert knn_ref.correlation(iv, jv, "cos", 2) == cos * (2 / 4.0)        # shrinkage n/(n+s)
    assert math.isnan(knn_ref.correlation([(1, 3.0)], [(2, 3.0)], "cos", -1))   # no overlap
    assert knn_ref.correlation([(1, 3.0)], [(2, 3.0)], "cos-binary", -1) == 0.0  # full-vector inner products: 0 / 9
    assert math.isnan(knn_ref.correlation([(1, 3.0)], [(1, 5.0)], "pcc", -1))   # a single common entry
    assert knn_ref.correlation([(1, 1.0), (2, 5.0)], [(1, 5.0), (2, 1.0)], "pcc", -1) == -cos  # anti-correlated: -8 / (sqrt(8) * sqrt(8))
    # +-Infinity: the products survive while the squares underflow (Java stores these)
    assert knn_ref.correlation([(0, 1e-170)], [(0, 1e140)], "cos", -1) == math.inf
    assert knn_ref.correlation([(0, -1e-170)], [(0, 1e140)], "cos", -1) == -math.inf


def test_java_hashmap_order():
    m = knn_ref.JavaIntHashMap()
    for k in (1, 17, 2, 33, 16):
        m.put(k, 1.0)
    assert [k for k, _ in m.items()] == [16, 1, 17, 33, 2]
    m = knn_ref.JavaIntHashMap()
    for k in range(13):  # all in bucket 0 of 16 slots: the 9th put makes a 9-node list, treeifyBin resizes to 32 slots (threshold 24)
        m.put(k * 16, 1.0)
    assert m.cap == 32
    assert [k for k, _ in m.items()] == [0, 32, 64, 96, 128, 160, 192, 16, 48, 80, 112, 144, 176]
    m = knn_ref.JavaIntHashMap()
    for k in range(1, 26):  # 25 keys: 64 slots
        m.put(k, 1.0)
    assert m.cap == 64
    with pytest.raises(knn_ref.Treeified):  # the 9th key of bucket 0 of a 64-slot table
        for k in range(64, 64 * 10, 64):
            m.put(k, 1.0)
