"""SLIM without a GPU: the C ABI symbols (header, binding table, library), the no-device refusal, the factory entry, and the driver's
refusal (decided before any data or device work)."""
import os
import re
import shutil
import subprocess

import pytest

import numpy as np

from carskit_amd import capi
from tests import knn_ref
from tests import slim_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carskit_amd", "bin", "carskit-mi355x")
GOLDEN = os.path.join(ROOT, "tests", "golden")

SLIM_SYMBOLS = ("cmi_slim_create", "cmi_slim_destroy", "cmi_slim_last_error", "cmi_slim_set_ratings", "cmi_slim_build_neighbors",
                "cmi_slim_cut_neighbors", "cmi_slim_get_neighbors", "cmi_slim_set_weights", "cmi_slim_get_weights", "cmi_slim_iterate", "cmi_slim_predict_batch",
                "cmi_slim_eval_rankings", "cmi_slim_last_build_ms", "cmi_slim_last_iter_ms")


def test_slim_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "carskit_mi355x.h")).read()
    assert sorted(set(re.findall(r"\b(cmi_slim_\w+)\(", header))) == sorted(SLIM_SYMBOLS)
    L = capi.lib()
    bound = {name for name, _, _ in capi.SYMBOLS}
    assert {n for n in bound if n.startswith("cmi_slim_")} == set(SLIM_SYMBOLS)
    for s in SLIM_SYMBOLS:
        assert getattr(L, s) is not None
    assert L.cmi_abi_version() == 5
    for m in ("set_ratings", "build_neighbors", "neighbors", "set_weights", "weights", "iterate", "predict", "eval_rankings",
              "last_build_ms", "last_iter_ms", "close"):
        assert callable(getattr(capi.SLIMInstance, m))


def _row(keys, n, seed):
    rng = np.random.default_rng(seed)
    sims = np.full(n, np.nan)
    sims[list(keys)] = np.round(rng.random(len(keys)) - 0.3, 2)   # ties, negative values, and some exact zeros (not neighbours)
    return sims


def test_neighbour_cut_equals_the_restatement_on_the_host():
    """cmi_slim_cut_neighbors (the per-item step of cmi_slim_build_neighbors: the map, the cut, the 4-slot value set) against
    tests/slim_ref.cut_neighbors, without a device: plain rows on both sides of every growth step, and keys that fall into ONE bin of
    every table up to 65 536 slots (key = a * 65536 + (a ^ 5): hash = key ^ key >> 16 has the low bits 5)"""
    for n_keys in (0, 1, 3, 4, 6, 7, 12, 13, 24, 25, 48, 49, 97, 300):
        sims = _row(np.random.default_rng(n_keys).choice(400, n_keys, replace=False), 400, n_keys)
        for knn in (1, 3, 4, 7, 13, 25, 1000):
            assert capi.slim_cut_neighbors(sims, knn) == sref.cut_neighbors(sims, knn), (n_keys, knn)
    collide = [a * 65536 + (a ^ 5) for a in range(12)]
    for n_keys in (8, 9, 10):   # the 9th and 10th key in one bin double the table (16 -> 32 -> 64): treeifyBin's resize, no tree yet
        sims = _row(collide[:n_keys], collide[11] + 1, n_keys)
        sims[collide[:n_keys]] += 2.0                                 # none is 0.0
        for knn in (3, 1000):
            got = capi.slim_cut_neighbors(sims, knn)
            assert got == sref.cut_neighbors(sims, knn) and len(got) == min(knn, n_keys), (n_keys, knn)
    sims = _row(collide[:11], collide[11] + 1, 11) + 2.0              # the 11th meets 8 nodes in a 64-slot table: a tree bin
    with pytest.raises(knn_ref.Treeified):
        sref.cut_neighbors(sims, 1000)
    with pytest.raises(capi.CmiError) as e:
        capi.slim_cut_neighbors(sims, 1000)
    assert e.value.code == capi.E_UNSUPPORTED and "treeify" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        capi.slim_cut_neighbors(sims, 0)
    assert e.value.code == capi.E_INVALID


def test_slim_instance_without_device():
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(capi.CmiError) as e:
        capi.SLIMInstance(10, 10)
    assert e.value.code == capi.E_NO_DEVICE and "cmi_slim_create" in str(e.value) and "no CPU fallback" in str(e.value)


def _conf(tmp_path, extra):
    shutil.copyfile(os.path.join(GOLDEN, "depaul_ratings_compact.csv"), tmp_path / "ratings.txt")
    conf = open(os.path.join(GOLDEN, "depaul_setting.conf")).read().replace("PLACEHOLDER_SET_BY_TEST", str(tmp_path / "ratings.txt"))
    lines = [ln for ln in conf.splitlines() if not ln.startswith(("recommender", "item.ranking", "num.max.iter", "SLIM"))]
    (tmp_path / "setting.conf").write_text("\n".join(lines + extra) + "\n")
    return str(tmp_path / "setting.conf")


def test_driver_knows_slim(tmp_path):
    """recommender=slim reaches the model, as a top-N run whatever item.ranking says: with a GPU the run ends with SLIM's ranking
    results, without one it stops at cmi_slim_create"""
    conf = _conf(tmp_path, ["recommender=SLIM", "item.ranking=off", "num.max.iter=2", "SLIM=-l1 1 -l2 1 -k 3", "similarity=cos", "num.shrinkage=30"])
    p = subprocess.run([EXE, "-c", conf], capture_output=True, text=True, timeout=300)
    assert "not on the accelerated path" not in p.stdout + p.stderr, p.stderr
    if capi.device_count() > 0:
        assert p.returncode == 0 and "Final Results by SLIM" in p.stdout and "Pre5" in p.stdout, p.stderr
    else:
        assert "cmi_slim_create" in p.stdout + p.stderr and "no HIP device" in p.stdout + p.stderr, (p.stdout, p.stderr)
    p = subprocess.run([EXE, "-c", _conf(tmp_path, ["recommender=slimx", "item.ranking=off"])], capture_output=True, text=True, timeout=300)
    out = p.stdout + p.stderr
    assert "not on the accelerated path" in out and " slim," in out and out.index(" slim,") < out.index("itemknn")


def test_driver_refuses_slim_shards(tmp_path):
    conf = _conf(tmp_path, ["recommender=SLIM", "item.ranking=on -topN 10"])
    p = subprocess.run([EXE, "-c", conf, "--shards", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "--shards 2 with slim" in p.stderr and "SLIM runs on one GPU" in p.stderr, p.stderr
    assert "Rating data set has been successfully loaded." not in p.stdout


def test_driver_refuses_diverse_ranking_with_slim(tmp_path):
    conf = _conf(tmp_path, ["recommender=SLIM", "item.ranking=on -topN 10 -diverse"])
    p = subprocess.run([EXE, "-c", conf], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "-diverse is not on the accelerated path" in p.stderr, p.stderr
    assert "Rating data set has been successfully loaded." not in p.stdout
