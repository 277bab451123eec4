"""NMF without a GPU: the C ABI symbols (header, binding table, library), the no-device refusal, the factory entry, and the driver's
refusals (decided before any data or device work)."""
import os
import re
import shutil
import subprocess

import pytest

from carskit_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carskit_amd", "bin", "carskit-mi355x")
GOLDEN = os.path.join(ROOT, "tests", "golden")

NMF_SYMBOLS = ("cmi_nmf_create", "cmi_nmf_destroy", "cmi_nmf_last_error", "cmi_nmf_set_ratings", "cmi_nmf_set_model",
               "cmi_nmf_get_model", "cmi_nmf_iterate", "cmi_nmf_predict_batch", "cmi_nmf_last_iter_ms")


def test_nmf_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "carskit_mi355x.h")).read()
    assert sorted(set(re.findall(r"\b(cmi_nmf_\w+)\(", header))) == sorted(NMF_SYMBOLS)
    L = capi.lib()
    bound = {name for name, _, _ in capi.SYMBOLS}
    assert {n for n in bound if n.startswith("cmi_nmf_")} == set(NMF_SYMBOLS)
    for s in NMF_SYMBOLS:
        assert getattr(L, s) is not None
    assert L.cmi_abi_version() == 5
    for m in ("set_ratings", "set_model", "model", "iterate", "predict", "last_iter_ms", "close"):
        assert callable(getattr(capi.NMFInstance, m))


def test_nmf_instance_without_device():
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(capi.CmiError) as e:
        capi.NMFInstance(10, 10, 10)
    assert e.value.code == capi.E_NO_DEVICE and "cmi_nmf_create" in str(e.value) and "no CPU fallback" in str(e.value)


def _conf(tmp_path, extra):
    shutil.copyfile(os.path.join(GOLDEN, "depaul_ratings_compact.csv"), tmp_path / "ratings.txt")
    conf = open(os.path.join(GOLDEN, "depaul_setting.conf")).read().replace("PLACEHOLDER_SET_BY_TEST", str(tmp_path / "ratings.txt"))
    lines = [ln for ln in conf.splitlines() if not ln.startswith(("recommender", "item.ranking", "num.max.iter"))]
    (tmp_path / "setting.conf").write_text("\n".join(lines + extra) + "\n")
    return str(tmp_path / "setting.conf")


def test_driver_knows_nmf(tmp_path):
    """recommender=nmf reaches the model: with a GPU the run ends with NMF's results, without one it stops at cmi_nmf_create"""
    conf = _conf(tmp_path, ["recommender=NMF", "item.ranking=off", "num.max.iter=2"])
    p = subprocess.run([EXE, "-c", conf], capture_output=True, text=True, timeout=300)
    assert "not on the accelerated path" not in p.stdout + p.stderr, p.stderr
    if capi.device_count() > 0:
        assert p.returncode == 0 and "Final Results by NMF" in p.stdout, p.stderr
    else:
        assert "cmi_nmf_create" in p.stdout + p.stderr and "no HIP device" in p.stdout + p.stderr, (p.stdout, p.stderr)
    p = subprocess.run([EXE, "-c", _conf(tmp_path, ["recommender=nmfx", "item.ranking=off"])], capture_output=True, text=True, timeout=300)
    assert "not on the accelerated path" in p.stdout + p.stderr and "slopeone, nmf)" in p.stdout + p.stderr


def test_driver_refuses_nmf_top_n(tmp_path):
    conf = _conf(tmp_path, ["recommender=NMF", "item.ranking=on -topN 10"])
    p = subprocess.run([EXE, "-c", conf], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "item.ranking=on with nmf" in p.stderr and "top-N recommendation of NMF is not accelerated yet" in p.stderr, p.stderr
    assert "Rating data set has been successfully loaded." not in p.stdout


def test_driver_refuses_nmf_shards(tmp_path):
    conf = _conf(tmp_path, ["recommender=NMF", "item.ranking=off"])
    p = subprocess.run([EXE, "-c", conf, "--shards", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "--shards 2 with nmf" in p.stderr and "NMF runs on one GPU" in p.stderr, p.stderr
    assert "Rating data set has been successfully loaded." not in p.stdout
