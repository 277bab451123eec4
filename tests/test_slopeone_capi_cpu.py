"""SlopeOne without a GPU: the C ABI symbols, the no-device refusal, and the driver's refusals (decided before any data or device
work)."""
import os
import shutil
import subprocess

import pytest

from carskit_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carskit_amd", "bin", "carskit-mi355x")
GOLDEN = os.path.join(ROOT, "tests", "golden")

SLOPE_SYMBOLS = ("cmi_slope_create", "cmi_slope_destroy", "cmi_slope_last_error", "cmi_slope_set_ratings", "cmi_slope_build",
                 "cmi_slope_get_deviation", "cmi_slope_predict_batch", "cmi_slope_last_build_ms")


def test_slope_symbols_load():
    L = capi.lib()
    bound = {name for name, _, _ in capi.SYMBOLS}
    for s in SLOPE_SYMBOLS:
        assert s in bound and getattr(L, s) is not None
    assert L.cmi_abi_version() == 5


def test_slope_instance_without_device():
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(capi.CmiError) as e:
        capi.SlopeOneInstance(10, 10)
    assert e.value.code == capi.E_NO_DEVICE and "no CPU fallback" in str(e.value)


def _conf(tmp_path, extra):
    shutil.copyfile(os.path.join(GOLDEN, "depaul_ratings_compact.csv"), tmp_path / "ratings.txt")
    conf = open(os.path.join(GOLDEN, "depaul_setting.conf")).read().replace("PLACEHOLDER_SET_BY_TEST", str(tmp_path / "ratings.txt"))
    lines = [ln for ln in conf.splitlines() if not ln.startswith(("recommender", "item.ranking"))]
    (tmp_path / "setting.conf").write_text("\n".join(lines + extra) + "\n")
    return str(tmp_path / "setting.conf")


def test_driver_refuses_slopeone_top_n(tmp_path):
    conf = _conf(tmp_path, ["recommender=SlopeOne", "item.ranking=on -topN 10"])
    p = subprocess.run([EXE, "-c", conf], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "item.ranking=on with slopeone" in p.stderr and "not accelerated yet" in p.stderr, p.stderr
    assert "Rating data set has been successfully loaded." not in p.stdout


def test_driver_refuses_slopeone_shards(tmp_path):
    conf = _conf(tmp_path, ["recommender=SlopeOne", "item.ranking=off"])
    p = subprocess.run([EXE, "-c", conf, "--shards", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "--shards 2 with slopeone" in p.stderr, p.stderr
    assert "Rating data set has been successfully loaded." not in p.stdout
