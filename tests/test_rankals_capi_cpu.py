"""RankALS without a GPU: the C ABI symbols (header, binding table, library), the argument checks that answer before any device call,
the no-device refusal, the host class's initModel() against the reference's own draw, Conf's RankALS=-sw, the factory entry and the
driver's refusals (decided before any data or device work)."""
import os
import re
import shutil
import subprocess

import pytest

from carskit_amd import capi
from tests import rankals_ref as rref
from tests.util import same_bits_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carskit_amd", "bin", "carskit-mi355x")
GOLDEN = os.path.join(ROOT, "tests", "golden")

SYMBOLS = ("cmi_rankals_create", "cmi_rankals_destroy", "cmi_rankals_last_error", "cmi_rankals_set_ratings", "cmi_rankals_set_model",
           "cmi_rankals_get_model", "cmi_rankals_iterate", "cmi_rankals_predict_batch", "cmi_rankals_eval_rankings",
           "cmi_rankals_last_iter_ms", "cmi_rankals_invert")


def test_rankals_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "carskit_mi355x.h")).read()
    assert sorted(set(re.findall(r"\b(cmi_rankals_\w+)\(", header))) == sorted(SYMBOLS)
    L = capi.lib()
    bound = {name for name, _, _ in capi.SYMBOLS}
    assert {n for n in bound if n.startswith("cmi_rankals_")} == set(SYMBOLS)
    for s in SYMBOLS:
        assert getattr(L, s) is not None
    assert L.cmi_abi_version() == 5
    for m in ("set_ratings", "set_model", "model", "iterate", "predict", "eval_rankings", "last_iter_ms", "invert", "close"):
        assert callable(getattr(capi.RankALSInstance, m))


def test_argument_checks_answer_before_any_device_call():
    """k = 65 and the null / non-positive arguments are refused whether or not a device is visible"""
    with pytest.raises(capi.CmiError) as e:
        capi.RankALSInstance(65, 10, 10)
    assert e.value.code == capi.E_UNSUPPORTED and "cmi_rankals_create" in str(e.value) and "k <= 64" in str(e.value)
    for k, nu, ni in ((0, 10, 10), (4, 0, 10), (4, 10, -1)):
        with pytest.raises(capi.CmiError) as e:
            capi.RankALSInstance(k, nu, ni)
        assert e.value.code == capi.E_INVALID, (k, nu, ni)
    L = capi.lib()
    assert L.cmi_rankals_create(4, 10, 10, 0, 0, None) == capi.E_INVALID
    for call in (lambda: L.cmi_rankals_iterate(None, 1), lambda: L.cmi_rankals_set_ratings(None, 0, None, None, None),
                 lambda: L.cmi_rankals_set_model(None, None, None), lambda: L.cmi_rankals_get_model(None, None, None),
                 lambda: L.cmi_rankals_predict_batch(None, 0, None, None, None), lambda: L.cmi_rankals_last_iter_ms(None, None),
                 lambda: L.cmi_rankals_invert(None, 0, 2, None, None)):
        assert call() == capi.E_INVALID
    assert L.cmi_rankals_destroy(None) == capi.OK


def test_rankals_instance_without_device():
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(capi.CmiError) as e:
        capi.RankALSInstance(10, 10, 10)
    assert e.value.code == capi.E_NO_DEVICE and "cmi_rankals_create" in str(e.value) and "no CPU fallback" in str(e.value)


HOST_PROBE = r"""
#include <cstdio>
#include "recommender.hpp"
using namespace carskit;
int main(int argc, char **argv) {
    FileConfiger cf(argv[1]);
    Conf c(cf);
    printf("sw %d set %d ranking %d\n", (int)c.rankalsSw, (int)c.rankalsSet, (int)c.isRankingPred);
    RatingData d;
    d.n_users = NU, d.n_items = NI;
    d.u = {0}, d.j = {0}, d.ctx = {0}, d.r = {1.0};
    RankALS m(d, d, 0, c);
    try {
        m.initModel();
    } catch (const std::exception &e) {
        printf("initModel: %s\n", e.what());
        return 0;
    }
    for (double x : m.P) printf("P %a\n", x);
    for (double x : m.Q) printf("Q %a\n", x);
    return 0;
}
"""


@pytest.fixture(scope="module")
def host_probe(tmp_path_factory):
    """a stand-alone program over the host classes' header: Conf from a setting file, then RankALS::initModel()"""
    g = rref.golden()["init"]
    d = tmp_path_factory.mktemp("rankals_probe")
    (d / "probe.cpp").write_text(HOST_PROBE.replace("NU", str(g["n_users"])).replace("NI", str(g["n_items"])))
    exe = str(d / "probe")
    subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "carskit_amd", "csrc", "host"), str(d / "probe.cpp"),
                    "-L" + os.path.join(ROOT, "carskit_amd", "lib"), "-lcarskit_mi355x",
                    "-Wl,-rpath," + os.path.join(ROOT, "carskit_amd", "lib"), "-o", exe], check=True, timeout=300)

    def run(lines):
        (d / "s.conf").write_text("\n".join(lines) + "\n")
        return subprocess.run([exe, str(d / "s.conf")], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    return run


def test_host_init_model_equals_the_reference_draw(host_probe):
    g = rref.golden()["init"]
    nu, ni, k = g["n_users"], g["n_items"], g["k"]
    out = host_probe(["num.factors=%d" % k, "evaluation.setup=cv -k 5 --rand-seed %d" % g["seed"], "RankALS=-sw on"])
    assert out[0] == "sw 1 set 1 ranking 0"            # item.ranking is absent: the class, not Conf, turns ranking on
    P = [float.fromhex(ln.split()[1]) for ln in out if ln.startswith("P ")]
    Q = [float.fromhex(ln.split()[1]) for ln in out if ln.startswith("Q ")]
    assert same_bits_exact(P, rref.unhex(g["P"], nu * k)) and same_bits_exact(Q, rref.unhex(g["Q"], ni * k))


def test_conf_reads_the_support_weight_switch(host_probe):
    assert host_probe(["RankALS=-sw off"])[0].startswith("sw 0 set 1")
    assert host_probe(["RankALS=-sw true"])[0].startswith("sw 1 set 1")
    assert host_probe(["RankALS=-x 1"])[0].startswith("sw 0 set 1")
    out = host_probe(["num.factors=2"])                # no RankALS key: the reference's algoOptions is null and initModel fails on it
    assert out[0].startswith("sw 0 set 0") and out[1].startswith("initModel: null (RankALS is not set")


def _conf(tmp_path, extra, threshold="0"):
    shutil.copyfile(os.path.join(GOLDEN, "depaul_ratings_compact.csv"), tmp_path / "ratings.txt")
    conf = open(os.path.join(GOLDEN, "depaul_setting.conf")).read().replace("PLACEHOLDER_SET_BY_TEST", str(tmp_path / "ratings.txt"))
    conf = conf.replace("-threshold -1", "-threshold " + threshold)
    lines = [ln for ln in conf.splitlines() if not ln.startswith(("recommender", "item.ranking", "num.max.iter"))]
    (tmp_path / "setting.conf").write_text("\n".join(lines + extra) + "\n")
    return str(tmp_path / "setting.conf")


def test_driver_knows_rankals(tmp_path):
    """recommender=rankals reaches the model, as a top-N run whatever item.ranking says: with a GPU the run ends with RankALS's ranking
    results, without one it stops at cmi_rankals_create"""
    conf = _conf(tmp_path, ["recommender=RankALS", "item.ranking=off", "num.max.iter=3", "RankALS=-sw on"])
    p = subprocess.run([EXE, "-c", conf], capture_output=True, text=True, timeout=300)
    assert "not on the accelerated path" not in p.stdout + p.stderr, p.stderr
    if capi.device_count() > 0:
        assert p.returncode == 0 and "Final Results by RankALS" in p.stdout and "Pre5" in p.stdout, p.stderr
    else:
        assert "cmi_rankals_create" in p.stdout + p.stderr and "no HIP device" in p.stdout + p.stderr, (p.stdout, p.stderr)
    p = subprocess.run([EXE, "-c", _conf(tmp_path, ["recommender=rankalsx", "item.ranking=off"])], capture_output=True, text=True, timeout=300)
    out = p.stdout + p.stderr
    assert "not on the accelerated path" in out and " rankals," in out


def test_driver_refuses_rankals_shards(tmp_path):
    conf = _conf(tmp_path, ["recommender=RankALS", "item.ranking=on -topN 10", "RankALS=-sw on"])
    p = subprocess.run([EXE, "-c", conf, "--shards", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "--shards 2 with rankals" in p.stderr and "RankALS runs on one GPU" in p.stderr, p.stderr
    assert "Rating data set has been successfully loaded." not in p.stdout


def test_driver_refuses_unbinarized_ratings_in_the_references_words(tmp_path):
    """checkBinary() (Recommender.java:1154-1160): val.binary.threshold < 0"""
    conf = _conf(tmp_path, ["recommender=RankALS", "item.ranking=off", "RankALS=-sw on"], threshold="-1")
    p = subprocess.run([EXE, "-c", conf], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0, p.stdout
    assert "val.binary.threshold=-1.0, ratings must be binarized first! Try set a non-negative value." in p.stderr, p.stderr
    # the threshold is a Java float printed by Float.toString: -0.1f is "-0.1" (not the double it widens to), -0.0005f is "-5.0E-4"
    for given, printed in (("-0.1", "-0.1"), ("-2.5", "-2.5"), ("-0.0005", "-5.0E-4"), ("-12345678", "-1.2345678E7")):
        conf = _conf(tmp_path, ["recommender=RankALS", "item.ranking=off", "RankALS=-sw on"], threshold=given)
        p = subprocess.run([EXE, "-c", conf], capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and "val.binary.threshold=%s, ratings must be binarized first!" % printed in p.stderr, (given, p.stderr)
