"""BPMF without a GPU: the C ABI symbols (header, binding table, library), the host's hyper-parameter step and moments against the
restatement and so the golden file (a start with a cached gaussian included), the argument checks that answer before any device call,
the no-device refusal, the sanitizer program over the host header, and the driver's entry and refusals."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from carskit_amd import capi
from tests import bpmf_ref as ref
from tests.util import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carskit_amd", "bin", "carskit-mi355x")
GOLDEN = os.path.join(ROOT, "tests", "golden")

SYMBOLS = ("cmi_bpmf_create", "cmi_bpmf_destroy", "cmi_bpmf_last_error", "cmi_bpmf_set_ratings", "cmi_bpmf_set_global_mean",
           "cmi_bpmf_get_global_mean", "cmi_bpmf_set_model", "cmi_bpmf_get_model", "cmi_bpmf_set_stream", "cmi_bpmf_get_stream",
           "cmi_bpmf_init_hyper", "cmi_bpmf_get_hyper", "cmi_bpmf_set_hyper", "cmi_bpmf_iterate", "cmi_bpmf_last_iter_ms",
           "cmi_bpmf_predict_batch", "cmi_bpmf_sample_side", "cmi_bpmf_gauss_attempts", "cmi_bpmf_moments", "cmi_bpmf_hyper_host")


def test_bpmf_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "carskit_mi355x.h")).read()
    assert sorted(set(re.findall(r"\b(cmi_bpmf_\w+)\(", header))) == sorted(SYMBOLS)
    assert "cmi_java_next_gaussians(" in header
    L = capi.lib()
    bound = {name for name, _, _ in capi.SYMBOLS}
    assert {n for n in bound if n.startswith("cmi_bpmf_")} == set(SYMBOLS) and "cmi_java_next_gaussians" in bound
    for s in SYMBOLS + ("cmi_java_next_gaussians",):
        assert getattr(L, s) is not None
    for m in ("set_ratings", "set_global_mean", "set_model", "model", "set_stream", "stream", "init_hyper", "hyper", "set_hyper", "iterate",
              "sample_side", "predict", "last_iter_ms", "close"):
        assert callable(getattr(capi.BPMFInstance, m))
    assert (capi.BPMF_MAX_K, capi.BPMF_TILE, capi.BPMF_CHUNK, capi.BPMF_GAUSS_BLOCK) == (64, 32, 64, 256)
    assert (capi.BPMF_BLOCK, capi.BPMF_STAGE_MIN) == (256, 1024)
    src = open(os.path.join(ROOT, "carskit_amd", "csrc", "bpmf_kernels.hpp")).read()
    for name, v in (("BPMF_MAX_K", 64), ("BPMF_TILE", 32), ("BPMF_CHUNK", 64), ("BPMF_GAUSS_BLOCK", 256), ("BPMF_BLOCK", 256),
                    ("BPMF_STAGE_MIN", 1024)):
        assert re.search(r"constexpr int %s = %d;" % (name, v), src), name


def test_argument_checks_answer_before_any_device_call():
    with pytest.raises(capi.CmiError) as e:
        capi.BPMFInstance(65, 10, 10)
    assert e.value.code == capi.E_UNSUPPORTED and "cmi_bpmf_create" in str(e.value) and "k <= 64" in str(e.value)
    for k, nu, ni, flags in ((0, 10, 10, 0), (4, 0, 10, 0), (4, 10, -1, 0), (4, 10, 10, 0x8)):
        with pytest.raises(capi.CmiError) as e:
            capi.BPMFInstance(k, nu, ni, flags=flags)
        assert e.value.code == capi.E_INVALID, (k, nu, ni, flags)
    L = capi.lib()
    assert L.cmi_bpmf_create(4, 10, 10, 0, 0, None) == capi.E_INVALID
    for call in (lambda: L.cmi_bpmf_iterate(None, None), lambda: L.cmi_bpmf_set_ratings(None, 0, None, None, None),
                 lambda: L.cmi_bpmf_set_model(None, None, None), lambda: L.cmi_bpmf_get_model(None, None, None),
                 lambda: L.cmi_bpmf_predict_batch(None, 0, None, None, 0, 0.0, 0.0, None), lambda: L.cmi_bpmf_last_iter_ms(None, None),
                 lambda: L.cmi_bpmf_init_hyper(None), lambda: L.cmi_bpmf_set_stream(None, 0, 0, 0.0),
                 lambda: L.cmi_bpmf_sample_side(None, 0, None, None, None, None),
                 lambda: L.cmi_bpmf_moments(None, 1, 1, None, None, 0), lambda: L.cmi_java_next_gaussians(None, None, None, 1, None),
                 lambda: L.cmi_bpmf_hyper_host(2, 5, None, None, None, None, None, None, None)):
        assert call() == capi.E_INVALID
    with pytest.raises(capi.CmiError) as e:
        capi.bpmf_moments(np.zeros((3, 65)), on_device=False)
    assert e.value.code == capi.E_UNSUPPORTED
    assert L.cmi_bpmf_destroy(None) == capi.OK


def test_bpmf_instance_without_device():
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(capi.CmiError) as e:
        capi.BPMFInstance(10, 10, 10)
    assert e.value.code == capi.E_NO_DEVICE and "cmi_bpmf_create" in str(e.value) and "no CPU fallback" in str(e.value)


def test_first_attempts_of_the_gaussian_stream():
    """the estimate the device starts from: 3 / 4 accepted (pi / 4 really) and three attempts of slack"""
    assert [capi.bpmf_gauss_attempts(p) for p in (1, 2, 3, 4, 30, 300)] == [4, 5, 7, 8, 43, 403]


@pytest.mark.parametrize("case", ref.golden()["cov"], ids=lambda c: c["name"])
def test_host_moments_equal_the_bytecode(case):
    X = ref.unhex(case["X"], case["rows"], case["k"])
    mean, cov = capi.bpmf_moments(X, on_device=False)
    assert same_bits(mean, ref.unhex(case["mean"], case["k"])) and same_bits(cov, ref.unhex(case["cov"], case["k"], case["k"]))


def _same_stream(a, b):
    """(state, have_cached, cached): the cached value counts only where there is one"""
    return a[0] == b[0] and bool(a[1]) == bool(b[1]) and (not a[1] or same_bits([a[2]], [b[2]]))


def _hyper_both(rows, X, alpha, mu, stream):
    """the C ABI's step beside the restatement's, from the same stream: ((alpha, mu, stream) of each)"""
    mean, cov = ref.column_mean(X), ref.cov(X)
    got = capi.bpmf_hyper_host(rows, mean, cov, alpha, mu, stream)
    r = ref.Stream(*stream)
    a, m = ref.hyper_side(r, X, np.array(alpha), np.array(mu))
    return got, (a, m, (r.state, r.have, r.cached if r.have else 0.0))


@pytest.mark.parametrize("run", ref.golden()["runs"], ids=lambda r: "%s-k%d" % (r["name"], r["k"]))
def test_hyper_host_equals_the_restatement_on_the_golden_runs(run):
    """the two hyper steps of the first iteration of every golden run (whose P, Q and loss after it pin the restatement's step to the
    reference, tests/test_bpmf_ref.py), and a second pair from the state that leaves.  (A step takes k^2 + k gaussians, an even number:
    a cached value at the start comes from a Gibbs pass only, as in the next test.)"""
    nu, ni, k = run["n_users"], run["n_items"], run["k"]
    P, Q = ref.unhex(run["P0"], nu, k), ref.unhex(run["Q0"], ni, k)
    m = ref.BPMF(nu, ni, ref.golden_cells(run), float.fromhex(run["global_mean"]))
    hy = m.init_hyper(P, Q)
    stream = (ref.random_state(run["seed_gibbs"]), False, 0.0)
    for rep in range(2):
        for X, a, mu in ((P, "alpha_u", "mu_u"), (Q, "alpha_m", "mu_m")):
            got, want = _hyper_both(X.shape[0], X, hy[a], hy[mu], stream)
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (rep, a)
            assert _same_stream(got[2], want[2]), (rep, a)
            hy[a], hy[mu], stream = want[0], want[1], want[2]


def test_hyper_host_from_a_cached_gaussian_and_a_null_wishart_scale():
    rng = np.random.default_rng(20261221)
    X = rng.standard_normal((9, 3))
    r = ref.Stream.seeded(77)
    r.gaussian()
    assert r.have
    got, want = _hyper_both(9, X, np.eye(3), np.zeros(3), (r.state, True, r.cached))
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and _same_stream(got[2], want[2])
    # a NaN in the factor matrix: cov() is NaN in that column, the Wishart scale has no factor, alpha keeps its value and only mu is drawn
    X[4, 1] = np.nan
    got, want = _hyper_both(9, X, np.eye(3) * 2.0, np.zeros(3), (r.state, True, r.cached))
    assert same_bits(got[0], np.eye(3) * 2.0) and same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and _same_stream(got[2], want[2])


@pytest.mark.parametrize("k", [5, 33, 64])
def test_hyper_host_at_the_sizes_the_golden_runs_do_not_reach(k):
    """k = 5 is the first size at which wishart()'s SparseVector.inner leaves out a term; 33 and 64 are past every golden run"""
    rng = np.random.default_rng(20261223 + k)
    X = rng.standard_normal((k + 20, k))
    alpha = ref.inv(ref.cov(X))
    got, want = _hyper_both(k + 20, X, alpha, ref.column_mean(X), (ref.random_state(k), False, 0.0))
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and _same_stream(got[2], want[2])
    assert not same_bits(got[0], alpha)                     # the Wishart draw replaced alpha


def test_host_check_program_runs_clean_under_sanitizers(tmp_path):
    """tests/tools/bpmf_host_check.cpp: the host header in a stand-alone program under ASan and UBSan (CPU only)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc: the host header shares java_math.hpp with the device"
    exe = str(tmp_path / "bpmf_host_check")
    subprocess.run([hipcc, "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "carskit_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "bpmf_host_check.cpp"), "-o", exe], check=True, timeout=600)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "bpmf host checks passed" in p.stdout, p.stdout + p.stderr


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
def _conf(tmp_path, extra):
    shutil.copyfile(os.path.join(GOLDEN, "depaul_ratings_compact.csv"), tmp_path / "ratings.txt")
    conf = open(os.path.join(GOLDEN, "depaul_setting.conf")).read().replace("PLACEHOLDER_SET_BY_TEST", str(tmp_path / "ratings.txt"))
    lines = [ln for ln in conf.splitlines() if not ln.startswith(("recommender", "item.ranking", "num.max.iter"))]
    (tmp_path / "setting.conf").write_text("\n".join(lines + extra) + "\n")
    return str(tmp_path / "setting.conf")


def test_driver_knows_bpmf(tmp_path):
    """recommender=bpmf reaches the model: with a GPU the run ends with BPMF's rating results, without one it stops at cmi_bpmf_create"""
    conf = _conf(tmp_path, ["recommender=bpmf", "item.ranking=off", "num.max.iter=2", "num.factors=4"])
    p = subprocess.run([EXE, "-c", conf], capture_output=True, text=True, timeout=300)
    assert "not on the accelerated path" not in p.stdout + p.stderr, p.stderr
    if capi.device_count() > 0:
        assert p.returncode == 0 and "Final Results by BPMF" in p.stdout and "RMSE" in p.stdout, p.stderr
    else:
        assert "cmi_bpmf_create" in p.stdout + p.stderr and "no HIP device" in p.stdout + p.stderr, (p.stdout, p.stderr)
    p = subprocess.run([EXE, "-c", _conf(tmp_path, ["recommender=bpmfx", "item.ranking=off"])], capture_output=True, text=True, timeout=300)
    assert "not on the accelerated path" in p.stdout + p.stderr and " bpmf," in p.stdout + p.stderr


def test_driver_refuses_bpmf_shards_and_ranking(tmp_path):
    conf = _conf(tmp_path, ["recommender=bpmf", "item.ranking=off"])
    p = subprocess.run([EXE, "-c", conf, "--shards", "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "--shards 2 with bpmf" in p.stderr and "BPMF runs on one GPU" in p.stderr, p.stderr
    conf = _conf(tmp_path, ["recommender=bpmf", "item.ranking=on -topN 10"])
    p = subprocess.run([EXE, "-c", conf], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "item.ranking=on with bpmf" in p.stderr, p.stderr
    assert "Rating data set has been successfully loaded." not in p.stdout
