"""RankSGD without a GPU: the C ABI symbols (header, binding table, library), the refusals that answer before any device call, and the
host-only entry points against tests/ranksgd_ref.py and the golden file: the item list, the tries, the walk that assigns them."""
import math
import os
import re

import numpy as np
import pytest

from carskit_amd import capi
from tests import ranksgd_ref as rr
from tests.util import same_bits_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = capi.RANKSGD_FLAG_NUM_RATES_SIZE

SYMBOLS = ("cmi_ranksgd_create", "cmi_ranksgd_destroy", "cmi_ranksgd_last_error", "cmi_ranksgd_set_ratings", "cmi_ranksgd_set_model",
           "cmi_ranksgd_get_model", "cmi_ranksgd_set_random_state", "cmi_ranksgd_get_random_state", "cmi_ranksgd_sample",
           "cmi_ranksgd_iterate", "cmi_ranksgd_predict_batch", "cmi_ranksgd_eval_rankings", "cmi_ranksgd_last_iter_ms",
           "cmi_ranksgd_last_schedule", "cmi_ranksgd_item_table", "cmi_ranksgd_tries", "cmi_ranksgd_assign_host",
           "cmi_ranksgd_sample_host")


def cols(cells):
    return ([c[0] for c in cells], [c[1] for c in cells], [c[2] for c in cells])


def flags_of(run):
    return SIZE if run["num_rates"] == rr.NUM_RATES_SIZE else 0


def table_3():
    return [4, 9, 2], [0.125, 0.5, 1.0]


def table_1000():
    """1 000 items, many equal probabilities (ties in the sums' steps, none in the sums)"""
    probs = np.repeat(np.arange(1, 11), 100).astype(np.float64)
    probs /= probs.sum()
    cum, s = [], 0.0
    for p in probs.tolist():
        s += p
        cum.append(s)
    return list(range(999, -1, -1)), cum


def table_half():
    """the last sum is 0.5: half the tries find no entry"""
    return [3, 1, 8, 6], [0.0625, 0.125, 0.375, 0.5]


TABLES = {"three": table_3, "thousand": table_1000, "half": table_half}


def test_ranksgd_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "carskit_mi355x.h")).read()
    assert sorted(set(re.findall(r"\b(cmi_ranksgd_\w+)\(", header))) == sorted(SYMBOLS)
    L = capi.lib()
    bound = {name for name, _, _ in capi.SYMBOLS}
    assert {n for n in bound if n.startswith("cmi_ranksgd_")} == set(SYMBOLS)
    for s in SYMBOLS:
        assert getattr(L, s) is not None
    assert L.cmi_abi_version() == 5
    for m in ("set_ratings", "set_model", "model", "set_random_state", "random_state", "sample", "iterate", "predict", "eval_rankings",
              "last_iter_ms", "last_schedule", "close"):
        assert callable(getattr(capi.RankSGDInstance, m))


def test_argument_checks_answer_before_any_device_call():
    with pytest.raises(capi.CmiError) as e:
        capi.RankSGDInstance(129, 10, 10)
    assert e.value.code == capi.E_UNSUPPORTED and "cmi_ranksgd_create" in str(e.value) and "k <= 128" in str(e.value)
    for k, nu, ni, flags in ((0, 10, 10, 0), (4, 0, 10, 0), (4, 10, -1, 0), (4, 10, 10, 0x100)):
        with pytest.raises(capi.CmiError) as e:
            capi.RankSGDInstance(k, nu, ni, flags=flags)
        assert e.value.code == capi.E_INVALID, (k, nu, ni, flags)
    L = capi.lib()
    assert L.cmi_ranksgd_create(4, 10, 10, 0, 0, None) == capi.E_INVALID
    for call in (lambda: L.cmi_ranksgd_iterate(None, 0.1, None), lambda: L.cmi_ranksgd_set_ratings(None, 0, None, None, None),
                 lambda: L.cmi_ranksgd_set_model(None, None, None), lambda: L.cmi_ranksgd_get_model(None, None, None),
                 lambda: L.cmi_ranksgd_predict_batch(None, 0, None, None, None), lambda: L.cmi_ranksgd_last_iter_ms(None, None),
                 lambda: L.cmi_ranksgd_last_schedule(None, None), lambda: L.cmi_ranksgd_sample(None, 0, 0, None, None, None, None, None),
                 lambda: L.cmi_ranksgd_set_random_state(None, 0), lambda: L.cmi_ranksgd_get_random_state(None, None)):
        assert call() == capi.E_INVALID
    assert L.cmi_ranksgd_destroy(None) == capi.OK
    with pytest.raises(capi.CmiError) as e:
        capi.ranksgd_tries(1 << 48, [1], [1.0], 4)
    assert e.value.code == capi.E_INVALID
    with pytest.raises(capi.CmiError) as e:
        capi.ranksgd_tries(1, [1, 2], [0.5, 0.25], 4)                       # sums that decrease
    assert e.value.code == capi.E_INVALID
    with pytest.raises(capi.CmiError) as e:
        capi.ranksgd_item_table(2, 3, [0, 2], [0, 1], [1.0, 1.0])
    assert e.value.code == capi.E_INVALID and "out of range" in str(e.value)


def test_ranksgd_instance_without_device():
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(capi.CmiError) as e:
        capi.RankSGDInstance(10, 10, 10)
    assert e.value.code == capi.E_NO_DEVICE and "cmi_ranksgd_create" in str(e.value) and "no CPU fallback" in str(e.value)


def test_item_table_equals_the_golden_lists():
    gd = rr.golden()
    for run in rr.golden_runs():
        item, cum = capi.ranksgd_item_table(run["n_users"], run["n_items"], *cols(run["cells"]), flags=flags_of(run))
        _, _, rcum = rr.item_table(run["n_users"], run["n_items"], run["cells"], run["num_rates"])
        assert item.tolist() == run["items"] and same_bits_exact(cum, rcum), run["name"]
        assert same_bits_exact(cum[:1], run["probs"][:1])
    for lst in gd["lists"]:                                                 # the reference as it stands: HashMap order, sums +Infinity
        cells = next((r["cells"] for r in rr.golden_runs() if r["name"].startswith(lst["name"])), None)
        assert cells is not None
        item, cum = capi.ranksgd_item_table(lst["n_users"], lst["n_items"], *cols(cells))
        assert item.tolist() == lst["items"] and all(c == math.inf for c in cum.tolist()), lst["name"]


def test_item_table_on_ids_past_65535_equals_the_restatement():
    """3 x 70 000, a dozen cells: Integer.hashCode() spreads ids above 65 535 (h ^ h >>> 16), and equal counts keep HashMap order"""
    ids = [5, 65536, 65537, 69999, 16, 32, 65552, 21, 40000, 66000, 3, 131]
    cells = [(n % 3, j, 1.0 + n % 4) for n, j in enumerate(ids)] + [(1, 5, 2.0), (2, 65536, 3.0), (0, 40000, 0.0)]
    for flags, nr in ((SIZE, rr.NUM_RATES_SIZE), (0, rr.NUM_RATES_REFERENCE)):
        item, cum = capi.ranksgd_item_table(3, 70000, *cols(cells), flags=flags)
        ritem, _, rcum = rr.item_table(3, 70000, cells, nr)
        assert item.tolist() == ritem and same_bits_exact(cum, rcum)
        assert ritem != sorted(ritem) and len(ritem) == 12


@pytest.mark.parametrize("name", sorted(TABLES))
def test_host_tries_equal_the_restatement(name):
    item, cum = TABLES[name]()
    st = rr.random_state(20270310)
    got = capi.ranksgd_tries(st, item, cum, 5000).tolist()
    rnd = rr.JavaStream(st)
    want = [rr.try_item(rnd, item, cum) for _ in range(5000)]
    assert got == want
    assert (-1 in got) == (name == "half")
    if name == "half":
        assert 2200 < got.count(-1) < 2800
    if name == "thousand":
        assert len(set(got)) > 900


def test_assign_host_rules():
    five = [(0, j, 1.0) for j in (10, 11, 12, 13, 14)]
    js, used = capi.ranksgd_assign_host(1, 20, *cols(five), [14, 12, 14, 10, 3, 14, 14, 11, 9])
    assert js.tolist() == [14, 14, 3, 14, 14] and used == 7                 # contains() misses the rated item 14; j == i on its own cell
    cells = [(0, 1, 1.0), (0, 2, 2.0), (0, 3, 3.0), (1, 4, 0.0), (2, 5, 1.0)]
    tries = [1, -1, 7, 0, 2, 4, 5, -1, 6]
    js, used = capi.ranksgd_assign_host(3, 9, *cols(cells), tries)
    assert js.tolist() == [7, 0, 4, 6] and used == 9                        # -1 after a rejection: one more rejection
    rows = [[1, 2, 3], [], [5]]
    assert (js.tolist(), used) == rr.assign(rows, tries)
    with pytest.raises(capi.CmiError) as e:
        capi.ranksgd_assign_host(3, 9, *cols(cells), [7, -1, 3])
    assert e.value.code == capi.E_NUMERIC and "predict(u, -1)" in str(e.value) and "cell 1" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        capi.ranksgd_assign_host(3, 9, *cols(cells), [7, 0])
    assert e.value.code == capi.E_UNSUPPORTED
    with pytest.raises(capi.CmiError) as e:
        capi.ranksgd_assign_host(3, 9, *cols(cells), [7, 9])
    assert e.value.code == capi.E_INVALID


def test_assign_host_equals_the_restatement_on_random_tries():
    rng = np.random.default_rng(20270311)
    cells = [(u, int(j), float(1 + (u + j) % 5)) for u in range(40) for j in rng.choice(50, size=1 + (u * 5) % 13, replace=False)]
    rows = [sorted(j for uu, j, _ in cells if uu == u) for u in range(40)]
    tries = rng.integers(-1, 50, 4000).tolist()
    tries[0] = 49 if 49 not in rows[0] else next(j for j in range(50) if j not in rows[0])
    try:
        want = rr.assign(rows, tries)
    except rr.FirstTryMiss:
        want = None
    if want is None:
        with pytest.raises(capi.CmiError):
            capi.ranksgd_assign_host(40, 50, *cols(cells), tries)
    else:
        js, used = capi.ranksgd_assign_host(40, 50, *cols(cells), tries)
        assert (js.tolist(), used) == want


def test_host_sampler_equals_the_golden_samples():
    for run in rr.golden_runs():
        st = rr.random_state(run["seed"])
        for it in run["iters"]:
            u, i, j, r, st, used = capi.ranksgd_sample_host(run["n_users"], run["n_items"], *cols(run["cells"]), st, flags=flags_of(run))
            nz = sorted((c[0], c[1], c[2]) for c in run["cells"] if c[2] != 0.0)
            assert list(zip(u.tolist(), i.tolist(), r.tolist())) == nz
            assert j.tolist() == it["j"] and st == it["state"] and used == len(it["randoms"]), run["name"]


def test_host_refusals():
    """what the reference cannot finish is refused with E_INVALID"""
    handmade = next(r for r in rr.golden_runs() if r["name"].startswith("handmade"))
    with pytest.raises(capi.CmiError) as e:                                 # the reference as it stands: every draw returns item 0
        capi.ranksgd_sample_host(handmade["n_users"], handmade["n_items"], *cols(handmade["cells"]), 1)
    assert e.value.code == capi.E_INVALID and "user 0 holds every item a draw can return" in str(e.value)
    assert "never assigns numRates" in str(e.value) and "item 0" in str(e.value)
    full = [(0, 0, 1.0), (1, 0, 2.0), (1, 1, 3.0)]                          # user 1 holds both items of the list
    with pytest.raises(capi.CmiError) as e:
        capi.ranksgd_sample_host(2, 3, *cols(full), 1, flags=SIZE)
    assert e.value.code == capi.E_INVALID and "user 1 holds every item" in str(e.value) and "numRates" not in str(e.value)
    full[2] = (1, 1, 0.0)                                                   # a stored zero is not held, and not in the list either
    with pytest.raises(capi.CmiError) as e:
        capi.ranksgd_sample_host(2, 3, *cols(full), 1, flags=SIZE)
    assert "user 0 holds every item" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        capi.ranksgd_sample_host(2, 3, [0], [1], [0.0], 1, flags=SIZE)
    assert e.value.code == capi.E_INVALID and "no non-zero cell" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        capi.ranksgd_sample_host(2, 3, [0, 0], [1, 1], [1.0, 2.0], 1, flags=SIZE)
    assert e.value.code == capi.E_INVALID and "duplicate cell" in str(e.value)


def test_host_check_program_runs_clean_under_sanitizers(tmp_path):
    """tests/tools/ranksgd_host_check.cpp: the list, the tries and the walk in a stand-alone program under ASan and UBSan (CPU only)"""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc: the host header shares functions with the device")
    exe = str(tmp_path / "ranksgd_host_check")
    subprocess.run([hipcc, "--offload-host-only", "-x", "hip", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "carskit_amd", "csrc"),
                    os.path.join(ROOT, "tests", "tools", "ranksgd_host_check.cpp"), "-o", exe], check=True, timeout=600)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "ranksgd host checks passed" in p.stdout, p.stdout + p.stderr


# ---- the driver ------------------------------------------------------------------------------------------------------------------
EXE = os.path.join(ROOT, "carskit_amd", "bin", "carskit-mi355x")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _conf(tmp_path, extra, threshold="0"):
    import shutil
    shutil.copyfile(os.path.join(GOLDEN, "depaul_ratings_compact.csv"), tmp_path / "ratings.txt")
    conf = open(os.path.join(GOLDEN, "depaul_setting.conf")).read().replace("PLACEHOLDER_SET_BY_TEST", str(tmp_path / "ratings.txt"))
    conf = conf.replace("-threshold -1", "-threshold " + threshold)
    lines = [ln for ln in conf.splitlines() if not ln.startswith(("recommender", "item.ranking", "num.max.iter"))]
    (tmp_path / "setting.conf").write_text("\n".join(lines + extra) + "\n")
    return str(tmp_path / "setting.conf")


def test_driver_knows_ranksgd(tmp_path):
    """recommender=ranksgd reaches the model, as a top-N run whatever item.ranking says: with a GPU and RankSGD=-numrates size the run
    ends with RankSGD's ranking results, without one it stops at cmi_ranksgd_create"""
    import subprocess
    p = subprocess.run([EXE, "-c", _conf(tmp_path, ["recommender=RankSGD", "item.ranking=off", "num.max.iter=2", "RankSGD=-numrates size"])],
                       capture_output=True, text=True, timeout=300)
    assert "not on the accelerated path" not in p.stdout + p.stderr, p.stderr
    if capi.device_count() > 0:
        assert p.returncode == 0 and "Final Results by RankSGD" in p.stdout and "Pre5" in p.stdout, p.stderr
    else:
        assert "cmi_ranksgd_create" in p.stdout + p.stderr and "no HIP device" in p.stdout + p.stderr, (p.stdout, p.stderr)
    p = subprocess.run([EXE, "-c", _conf(tmp_path, ["recommender=ranksgdx", "item.ranking=off"])], capture_output=True, text=True, timeout=300)
    assert "not on the accelerated path" in p.stdout + p.stderr and " ranksgd," in p.stdout + p.stderr
    p = subprocess.run([EXE, "-c", _conf(tmp_path, ["recommender=ranksgd", "RankSGD=-numrates half"])], capture_output=True, text=True, timeout=300)
    assert p.returncode == 1 and "RankSGD=-numrates half: size or reference" in p.stderr, p.stderr


def test_driver_refuses_ranksgd_shards_and_a_negative_threshold(tmp_path):
    import subprocess
    p = subprocess.run([EXE, "-c", _conf(tmp_path, ["recommender=RankSGD", "item.ranking=on -topN 10"]), "--shards", "2"], capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 1 and "--shards 2 with ranksgd" in p.stderr and "RankSGD runs on one GPU" in p.stderr, p.stderr
    assert "Rating data set has been successfully loaded." not in p.stdout
    p = subprocess.run([EXE, "-c", _conf(tmp_path, ["recommender=RankSGD", "item.ranking=on -topN 10"], threshold="-1")], capture_output=True,
                       text=True, timeout=120)                          # checkBinary(): RankSGD.java:58, Recommender.java:1154-1160
    assert p.returncode == 1 and "val.binary.threshold=-1.0, ratings must be binarized first! Try set a non-negative value." in p.stderr, p.stderr


HOST_PROBE = r"""
#include <cstdio>
#include "recommender.hpp"
using namespace carskit;
int main(int argc, char **argv) {
    FileConfiger cf(argv[1]);
    Conf c(cf);
    RatingData d;
    d.n_users = NU, d.n_items = NI;
    d.u = {0}, d.j = {0}, d.ctx = {0}, d.r = {1.0};
    RankSGD m(d, d, 0, c);
    m.initModel();
    printf("ranking %d size %d\n", (int)c.isRankingPred, (int)c.ranksgdNumRatesSize);
    for (double x : m.P) printf("P %a\n", x);
    for (double x : m.Q) printf("Q %a\n", x);
    return 0;
}
"""


def test_host_init_model_equals_the_reference_draw(tmp_path):
    """a stand-alone program over the host classes' header: RankSGD::initModel() (gaussian, initByNorm = true) against the golden draw"""
    import subprocess
    g = rr.golden()["init"]
    nu, ni, k = g["n_users"], g["n_items"], g["k"]
    (tmp_path / "probe.cpp").write_text(HOST_PROBE.replace("NU", str(nu)).replace("NI", str(ni)))
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "carskit_amd", "csrc", "host"), str(tmp_path / "probe.cpp"),
                    "-L" + os.path.join(ROOT, "carskit_amd", "lib"), "-lcarskit_mi355x",
                    "-Wl,-rpath," + os.path.join(ROOT, "carskit_amd", "lib"), "-o", exe], check=True, timeout=300)
    (tmp_path / "s.conf").write_text("num.factors=%d\nevaluation.setup=cv -k 5 --rand-seed %d\n" % (k, g["seed"]))
    out = subprocess.run([exe, str(tmp_path / "s.conf")], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert out[0] == "ranking 0 size 0"                    # the class, not Conf, turns ranking on; the divisor is the reference's
    P = [float.fromhex(ln.split()[1]) for ln in out if ln.startswith("P ")]
    Q = [float.fromhex(ln.split()[1]) for ln in out if ln.startswith("Q ")]
    assert same_bits_exact(P, rr.unhex(g["P"], nu * k)) and same_bits_exact(Q, rr.unhex(g["Q"], ni * k))
