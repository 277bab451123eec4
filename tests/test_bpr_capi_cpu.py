"""BPR without a GPU: the C ABI symbols (header, binding table, library), the refusals that answer before any device call, and the
host-only entry points against tests/bpr_ref.py: java.util.Random.nextInt(bound), StrictMath.exp / log, the host walk of the sampler
and the level builder."""
import os
import re

import numpy as np
import pytest

from carskit_amd import capi
from tests import bpr_ref as bref
from tests.util import same_bits_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("cmi_bpr_create", "cmi_bpr_destroy", "cmi_bpr_last_error", "cmi_bpr_set_ratings", "cmi_bpr_set_model", "cmi_bpr_get_model",
           "cmi_bpr_set_random_state", "cmi_bpr_get_random_state", "cmi_bpr_sample", "cmi_bpr_iterate", "cmi_bpr_predict_batch",
           "cmi_bpr_eval_rankings", "cmi_bpr_last_iter_ms", "cmi_bpr_last_schedule", "cmi_bpr_levels", "cmi_bpr_sample_host",
           "cmi_bpr_rank_block")
JAVA_SYMBOLS = ("cmi_java_next_ints", "cmi_java_exp_log")


def edge_cells():
    """37 x 60: user 0 has no cell, user 1 one cell, user 2 holds 59 of the 60 items, user 3 only a stored zero; the others 1 .. 12
    items (counts that are and are not powers of two)"""
    rng = np.random.default_rng(20261220)
    cells = [(1, 17, 4.0), (3, 5, 0.0)] + [(2, j, 1.0 + j % 5) for j in range(60) if j != 31]
    for u in range(4, 37):
        for j in rng.choice(60, size=1 + (u * 5) % 12, replace=False):
            cells.append((u, int(j), float(1 + (u + j) % 5)))
    return 37, 60, cells


def pow2_cells():
    """64 x 128: both nextInt bounds of the u and j draws are powers of two"""
    rng = np.random.default_rng(20261221)
    cells = []
    for u in range(64):
        for j in rng.choice(128, size=1 + (u * 7) % 20, replace=False):
            cells.append((u, int(j), float(1 + (u + j) % 5)))
    return 64, 128, cells


def cols(cells):
    return ([c[0] for c in cells], [c[1] for c in cells], [c[2] for c in cells])


def test_bpr_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "carskit_mi355x.h")).read()
    assert sorted(set(re.findall(r"\b(cmi_bpr_\w+)\(", header))) == sorted(SYMBOLS)
    assert set(JAVA_SYMBOLS) <= set(re.findall(r"\b(cmi_java_\w+)\(", header))
    L = capi.lib()
    bound = {name for name, _, _ in capi.SYMBOLS}
    assert {n for n in bound if n.startswith("cmi_bpr_")} == set(SYMBOLS) and set(JAVA_SYMBOLS) <= bound
    for s in SYMBOLS + JAVA_SYMBOLS:
        assert getattr(L, s) is not None
    assert L.cmi_abi_version() == 5
    for m in ("set_ratings", "set_model", "model", "set_random_state", "random_state", "sample", "iterate", "predict", "eval_rankings",
              "last_iter_ms", "last_schedule", "close"):
        assert callable(getattr(capi.BPRInstance, m))
    assert L.cmi_bpr_rank_block() >= 256


def test_argument_checks_answer_before_any_device_call():
    with pytest.raises(capi.CmiError) as e:
        capi.BPRInstance(129, 10, 10)
    assert e.value.code == capi.E_UNSUPPORTED and "cmi_bpr_create" in str(e.value) and "k <= 128" in str(e.value)
    for k, nu, ni, flags in ((0, 10, 10, 0), (4, 0, 10, 0), (4, 10, -1, 0), (4, 10, 10, 0x100)):
        with pytest.raises(capi.CmiError) as e:
            capi.BPRInstance(k, nu, ni, flags=flags)
        assert e.value.code == capi.E_INVALID, (k, nu, ni, flags)
    L = capi.lib()
    assert L.cmi_bpr_create(4, 10, 10, 0, 0, None) == capi.E_INVALID
    for call in (lambda: L.cmi_bpr_iterate(None, 0.1, 0.1, 0.1, None), lambda: L.cmi_bpr_set_ratings(None, 0, None, None, None),
                 lambda: L.cmi_bpr_set_model(None, None, None), lambda: L.cmi_bpr_get_model(None, None, None),
                 lambda: L.cmi_bpr_predict_batch(None, 0, None, None, None), lambda: L.cmi_bpr_last_iter_ms(None, None),
                 lambda: L.cmi_bpr_last_schedule(None, None), lambda: L.cmi_bpr_sample(None, 0, None, None, None, None),
                 lambda: L.cmi_bpr_set_random_state(None, 0), lambda: L.cmi_bpr_get_random_state(None, None)):
        assert call() == capi.E_INVALID
    assert L.cmi_bpr_destroy(None) == capi.OK


def test_bpr_instance_without_device():
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(capi.CmiError) as e:
        capi.BPRInstance(10, 10, 10)
    assert e.value.code == capi.E_NO_DEVICE and "cmi_bpr_create" in str(e.value) and "no CPU fallback" in str(e.value)


def test_host_refusals_full_row_bad_ids_no_cells():
    """the reference would spin on a user who holds every item (and on a matrix without a non-zero cell): refused with E_INVALID"""
    full = [(0, 0, 1.0), (1, 0, 2.0), (1, 1, 3.0), (1, 2, 1.0)]
    with pytest.raises(capi.CmiError) as e:
        capi.bpr_sample_host(2, 3, *cols(full), bref.random_state(1), 10)
    assert e.value.code == capi.E_INVALID and "user 1 holds every item" in str(e.value)
    full[3] = (1, 2, 0.0)                   # a stored zero is not held
    assert len(capi.bpr_sample_host(2, 3, *cols(full), bref.random_state(1), 10)[0]) == 10
    with pytest.raises(capi.CmiError) as e:
        capi.bpr_sample_host(2, 3, [0, 2], [0, 1], [1.0, 1.0], bref.random_state(1), 10)
    assert e.value.code == capi.E_INVALID and "out of range" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        capi.bpr_sample_host(2, 3, [0], [1], [0.0], bref.random_state(1), 10)
    assert e.value.code == capi.E_INVALID and "no user with a non-zero cell" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        capi.bpr_levels(2, 3, [0, 1], [0, 3], [1, 2])
    assert e.value.code == capi.E_INVALID


@pytest.mark.parametrize("bound", [1, 2, 64, 60, (1 << 30) + 1])
def test_host_next_int_equals_the_restatement(bound):
    n = 3000
    st = bref.random_state(20261222 + bound)
    v, after = capi.java_next_ints(st, bound, n)
    r = bref.JavaStream(st)
    assert v.tolist() == [r.next_int(bound) for _ in range(n)] and after == r.state
    if bound == (1 << 30) + 1:
        assert r.draws > n + n // 4         # the rejection branch was taken, about once a value
    elif bound & (bound - 1) == 0:
        assert r.draws == n


def test_host_exp_log_equal_the_restatement():
    inf, nan = float("inf"), float("nan")
    xs = np.concatenate([np.random.default_rng(20261223).uniform(-40.0, 40.0, 20000),
                         [0.0, -0.0, inf, -inf, nan, 709.782712893384, 709.7827128933841, -745.1332191019411, -745.1332191019412, -710.0,
                          1e-10, -1e-10, 0.3, -0.3, 0.4, 1.0, -1.0, 1.03, 5e-324, 1e-310, 2.2250738585072014e-308, -2.5, 1e300]])
    e, l = capi.java_exp_log(xs)
    with np.errstate(all="ignore"):
        re_ = np.array([bref.fdlibm_exp(x) for x in xs.tolist()])
        rl = np.array([bref.fdlibm_log(x) for x in xs.tolist()])
    assert np.array_equal(np.isnan(e), np.isnan(re_)) and np.array_equal(np.isnan(l), np.isnan(rl))   # where a NaN stands, not which
    ok = ~np.isnan(re_)
    assert same_bits_exact(e[ok], re_[ok])
    ok = ~np.isnan(rl)
    assert same_bits_exact(l[ok], rl[ok])


@pytest.mark.parametrize("make", [edge_cells, pow2_cells])
def test_host_sampler_equals_the_restatement(make):
    nu, ni, cells = make()
    m = bref.BPR(nu, ni, cells)
    st = bref.random_state(20261224)
    u, i, j, after = capi.bpr_sample_host(nu, ni, *cols(cells), st, nu * 100)
    r = bref.JavaStream(st)
    tri = m.sample_iteration(r)
    assert list(zip(u.tolist(), i.tolist(), j.tolist())) == tri and after == r.state
    assert r.draws > 3 * nu * 100           # redraws happened (an empty user or a held j)
    # the stream goes on where it stopped
    u2, i2, j2, after2 = capi.bpr_sample_host(nu, ni, *cols(cells), after, 50)
    assert list(zip(u2.tolist(), i2.tolist(), j2.tolist())) == m.sample_iteration(r, 50) and after2 == r.state


def test_host_sampler_equals_the_golden_triples():
    for run in bref.golden_runs():
        st = bref.random_state(run["seed"])
        for it in run["iters"]:
            u, i, j, st = capi.bpr_sample_host(run["n_users"], run["n_items"], *cols(run["cells"]), st, run["n_users"] * 100)
            assert list(zip(u.tolist(), i.tolist(), j.tolist())) == it["triples"] and st == it["state"], run["name"]


def test_levels_are_a_row_disjoint_order_preserving_schedule():
    nu, ni, k = 23, 31, 3
    rng = np.random.default_rng(20261225)
    n = 4000
    u, i, j = rng.integers(0, nu, n), rng.integers(0, ni, n), rng.integers(0, ni, n)
    j[::97] = i[::97]                       # j == i happens in the reference (contains() misses entries)
    order, level_of, n_levels, chain = capi.bpr_levels(nu, ni, u, i, j)
    tri = list(zip(u.tolist(), i.tolist(), j.tolist()))
    assert sorted(order.tolist()) == list(range(n))                         # a permutation
    assert level_of.tolist() == bref.levels(nu, ni, tri) and n_levels == max(level_of)
    assert np.all(np.diff(level_of[order]) >= 0)                            # sorted by level ...
    last_p, last_q = {}, {}
    seen = {}
    for x, s in enumerate(order.tolist()):
        lv = int(level_of[s])
        rows = {("P", tri[s][0]), ("Q", tri[s][1]), ("Q", tri[s][2])}
        for r in rows:
            assert seen.get((lv, r)) is None, "two samples of level %d share row %s" % (lv, r)    # row-disjoint inside a level
            seen[(lv, r)] = s
            d = last_p if r[0] == "P" else last_q
            assert d.get(r[1], -1) < s                                      # per row, schedule order == sample order
            d[r[1]] = s
    counts = np.bincount(np.concatenate([u, i + nu, np.where(j != i, j, -1)[j != i] + nu]))
    assert chain == counts.max() and n_levels >= chain
    # replaying the single-sample update in schedule order gives the sequential epoch's bits
    P0, Q0 = rng.random((nu, k)), rng.random((ni, k))
    P, Q = P0.tolist(), Q0.tolist()
    bref.epoch(P, Q, tri, 0.05, 0.02, 0.03)
    P2, Q2 = P0.tolist(), Q0.tolist()
    for s in order.tolist():
        bref.update(P2, Q2, *tri[s], 0.05, 0.02, 0.03)
    assert same_bits_exact(np.array(P), np.array(P2)) and same_bits_exact(np.array(Q), np.array(Q2))


# ---- the driver ------------------------------------------------------------------------------------------------------------------
EXE = os.path.join(ROOT, "carskit_amd", "bin", "carskit-mi355x")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _conf(tmp_path, extra):
    import shutil
    shutil.copyfile(os.path.join(GOLDEN, "depaul_ratings_compact.csv"), tmp_path / "ratings.txt")
    conf = open(os.path.join(GOLDEN, "depaul_setting.conf")).read().replace("PLACEHOLDER_SET_BY_TEST", str(tmp_path / "ratings.txt"))
    conf = conf.replace("-threshold -1", "-threshold 0")
    lines = [ln for ln in conf.splitlines() if not ln.startswith(("recommender", "item.ranking", "num.max.iter"))]
    (tmp_path / "setting.conf").write_text("\n".join(lines + extra) + "\n")
    return str(tmp_path / "setting.conf")


def test_driver_knows_bpr(tmp_path):
    """recommender=bpr reaches the model, as a top-N run whatever item.ranking says: with a GPU the run ends with BPR's ranking results,
    without one it stops at cmi_bpr_create"""
    import subprocess
    p = subprocess.run([EXE, "-c", _conf(tmp_path, ["recommender=BPR", "item.ranking=off", "num.max.iter=2"])], capture_output=True,
                       text=True, timeout=300)
    assert "not on the accelerated path" not in p.stdout + p.stderr, p.stderr
    if capi.device_count() > 0:
        assert p.returncode == 0 and "Final Results by BPR" in p.stdout and "Pre5" in p.stdout, p.stderr
    else:
        assert "cmi_bpr_create" in p.stdout + p.stderr and "no HIP device" in p.stdout + p.stderr, (p.stdout, p.stderr)
    p = subprocess.run([EXE, "-c", _conf(tmp_path, ["recommender=bprx", "item.ranking=off"])], capture_output=True, text=True, timeout=300)
    assert "not on the accelerated path" in p.stdout + p.stderr and " bpr," in p.stdout + p.stderr


def test_driver_refuses_bpr_shards(tmp_path):
    import subprocess
    p = subprocess.run([EXE, "-c", _conf(tmp_path, ["recommender=BPR", "item.ranking=on -topN 10"]), "--shards", "2"], capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 1 and "--shards 2 with bpr" in p.stderr and "BPR runs on one GPU" in p.stderr, p.stderr
    assert "Rating data set has been successfully loaded." not in p.stdout


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
    BPR m(d, d, 0, c);
    m.initModel();
    printf("ranking %d\n", (int)c.isRankingPred);
    for (double x : m.P) printf("P %a\n", x);
    for (double x : m.Q) printf("Q %a\n", x);
    JavaRandom r(42);                       // fdlibm's log moved to java_math.hpp: nextGaussian keeps its known answer
    printf("G %.17g\n", r.nextGaussian());
    JavaRandom q(42);                       // nextInt(bound) on the host stream, then the stream goes on
    printf("I");
    for (int t = 0; t < 5; ++t) printf(" %d", q.nextInt(10));
    printf(" %d\n", q.next(31));
    return 0;
}
"""


def test_host_init_model_equals_the_reference_draw(tmp_path):
    """a stand-alone program over the host classes' header: BPR::initModel() (uniform, initByNorm = false) against the golden draw"""
    import subprocess
    g = bref.golden()["init"]
    nu, ni, k = g["n_users"], g["n_items"], g["k"]
    (tmp_path / "probe.cpp").write_text(HOST_PROBE.replace("NU", str(nu)).replace("NI", str(ni)))
    exe = str(tmp_path / "probe")
    subprocess.run(["g++", "-O0", "-std=c++17", "-pthread", "-I", os.path.join(ROOT, "carskit_amd", "csrc", "host"), str(tmp_path / "probe.cpp"),
                    "-L" + os.path.join(ROOT, "carskit_amd", "lib"), "-lcarskit_mi355x",
                    "-Wl,-rpath," + os.path.join(ROOT, "carskit_amd", "lib"), "-o", exe], check=True, timeout=300)
    (tmp_path / "s.conf").write_text("num.factors=%d\nevaluation.setup=cv -k 5 --rand-seed %d\n" % (k, g["seed"]))
    out = subprocess.run([exe, str(tmp_path / "s.conf")], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    assert out[0] == "ranking 0"                           # item.ranking is absent: the class, not Conf, turns ranking on
    P = [float.fromhex(ln.split()[1]) for ln in out if ln.startswith("P ")]
    Q = [float.fromhex(ln.split()[1]) for ln in out if ln.startswith("Q ")]
    assert same_bits_exact(P, bref.unhex(g["P"], nu * k)) and same_bits_exact(Q, bref.unhex(g["Q"], ni * k))
    assert out[-2] == "G 1.1419053154730547"               # new java.util.Random(42).nextGaussian()
    r = bref.JavaStream(bref.random_state(42))
    assert out[-1] == "I 0 3 8 4 0 %d" % r_after(r)        # new java.util.Random(42).nextInt(10) five times, then next(31)


def r_after(r):
    for _ in range(5):
        r.next_int(10)
    return r.next(31)
