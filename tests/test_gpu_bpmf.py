"""BPMF on the GPU through the C ABI, bit for bit: the device's nextGaussian() stream against java.util.Random (the host restatement and
the golden file's draws), the moment kernels against DenseMatrix.columnMean / cov(), whole iterations against the run of the reference's
own source (tests/golden/reference_bpmf.json.gz), the row kernel at every shape that takes another path against the CPU restatement
(tests/bpmf_ref.py), the null factor and the exact second pass of the draw offsets, and the driver's RMSE / MAE on a generated file."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from carskit_amd import capi, dao
from oracle.oracle_np import JavaRandom
from tests import bpmf_ref as ref
from tests.hostmirror import splitter
from tests.knn_ref import eval_ratings
from tests.util import global_mean, same_bits, to2d

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "carskit_amd", "bin", "carskit-mi355x")

BLOCK, TILE, CHUNK = capi.BPMF_GAUSS_BLOCK, capi.BPMF_TILE, capi.BPMF_CHUNK
ROW_BLOCK, STAGE_MIN = capi.BPMF_BLOCK, capi.BPMF_STAGE_MIN
RUNS = ref.golden()["runs"]


# ---- the gaussian stream ----------------------------------------------------------------------------------------------------------
def host_gaussians(stream, n):
    r = ref.Stream(*stream)
    out = np.array([r.gaussian() for _ in range(n)])
    return out, (r.state, r.have, r.cached if r.have else 0.0)


def same_stream(a, b):
    return a[0] == b[0] and bool(a[1]) == bool(b[1]) and (not a[1] or same_bits([a[2]], [b[2]]))


def check_gaussians(stream, n, want=None):
    got, after = capi.java_next_gaussians(stream[0], n, stream[1], stream[2])
    if want is None:
        want = host_gaussians(stream, n)
    assert same_bits(got, want[0]), (n, np.flatnonzero(got != want[0])[:5])
    assert same_stream(after, want[1]), (n, after, want[1])
    return after


def pairs_needed(n, have):
    return (n - (1 if have else 0) + 1) // 2


LONG_SEED = (ref.random_state(20261230), False, 0.0)
LONG_CUTS = (377, 378, 379, 380, 381, 382, 98300, 98302, 110001)


@functools.lru_cache(maxsize=None)
def long_run():
    """110 001 values from one seed and the stream after each of LONG_CUTS, shared by the cases that cut a prefix of it"""
    r = ref.Stream(*LONG_SEED)
    out, after = [], {}
    for n in range(1, LONG_CUTS[-1] + 1):
        out.append(r.gaussian())
        if n in LONG_CUTS:
            after[n] = (r.state, r.have, r.cached if r.have else 0.0)
    return np.array(out), after


def test_gaussians_equal_the_golden_draws():
    g = ref.golden()["gaussian"]
    want = np.array([float.fromhex(x) for x in g["draws"]])
    got, _ = capi.java_next_gaussians(ref.random_state(g["seed"]), len(want))
    assert same_bits(got, want)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 7])
def test_gaussians_small_counts_with_and_without_a_cached_value(n):
    fresh = (ref.random_state(5), False, 0.0)
    after = check_gaussians(fresh, n)
    r = ref.Stream(fresh[0])
    r.gaussian()
    cached = (r.state, True, r.cached)
    check_gaussians(cached, n)             # n odd from a cached value ends without one; n even ends on a fresh pair's first
    check_gaussians(after, n)              # and on from where the first call ended (cached after an odd n)


def test_gaussians_across_the_block_border():
    """the first round takes attempts(pairs) attempts, BLOCK a workgroup: pairs = 189, 190, 191 give BLOCK - 1, BLOCK, BLOCK + 1"""
    assert [capi.bpmf_gauss_attempts(p) for p in (189, 190, 191)] == [BLOCK - 1, BLOCK, BLOCK + 1]
    run, after = long_run()
    for n in (377, 378, 379, 380, 381, 382):
        check_gaussians(LONG_SEED, n, (run[:n], after[n]))
    r = ref.Stream(LONG_SEED[0])
    r.gaussian()
    for n in (379, 381, 383):              # the same borders from a cached value: pairs = (n - 1) / 2
        assert pairs_needed(n, True) in (189, 190, 191)
        check_gaussians((r.state, True, r.cached), n)


def test_gaussians_across_the_scan_border():
    """the scan takes BLOCK workgroups a pass: pairs = 49150 and 49151 give BLOCK and BLOCK + 1 workgroups; 110 001 values take their
    last pairs from workgroups past the first pass, so the carried total is read"""
    att = [capi.bpmf_gauss_attempts(p) for p in (49150, 49151)]
    assert [(a + BLOCK - 1) // BLOCK for a in att] == [BLOCK, BLOCK + 1]
    run, after = long_run()
    for n in (98300, 98302, 110001):
        check_gaussians(LONG_SEED, n, (run[:n], after[n]))
    assert 110001 // 2 * 4 // 3 > BLOCK * BLOCK   # more attempts needed than one pass of the scan covers


def attempts_accepted(state, n_att):
    ok = 0
    for _ in range(n_att):
        ok += ref.polar_attempt(state)[0]
        for _ in range(4):
            state = (state * 0x5DEECE66D + 0xB) & ref.MASK
    return ok


@functools.lru_cache(maxsize=None)
def short_states():
    """start states (by a search over seeds) whose first attempts(pairs) attempts accept fewer than `pairs`, for n = 2, 4 and 9: the
    device's first round falls short and the next one goes on from where it ended"""
    found = {}
    for n in (2, 4, 9):
        pairs = pairs_needed(n, False)
        for seed in range(1, 200000):
            st = ref.random_state(seed)
            if attempts_accepted(st, capi.bpmf_gauss_attempts(pairs)) < pairs:
                found[n] = st
                break
    return found


def test_gaussians_when_the_first_round_accepts_too_few():
    found = short_states()
    assert sorted(found) == [2, 4, 9]
    for n, st in found.items():
        pairs = pairs_needed(n, False)
        assert attempts_accepted(st, capi.bpmf_gauss_attempts(pairs)) < pairs   # the property, by the host stream
        check_gaussians((st, False, 0.0), n)
        check_gaussians((st, False, 0.0), n - 1)


# ---- columnMean and cov() ---------------------------------------------------------------------------------------------------------
# every row count at k = 1, 3, 64 (one workgroup of bpmf_cov_kernel, or only full ones); two row counts at k = 16 (exactly one full
# workgroup) and at k = 17, 33, 63, whose last workgroup has dead lanes that still stage rows and meet the barriers
MOMENT_SHAPES = [(rows, k) for k in (1, 3, 64) for rows in (1, 2, TILE - 1, TILE, TILE + 1, 3 * TILE + 1)] + \
                [(rows, k) for k in (16, 17, 33, 63) for rows in (TILE + 1, 3 * TILE + 1)]


@pytest.mark.parametrize("rows,k", MOMENT_SHAPES, ids=["%d-%d" % s for s in MOMENT_SHAPES])
def test_moments_equal_the_restatement(rows, k):
    rng = np.random.default_rng(1000 * rows + k)
    X = rng.standard_normal((rows, k)) * 2.0 + 0.5
    mean, cov = capi.bpmf_moments(X)
    assert same_bits(mean, ref.column_mean(X)) and same_bits(cov, ref.cov(X))
    if rows == 1:
        assert np.isnan(cov).all()                       # 0 / 0, as the golden file has it
    if rows > 2:
        X[rows // 2, k // 2] = np.nan                    # Stats.mean skips it, columnMean does not
        mean, cov = capi.bpmf_moments(X)
        assert same_bits(mean, ref.column_mean(X)) and same_bits(cov, ref.cov(X))
        assert np.isnan(mean[k // 2]) and np.isnan(cov[k // 2]).all()
    if k in (16, 17, 33, 63):
        # the NaN in the LAST column: its elements (f, k - 1) start in the first workgroup and its row (k - 1, g) ends the last one
        groups = (k * k + ROW_BLOCK - 1) // ROW_BLOCK
        assert k - 1 < ROW_BLOCK and (k * k - 1) // ROW_BLOCK == groups - 1
        assert (groups, k * k % ROW_BLOCK) == {16: (1, 0), 17: (2, 33), 33: (5, 65), 63: (16, 129)}[k]   # the live lanes of the last one
        X = rng.standard_normal((rows, k)) * 2.0 + 0.5
        X[rows // 3, k - 1] = np.nan
        mean, cov = capi.bpmf_moments(X)
        want = ref.cov(X)
        assert same_bits(mean, ref.column_mean(X)) and same_bits(cov, want)
        assert np.isnan(cov[k - 1]).all() and np.isnan(cov[:, k - 1]).all() and np.isnan(cov).sum() == 2 * k - 1


def test_moments_with_a_column_that_is_nan_in_every_row():
    """Stats.mean of that column is 0 / 0: the centred column, and so its row and column of cov(), are NaN; columnMean is NaN as well.
    Held to the restatement alone: the golden file's `cov` cases record a single NaN entry (`nan_entry`) and no column without a
    number, so the reference's own answer to this input is not on record."""
    assert not any(np.isnan(ref.unhex(c["X"], c["rows"], c["k"])).all(axis=0).any() for c in ref.golden()["cov"])
    rows, k = TILE + 1, 17
    rng = np.random.default_rng(20270110)
    X = rng.standard_normal((rows, k)) * 2.0 + 0.5
    X[:, 0] = np.nan                                     # elements in the first workgroup
    X[:, k - 1] = np.nan                                 # and in the partial last one
    want_mean, want_cov = ref.column_mean(X), ref.cov(X)
    assert np.isnan(want_mean[[0, k - 1]]).all() and np.isnan(want_cov).sum() == 4 * k - 4
    mean, cov = capi.bpmf_moments(X)
    assert same_bits(mean, want_mean) and same_bits(cov, want_cov)
    assert np.array_equal(np.isnan(cov), np.isnan(want_cov))


def test_moments_equal_the_golden_cases():
    for case in ref.golden()["cov"]:
        X = ref.unhex(case["X"], case["rows"], case["k"])
        mean, cov = capi.bpmf_moments(X)
        assert same_bits(mean, ref.unhex(case["mean"], case["k"])) and same_bits(cov, ref.unhex(case["cov"], case["k"], case["k"])), case["name"]


# ---- whole iterations against the reference's run ------------------------------------------------------------------------------------
def all_tuples(nu, ni):
    return np.repeat(np.arange(nu, dtype=np.int32), ni), np.tile(np.arange(ni, dtype=np.int32), nu)


def instance(run, flags=capi.BPMF_FLAG_STRICT):
    nu, ni, k = run["n_users"], run["n_items"], run["k"]
    cells = ref.golden_cells(run)
    h = capi.BPMFInstance(k, nu, ni, flags=flags)
    h.set_ratings([c[0] for c in cells], [c[1] for c in cells], [c[2] for c in cells])
    h.set_global_mean(float.fromhex(run["global_mean"]))
    h.set_model(ref.unhex(run["P0"], nu, k), ref.unhex(run["Q0"], ni, k))
    h.set_stream(ref.random_state(run["seed_gibbs"]))
    return h


@pytest.mark.parametrize("run", RUNS, ids=lambda r: "%s-k%d" % (r["name"], r["k"]))
def test_golden_runs_match_the_reference_run(run):
    nu, ni, k = run["n_users"], run["n_items"], run["k"]
    h = instance(run)
    assert h.global_mean() == float.fromhex(run["global_mean"])
    h.init_hyper()
    for n, it in enumerate(run["iters"]):
        loss = h.iterate()
        P, Q = h.model()
        assert same_bits(P, ref.unhex(it["P"], nu, k)), (n, np.argwhere(P != ref.unhex(it["P"], nu, k))[:5])
        assert same_bits(Q, ref.unhex(it["Q"], ni, k)), (n, np.argwhere(Q != ref.unhex(it["Q"], ni, k))[:5])
        assert float(loss).hex() == it["loss"], n
    tu, tj = all_tuples(nu, ni)
    want = np.array([[float.fromhex(x) for x in row] for row in run["predict"]])
    assert same_bits(h.predict(tu, tj).reshape(nu, ni), want)
    lo, hi = 2.0, 4.0
    assert same_bits(h.predict(tu, tj, bound=True, lo=lo, hi=hi).reshape(nu, ni), np.where(want > hi, hi, np.where(want < lo, lo, want)))
    ms = h.last_iter_ms()
    assert len(ms) == 5 and all(x >= 0.0 for x in ms) and ms[2] > 0.0 and ms[3] > 0.0
    # the stream stands where the restatement's does after the same three iterations
    m = ref.BPMF(nu, ni, ref.golden_cells(run), float.fromhex(run["global_mean"]))
    P, Q = ref.unhex(run["P0"], nu, k), ref.unhex(run["Q0"], ni, k)
    r = ref.Stream.seeded(run["seed_gibbs"])
    hy = m.init_hyper(P, Q)
    for _ in run["iters"]:
        m.iterate(r, P, Q, hy)
    assert same_stream(h.stream(), (r.state, r.have, r.cached))
    au, mu, am, mm = h.hyper()
    assert same_bits(au, hy["alpha_u"]) and same_bits(mu, hy["mu_u"]) and same_bits(am, hy["alpha_m"]) and same_bits(mm, hy["mu_m"])
    h.close()


def tree_loss(terms):
    """the loss without CMI_BPMF_FLAG_STRICT: 256 terms a workgroup, in each wave the shuffle tree, the four waves in order, the
    workgroups' sums in one chain"""
    total = 0.0
    for b in range(0, len(terms), 256):
        t = np.zeros(256)
        t[:len(terms[b:b + 256])] = terms[b:b + 256]
        w = t.reshape(4, 64).copy()
        for off in (32, 16, 8, 4, 2, 1):
            w[:, :off] = w[:, :off] + w[:, off:2 * off]
        total += float(((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0])
    return total * 0.5


def test_loss_as_a_fixed_tree_without_the_strict_flag():
    run = next(r for r in RUNS if r["name"] == "knn_matrix" and r["k"] == 3)
    h = instance(run, flags=0)
    h.init_hyper()
    loss = h.iterate()
    P, Q = h.model()
    m = ref.BPMF(run["n_users"], run["n_items"], ref.golden_cells(run), float.fromhex(run["global_mean"]))
    assert len(m.loss_cells) > 256                                       # more than one workgroup
    terms = np.array([(r - ref.predict(P, Q, m.gm, u, j)) ** 2 for u, j, r in m.loss_cells])
    assert float(loss).hex() == float(tree_loss(terms)).hex()
    assert abs(loss - float.fromhex(run["iters"][0]["loss"])) <= 1e-12 * loss    # and the same sum, up to the order
    h.close()


def test_calls_out_of_order_and_bad_arguments():
    run = next(r for r in RUNS if r["name"] == "handmade" and r["k"] == 2)
    nu, ni, k = run["n_users"], run["n_items"], run["k"]
    cells = ref.golden_cells(run)
    h = capi.BPMFInstance(k, nu, ni)
    for call in (h.iterate, h.init_hyper, h.model, h.last_iter_ms, h.hyper, lambda: h.predict([0], [1])):
        with pytest.raises(capi.CmiError) as e:
            call()
        assert e.value.code == capi.E_INVALID
    h.set_ratings([c[0] for c in cells], [c[1] for c in cells], [c[2] for c in cells])
    with pytest.raises(capi.CmiError) as e:
        h.iterate()                                                      # ratings, but no model
    assert e.value.code == capi.E_INVALID and "cmi_bpmf_set_model first" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        h.set_model(P=np.zeros((nu, k)))                                 # the first call sets both sides
    assert e.value.code == capi.E_INVALID
    h.set_model(ref.unhex(run["P0"], nu, k), ref.unhex(run["Q0"], ni, k))
    with pytest.raises(capi.CmiError) as e:
        h.iterate()
    assert e.value.code == capi.E_INVALID and "cmi_bpmf_init_hyper first" in str(e.value)
    h.init_hyper()
    with pytest.raises(capi.CmiError) as e:
        h.iterate()
    assert e.value.code == capi.E_INVALID and "cmi_bpmf_set_stream first" in str(e.value)
    for bad in (lambda: h.set_stream(-1), lambda: h.set_stream(1 << 48), lambda: h.sample_side(2, np.eye(k), np.zeros(k)),
                lambda: h.predict([0], [ni]), lambda: h.set_ratings([0, 0], [1, 1], [1.0, 2.0])):
        with pytest.raises(capi.CmiError) as e:
            bad()
        assert e.value.code == capi.E_INVALID
    h.close()


# ---- the row kernel at the shapes that take another path -------------------------------------------------------------------------------
def row_per(k):
    """entries of a row the row kernel stages a pass at k factors"""
    return min(CHUNK, max(k * k, STAGE_MIN) // k)


@functools.lru_cache(maxsize=None)
def shape_matrix(per=CHUNK, twice=False):
    """14 users x 210 items (16 users with `twice`).  User 0 has no cell and user 1 one; users 2 .. 6 have per - 2 .. per + 2 (the
    staging chunk is `per` entries: CHUNK up to k = 16, fewer where 1024 or k x k LDS doubles hold fewer rows); user 7 has 200 (several
    chunks); user 8 has a NaN rating among 5 (the mean goes NaN, the factor does not); user 9 only a stored zero; the others 3 .. 6;
    with `twice` users 14 and 15 have 2 per and 2 per + 1.  Item 209 has no cell; items have 1 to a dozen entries."""
    rng = np.random.default_rng(20261231)
    nu, ni = (16 if twice else 14), 210
    counts = {0: 0, 1: 1, 2: per - 2, 3: per - 1, 4: per, 5: per + 1, 6: per + 2, 7: 200, 8: 5, 9: 0, 10: 3, 11: 4, 12: 5, 13: 6}
    if twice:
        counts.update({14: 2 * per, 15: 2 * per + 1})
    cells = []
    for u, c in counts.items():
        for j in sorted(rng.choice(ni - 1, size=c, replace=False).tolist()):
            cells.append((u, j, float(rng.integers(1, 11)) / 2.0))
    first8 = next(n for n, c in enumerate(cells) if c[0] == 8)
    cells[first8 + 2] = (8, cells[first8 + 2][1], float("nan"))
    cells.append((9, 17, 0.0))
    return nu, ni, cells


# k -> (per, element groups a thread): the borders between k = 10 and k = 63
ROW_BORDERS = {16: (64, 1), 17: (60, 2), 22: (46, 2), 23: (44, 3), 32: (32, 4), 33: (33, 5), 48: (48, 9)}


@pytest.mark.parametrize("k", [1, 2, 3, 10, 63, 64] + sorted(ROW_BORDERS))
def test_row_kernel_shapes_equal_the_restatement(k):
    """k = 1, 2, 3, 10, 63, 64 on the matrix cut around CHUNK; every k of ROW_BORDERS on the matrix cut around that k's own `per`, with
    rows of 2 per and 2 per + 1 entries as well"""
    per = CHUNK
    if k in ROW_BORDERS:
        per, stage = row_per(k), max(k * k, STAGE_MIN)
        assert (per, (k * k + ROW_BLOCK - 1) // ROW_BLOCK) == ROW_BORDERS[k]
        assert k != 32 or (stage == STAGE_MIN and 31 * 31 < STAGE_MIN)     # the last k that stages in STAGE_MIN doubles
        assert k != 33 or (stage == k * k and stage > STAGE_MIN)           # the first that stages in k x k
    nu, ni, cells = shape_matrix(per, k in ROW_BORDERS)
    rng = np.random.default_rng(4000 + k)
    P, Q = rng.standard_normal((nu, k)), rng.standard_normal((ni, k))
    b = rng.standard_normal((k, k)) * 0.3
    alpha, mu, gm = b @ b.T + np.eye(k), rng.standard_normal(k) * 0.2, 2.75
    m = ref.BPMF(nu, ni, cells, gm)
    assert [len(r) for r in m.rows][:10] == [0, 1, per - 2, per - 1, per, per + 1, per + 2, 200, 5, 0] and not m.cols[209]
    if k in ROW_BORDERS:
        assert [len(r) for r in m.rows][14:] == [2 * per, 2 * per + 1]
    h = capi.BPMFInstance(k, nu, ni)
    h.set_ratings([c[0] for c in cells], [c[1] for c in cells], [c[2] for c in cells])
    h.set_global_mean(gm)
    h.set_model(P, Q)
    r = ref.Stream.seeded(900 + k)
    h.set_stream(r.state)
    Pr, Qr = P.copy(), Q.copy()
    for side in (0, 1):
        flags, draws = h.sample_side(side, alpha, mu)
        want_flags, want_draws = m.sample_side(r, side, Pr, Qr, alpha, mu)
        Pd, Qd = h.model()
        assert same_bits(Pd, Pr), (side, np.argwhere(~((Pd == Pr) | (np.isnan(Pd) & np.isnan(Pr))))[:5])
        assert same_bits(Qd, Qr), (side, np.argwhere(~((Qd == Qr) | (np.isnan(Qd) & np.isnan(Qr))))[:5])
        assert flags.tolist() == want_flags and draws == want_draws
        assert same_stream(h.stream(), (r.state, r.have, r.cached))
        # a NaN RATING makes the mean NaN, never the factor (user 8).  A NaN partner ROW (what user 8's items then read) makes the whole
        # matrix NaN: inv() finds no pivot and returns the identity as it stands, so the factor exists and the mean is NaN -- but for
        # k = 1, where inv() is 1 / NaN and the factor is null: those five items keep their rows and take no draw
        assert sum(want_flags) == (5 if (side, k) == (1, 1) else 0)
    assert np.isnan(Pr[8]).all() and same_bits(Pr[0], P[0]) and same_bits(Pr[9], P[9]) and same_bits(Qr[209], Q[209])   # NaN mean; kept rows
    assert np.isnan(Qr).any(axis=1).sum() == (0 if k == 1 else 5)
    h.close()


# ---- a null factor and the exact second pass -----------------------------------------------------------------------------------------
def null_matrix(all_null):
    """k = 2 with alpha = -I: a user with one entry has a rank-1 Gram matrix, 2 G - I is indefinite and covar has no factor; a user with
    eight well-spread entries has 2 G - I positive definite.  Users 0, 3, 4, 8 are of the first kind (or everyone, all_null)"""
    nu, ni = 10, 40
    rng = np.random.default_rng(20270101)
    cells = []
    for u in range(nu):
        c = 1 if all_null or u in (0, 3, 4, 8) else 8
        cells += [(u, j, float(rng.integers(1, 6))) for j in sorted(rng.choice(ni, size=c, replace=False).tolist())]
    return nu, ni, cells


def null_cells(counts, n_other, seed):
    """a side whose row x has counts[x] entries among n_other partners: (x, partner, value)"""
    rng = np.random.default_rng(seed)
    cells = []
    for x, c in enumerate(counts):
        cells += [(x, j, float(rng.integers(1, 6))) for j in sorted(rng.choice(n_other, size=c, replace=False).tolist())]
    return cells


def null_side0(counts):
    return len(counts), 40, null_cells(counts, 40, 20270104)


def null_side1(counts):
    """the same kinds among the ITEMS: 40 users, an item per count"""
    return 40, len(counts), [(u, j, v) for j, u, v in null_cells(counts, 40, 20270105)]


# with alpha = -I a row with fewer entries than k has a Gram matrix of lower rank, so 2 G - I is indefinite and covar has no factor; a
# dozen well-spread entries make it positive definite.  name -> (k, side, start from a cached gaussian, matrix, flags of the side's rows)
K3_MIXED = (1, 12, 12, 2, 1, 12, 12, 12, 1, 2)            # five rows draw: 15 draws, an odd number
NULL_CASES = {
    "mixed": (2, 0, False, lambda: null_matrix(False), [1, 0, 0, 1, 1, 0, 0, 0, 1, 0]),
    "all_null": (2, 0, False, lambda: null_matrix(True), [1] * 10),
    "k2_cached": (2, 0, True, lambda: null_matrix(False), [1, 0, 0, 1, 1, 0, 0, 0, 1, 0]),
    "k3_mixed": (3, 0, False, lambda: null_side0(K3_MIXED), [int(c < 3) for c in K3_MIXED]),
    "k3_cached": (3, 0, True, lambda: null_side0(K3_MIXED), [int(c < 3) for c in K3_MIXED]),
    "k2_side1": (2, 1, False, lambda: null_matrix(False), None),      # the items of the users' matrix: what they are is asserted below
    "k3_side1": (3, 1, False, lambda: null_side1(K3_MIXED), [int(c < 3) for c in K3_MIXED]),
    "k3_side1_cached": (3, 1, True, lambda: null_side1(K3_MIXED), [int(c < 3) for c in K3_MIXED]),
    "last_only": (3, 0, False, lambda: null_side0((12, 12, 12, 12, 12, 1)), [0, 0, 0, 0, 0, 1]),
    "first_only": (3, 0, False, lambda: null_side0((1, 12, 12, 12, 12, 12)), [1, 0, 0, 0, 0, 0]),
    "first_only_cached": (3, 0, True, lambda: null_side0((1, 12, 12, 12, 12, 12)), [1, 0, 0, 0, 0, 0]),
}


@functools.lru_cache(maxsize=None)
def null_case(case):
    """the inputs of a case and the restatement's pass over them"""
    k, side, cached, matrix, flags = NULL_CASES[case]
    nu, ni, cells = matrix()
    rng = np.random.default_rng(20270102)
    P, Q = rng.standard_normal((nu, k)), rng.standard_normal((ni, k)) * 1.5
    if side == 1 and k == 3:
        P = P * 1.5                                                      # the partners' rows, as spread as Q is for the users
    alpha, mu, gm = -np.eye(k), np.array([0.25, -0.5, 0.125][:k]), 3.0
    m = ref.BPMF(nu, ni, cells, gm)
    r = ref.Stream.seeded(4242)
    if cached:
        r.gaussian()
        assert r.have
    start = (r.state, r.have, r.cached if r.have else 0.0)
    Pr, Qr = P.copy(), Q.copy()
    want_flags, want_draws = m.sample_side(r, side, Pr, Qr, alpha, mu)
    return k, side, (nu, ni, cells), (P, Q, alpha, mu, gm), start, (Pr, Qr, want_flags, want_draws, (r.state, r.have, r.cached)), m


@pytest.mark.parametrize("case", sorted(NULL_CASES, key=list(NULL_CASES).index))
def test_null_factor_rows_and_the_exact_draw_offsets(case):
    all_null = case == "all_null"
    k, side, (nu, ni, cells), (P, Q, alpha, mu, gm), start, (Pr, Qr, want_flags, want_draws, end), m = null_case(case)
    own0, own_r, other0, other_r = (P, Pr, Q, Qr) if side == 0 else (Q, Qr, P, Pr)
    # the condition on the input, by the restatement: both kinds at least twice and a null row BEFORE a non-null one -- else the
    # first launch's offsets (every row with entries counted) would be right by accident
    if all_null:
        assert want_flags == [1] * nu and want_draws == 0 and end[:2] == start[:2] and same_bits(Pr, P)
    elif case == "mixed":
        assert want_flags == [1, 0, 0, 1, 1, 0, 0, 0, 1, 0] and want_draws == k * 6
        assert want_flags.count(1) >= 2 and want_flags.count(0) >= 2 and want_flags.index(1) < len(want_flags) - 1 - want_flags[::-1].index(0)
    lists = m.rows if side == 0 else m.cols
    slots = [x for x in range(len(lists)) if lists[x]]                   # the rows with entries, in the order of the pass
    slot_null = [want_flags[x] for x in slots]
    drawing = slot_null.count(0)
    if NULL_CASES[case][4] is not None:
        assert want_flags == NULL_CASES[case][4]
    assert want_draws == k * drawing and all(want_flags[x] == 0 for x in range(len(lists)) if not lists[x])
    assert start[1] == NULL_CASES[case][2] and end[1] == (start[1] != (want_draws % 2 == 1))
    if case in ("k3_mixed", "k3_cached", "k2_side1", "k3_side1", "k3_side1_cached", "k2_cached"):
        assert slot_null.count(1) >= 2 and drawing >= 2 and slot_null.index(1) < len(slot_null) - 1 - slot_null[::-1].index(0)
    if case.startswith("k3_"):
        assert drawing % 2 == 1 and end[1] != start[1]                   # the stream flips between cached and not across the pass
    if case == "k2_side1":
        assert len(slots) < ni and drawing == 6                          # items without a cell are no slot
    if case == "last_only":
        # nothing runs again, yet the stream must stand k (R - 1) draws on: an odd number, so it ends on a cached value
        assert slot_null == [0] * (len(slots) - 1) + [1] and want_draws == k * (len(slots) - 1) and end[1]
        rr = ref.Stream(*start)
        for _ in range(k * (len(slots) - 1)):
            rr.gaussian()
        assert (rr.state, rr.have) == end[:2]
    if case.startswith("first_only"):
        assert slot_null == [1] + [0] * (len(slots) - 1)                 # every other slot runs again, one rank lower
    h = capi.BPMFInstance(k, nu, ni)
    h.set_ratings([c[0] for c in cells], [c[1] for c in cells], [c[2] for c in cells])
    h.set_global_mean(gm)
    h.set_model(P, Q)
    h.set_stream(*start)
    flags, draws = h.sample_side(side, alpha, mu)
    got = h.model()
    own_d, other_d = got[side], got[1 - side]
    assert flags.tolist() == want_flags and draws == want_draws
    assert same_bits(own_d, own_r) and same_bits(other_d, other0) and same_bits(other_r, other0)
    null_rows = [x for x in range(len(lists)) if want_flags[x]]
    assert same_bits(own_d[null_rows], own0[null_rows])                  # the kept old rows
    assert same_stream(h.stream(), end)
    h.close()


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
def test_driver_reproduces_the_restatement_on_a_generated_file(tmp_path):
    iters, k, seed = 2, 3, 7
    rng = np.random.default_rng(20270103)
    lines = ["userid,itemid,rating,Time,Location"]
    seen = set()
    while len(lines) < 241:
        u, i, t, loc = int(rng.integers(24)), int(rng.integers(15)), ("day", "night")[int(rng.integers(2))], ("home", "out", "NA")[int(rng.integers(3))]
        if (u, i, t, loc) not in seen:
            seen.add((u, i, t, loc))
            lines.append("u%d,i%d,%d,%s,%s" % (u, i, int(rng.integers(1, 6)), t, loc))
    (tmp_path / "ratings.txt").write_text("\n".join(lines) + "\n")
    dao.transform(str(tmp_path / "ratings.txt"), str(tmp_path / "train.csv"))
    d = dao.DataDAO(str(tmp_path / "train.csv")).rating_data()
    labels, nf = splitter.split_folds(d.n, 3, seed)
    (tmp_path / "bpmf.conf").write_text("\n".join([
        "dataset.ratings.lins=%s" % (tmp_path / "ratings.txt"), "ratings.setup=-threshold -1 -datatransformation 1 -fullstat -1",
        "recommender=bpmf", "evaluation.setup=cv -k 3 -p off --rand-seed %d --test-view all" % seed, "item.ranking=off -topN 10",
        "output.setup=-folder %s -verbose off" % (tmp_path / "ws"), "num.factors=%d" % k, "num.max.iter=%d" % iters,
        "learn.rate=2e-2 -max -1 -bold-driver", "reg.lambda=0.0001 -c 0.001"]) + "\n")
    p = subprocess.run([EXE, "-c", str(tmp_path / "bpmf.conf")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    got = re.search(r"Final Results by BPMF, MAE: (\S+), RMSE: (\S+),", p.stdout)
    assert got, p.stdout
    mae = rmse = 0.0
    for f in range(1, nf + 1):
        tr, te = splitter.kth_fold(d, labels, f)
        u, i, r = to2d(tr.u, tr.j, tr.r)
        m = ref.BPMF(d.n_users, d.n_items, list(zip(u.tolist(), i.tolist(), r.tolist())), global_mean(tr.r))
        init = JavaRandom(seed)
        for _ in range((d.n_users + d.n_items) * k):    # IterativeRecommender.initModel's own P and Q, overwritten by BPMF's
            init.next_gaussian()
        P, Q = ref.init_model(init, d.n_users, d.n_items, k)
        gibbs = ref.Stream.seeded(seed)
        hy = m.init_hyper(P, Q)
        for _ in range(iters):
            m.iterate(gibbs, P, Q, hy)
        pred = np.array([ref.predict(P, Q, m.gm, int(a), int(b)) for a, b in zip(te.u, te.j)])
        pred = np.where(pred > d.max_rate, d.max_rate, np.where(pred < d.min_rate, d.min_rate, pred))
        fm, fr = eval_ratings(pred.tolist(), te.r.tolist(), d.min_rate)
        mae += fm / nf
        rmse += fr / nf
    assert (got.group(1), got.group(2)) == ("%.6f" % mae, "%.6f" % rmse), (got.groups(), repr(mae), repr(rmse))
