"""LRMF on the GPU: the golden runs of the reference through the C ABI, the unit epoch against tests/lrmf_ref.py in the LDS form and the
global form (factor counts, unit sizes at the workgroup and LDS borders, the launch shapes of the schedule), the two loss forms, the
numeric failure, prediction, the top-N evaluation and the driver."""
import functools

import numpy as np
import pytest

from carskit_amd import capi
from tests import lrmf_ref as lref
from tests.test_gpu_rankals import all_tuples, check_rankings, contextual_split
from tests.test_lrmf_capi_cpu import cols
from tests.util import same_bits, same_bits_exact

pytestmark = pytest.mark.gpu

RUNS = lref.golden_runs()
LR, REG_U, REG_I = 0.05, float(np.float32(0.02)), float(np.float32(0.03))    # distinct, loud regularisation
FORMS = [("lds", 0), ("global", capi.LRMF_FLAG_GLOBAL_ROWS)]
ITERS = 3


def instance(k, nu, ni, cells, P=None, Q=None, flags=capi.LRMF_FLAG_STRICT):
    h = capi.LRMFInstance(k, nu, ni, flags=flags)
    h.set_ratings(*cols(cells))
    if P is not None:
        h.set_model(P, Q)
    return h


@pytest.mark.parametrize("form,flag", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_golden_runs_match_the_reference_run(run, form, flag):
    nu, ni = run["n_users"], run["n_items"]
    h = instance(run["k"], nu, ni, run["cells"], run["P0"], run["Q0"], flags=capi.LRMF_FLAG_STRICT | flag)
    finite = not run["name"].startswith("handmade k")
    for n, it in enumerate(run["iters"]):
        if finite:
            loss = h.iterate(run["lrate"], run["reg_u"], run["reg_i"])
            assert same_bits_exact([loss], [it["loss"]]), (n, loss, it["loss"])
        else:                                                        # the user whose only cell is a stored zero: uexp = 0.0
            with pytest.raises(capi.CmiError) as e:
                h.iterate(run["lrate"], run["reg_u"], run["reg_i"])
            assert e.value.code == capi.E_NUMERIC and "loss = -inf" in str(e.value)
        P, Q = h.model()
        assert same_bits(P, it["P"]), (n, np.argwhere(P != it["P"])[:5])       # NaN where the reference has NaN, else bit for bit
        assert same_bits(Q, it["Q"]), (n, np.argwhere(Q != it["Q"])[:5])
    tu, tj = all_tuples(nu, ni)
    assert same_bits(h.predict(tu, tj).reshape(nu, ni), run["predict"])
    ms = h.last_iter_ms()
    assert len(ms) == 3 and all(x >= 0.0 for x in ms) and ms[0] > 0.0
    s = h.last_schedule()
    assert s["levels"] == max(lref.levels(nu, ni, run["cells"]))
    assert s["global_units"] == (sum(1 for row in lref.LRMF(nu, ni, run["cells"]).stored if row) if flag else 0)
    h.close()


# ---- the epoch against the restatement -------------------------------------------------------------------------------------------------
def reference(nu, ni, cells, k, seed, iters=ITERS):
    """the restatement's run: (P0, Q0, [(P, Q, strict loss, terms)] per iteration)"""
    rng = np.random.default_rng(seed)
    P0, Q0 = rng.random((nu, k)) * 0.5, rng.random((ni, k)) * 0.5
    m = lref.LRMF(nu, ni, cells)
    P, Q = P0.copy(), Q0.copy()
    out = []
    for _ in range(iters):
        loss, terms = m.epoch_np(P, Q, LR, REG_U, REG_I)
        out.append((P.copy(), Q.copy(), loss, terms))
    return P0, Q0, out


def check_forms(nu, ni, cells, k, seed, forms=FORMS, iters=ITERS):
    """both forms of the epoch against the restatement, bit for bit on P, Q and the strict loss; returns the schedules"""
    P0, Q0, ref = reference(nu, ni, cells, k, seed, iters)
    scheds = {}
    for form, flag in forms:
        h = instance(k, nu, ni, cells, P0, Q0, flags=capi.LRMF_FLAG_STRICT | flag)
        for n, (P, Q, loss, _) in enumerate(ref):
            got = h.iterate(LR, REG_U, REG_I)
            gP, gQ = h.model()
            assert same_bits_exact(gP, P), (form, n, np.argwhere(gP != P)[:5])
            assert same_bits_exact(gQ, Q), (form, n, np.argwhere(gQ != Q)[:5])
            assert same_bits_exact([got], [loss]), (form, n, got, loss)
        scheds[form] = h.last_schedule()
        h.close()
    return scheds


@functools.lru_cache(maxsize=None)
def uniform_cells(nu=300, ni=200, per=10, seed=20270301):
    """10 cells a user, uniform over the items; every seventh cell a stored zero"""
    rng = np.random.default_rng(seed)
    cells = []
    for u in range(nu):
        for n, j in enumerate(sorted(rng.choice(ni, size=per, replace=False).tolist())):
            cells.append((u, j, 0.0 if (u + n) % 7 == 0 else float(1 + (u + j) % 5) / 2.0))
    return nu, ni, cells


@pytest.mark.parametrize("k", [1, 2, 3, 10, 16, 17, 128])
def test_epoch_matches_the_restatement_at_every_factor_count(k):
    """120 x 80, 8 cells a user: wide levels and single-unit runs, at the factor counts around the odd-stride padding and the limit"""
    nu, ni, cells = uniform_cells(120, 80, 8, 20270302)
    s = check_forms(nu, ni, cells, k, 20270310 + k)
    assert s["lds"]["global_units"] == 0 and s["global"]["global_units"] == nu
    assert s["lds"]["alone"] >= 1


def one_big_user(n_u, ni=None, others=3):
    """user 0 with n_u cells (every fifth a stored zero), then a few small users on its items"""
    ni = ni or n_u + 5
    cells = [(0, j, 0.0 if j % 5 == 3 else float(1 + j % 4) / 2.0) for j in range(n_u)]
    for u in range(1, 1 + others):
        cells += [(u, (u * 3) % n_u, 2.0), (u, ni - u, 1.5)]
    return 1 + others, ni, cells


def test_unit_of_one_cell():
    s = check_forms(2, 3, [(0, 1, 2.5), (1, 2, 1.0)], 4, 20270320)
    assert s["lds"]["levels"] == 1 and s["lds"]["widest"] == 2


@pytest.mark.parametrize("extra", [0, 1], ids=["block", "block+1"])
def test_unit_at_the_workgroup_size_and_one_past_it(extra):
    """exactly one pass of the item lanes, and a second pass of one lane: the uexp chain goes on across the pass border (the sum of
    the first pass alone, or a restart at 0.0 in the second, gives other bits: the restatement's chain is one)"""
    B = capi.lrmf_block()
    n_u = B + extra
    nu, ni, cells = one_big_user(n_u)
    m = lref.LRMF(nu, ni, cells)
    assert len(m.stored[0]) == n_u and m.columns[0][-1] == n_u - 1    # the last lane's exp is a term of the sum
    s = check_forms(nu, ni, cells, 3, 20270321 + extra, iters=2)
    assert s["lds"]["global_units"] == 0


def test_unit_one_past_the_lds_bound_switches_to_the_global_form():
    """k = 32: cmi_lrmf_lds_rows(32) cells keep their rows in LDS (the largest launch, all of the 160 KiB), one more leaves them in
    memory, and last_schedule counts that unit"""
    k = 32
    rows = capi.lrmf_lds_rows(k)
    assert 256 < rows < 1000
    nu, ni, cells = one_big_user(rows, ni=rows + 6)
    s = check_forms(nu, ni, cells, k, 20270330, forms=FORMS[:1], iters=1)
    assert s["lds"]["global_units"] == 0
    nu, ni, cells = one_big_user(rows + 1, ni=rows + 6)
    s = check_forms(nu, ni, cells, k, 20270331, forms=FORMS[:1], iters=1)
    assert s["lds"]["global_units"] == 1


# ---- the launch shapes of the schedule -------------------------------------------------------------------------------------------------
def test_wide_levels_several_workgroups_a_launch():
    """300 x 200, 10 cells a user, uniform: a user misses the 10 items of another with probability 0.59, so most levels hold two to
    four units, each launched as a grid of as many workgroups"""
    nu, ni, cells = uniform_cells()
    lv = lref.levels(nu, ni, cells)
    s = check_forms(nu, ni, cells, 10, 20270340, iters=2)["lds"]
    widths = np.bincount(lv)[1:]
    print("level widths", np.bincount(widths)[1:].tolist(), s)
    assert s["levels"] == len(widths) and s["widest"] == widths.max() >= 3
    assert s["alone"] == int(np.sum(widths > 1)) > s["levels"] // 2


def shared_item_cells(n=40):
    """n users on item 0, each with two items of its own besides"""
    cells = []
    for u in range(n):
        cells += [(u, 0, float(1 + u % 5)), (u, 1 + 2 * u, 2.0), (u, 2 + 2 * u, 0.0 if u % 4 == 0 else 3.0)]
    return n, 1 + 2 * n, cells


def test_forty_users_on_one_item_are_one_run():
    nu, ni, cells = shared_item_cells()
    s = check_forms(nu, ni, cells, 5, 20270341)["lds"]
    assert (s["levels"], s["alone"], s["runs"], s["widest"]) == (40, 0, 1, 1)


def mixed_cells():
    """blocks of 12 pairwise disjoint users (one level, a grid launch) between chains of 5 users on one hub item (a run each).  A
    chain's first user also stores an item of the block before it, so the chain comes after that block; its last user stores 12
    link items, one for every user of the next block, so that block comes after the chain and stays one level"""
    cells, u, j = [], 0, 0
    links = []
    for _ in range(3):
        first = j
        for t in range(12):
            cells += [(u, j, 2.0), (u, j + 1, 0.0 if t % 5 == 2 else 1.0)]
            if links:
                cells.append((u, links[t], 1.5))
            u, j = u + 1, j + 2
        hub, links = j, list(range(j + 1, j + 13))
        j += 13
        for n in range(5):
            cells += [(u, hub, 3.0), (u, j, 1.5)]
            if n == 0:
                cells.append((u, first, 0.5))
            if n == 4:
                cells += [(u, b, 2.5) for b in links]
            u, j = u + 1, j + 1
    return u, j, cells


def test_run_and_grid_launches_alternate():
    nu, ni, cells = mixed_cells()
    widths = np.bincount(lref.levels(nu, ni, cells))[1:].tolist()
    assert widths == [12, 1, 1, 1, 1, 1, 12, 1, 1, 1, 1, 1, 12, 1, 1, 1, 1, 1]
    s = check_forms(nu, ni, cells, 6, 20270342)["lds"]
    assert (s["levels"], s["alone"], s["runs"], s["widest"]) == (18, 3, 3, 12)


def test_two_units_whose_only_common_row_is_a_stored_zeros():
    """user 1 stores item 1 as a zero: the cell is no part of its uexp, but Q[1] is read and written, after user 0 has written it"""
    cells = [(0, 0, 3.0), (0, 1, 2.0), (1, 1, 0.0), (1, 2, 4.0), (1, 3, 1.0)]
    s = check_forms(2, 4, cells, 3, 20270343)["lds"]
    assert (s["levels"], s["runs"], s["alone"]) == (2, 1, 0)
    P0, Q0, ref = reference(2, 4, cells, 3, 20270343)
    assert not np.array_equal(ref[0][1][1], Q0[1])


# ---- the loss ---------------------------------------------------------------------------------------------------------------------------
def test_tree_loss_within_the_derived_bound_and_reproducible():
    """the fixed tree against the strict chain.  The terms have both signs (a stored-zero cell's log(B) can be positive), so each sum
    lies within n * 2^-53 * sum|term| of the exact one (first order) and the two within twice that of each other, n = cells (k + 1);
    two identical runs give identical bits"""
    k = 17
    nu, ni, cells = uniform_cells()
    P0, Q0, ref = reference(nu, ni, cells, k, 20270350, iters=2)
    outs = []
    for _ in range(2):
        h = instance(k, nu, ni, cells, P0, Q0, flags=0)
        losses = [h.iterate(LR, REG_U, REG_I) for _ in range(2)]
        outs.append((losses, h.model()))
        h.close()
    (la, (Pa, Qa)), (lb, (Pb, Qb)) = outs
    assert same_bits_exact(la, lb) and same_bits_exact(Pa, Pb) and same_bits_exact(Qa, Qb)
    assert same_bits_exact(Pa, ref[1][0]) and same_bits_exact(Qa, ref[1][1])
    n = len(cells) * (k + 1)
    for got, (_, _, strict, terms) in zip(la, ref):
        bound = 2 * n * 2.0 ** -53 * float(np.sum(np.abs(terms)))
        print("tree loss %r strict %r bound %r" % (got, strict, bound))
        assert len(terms) == n and abs(got - strict) <= bound


# ---- numeric failure ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,flag", FORMS, ids=[f[0] for f in FORMS])
def test_only_stored_zero_user_gives_e_numeric(form, flag):
    cells = [(0, 0, 2.0), (0, 1, 1.0), (1, 1, 0.0), (2, 2, 3.0)]
    rng = np.random.default_rng(20270360)
    P0, Q0 = rng.random((3, 4)), rng.random((3, 4))
    h = instance(4, 3, 3, cells, P0, Q0, flags=capi.LRMF_FLAG_STRICT | flag)
    with pytest.raises(capi.CmiError) as e:
        h.iterate(LR, REG_U, REG_I)
    assert e.value.code == capi.E_NUMERIC and "cmi_lrmf_iterate" in str(e.value)
    P, Q = P0.copy(), Q0.copy()
    loss, _ = lref.LRMF(3, 3, cells).epoch_np(P, Q, LR, REG_U, REG_I)
    assert loss == -np.inf
    gP, gQ = h.model()
    assert same_bits(gP, P) and same_bits(gQ, Q) and not np.all(np.isfinite(gP[1])) and np.all(np.isfinite(gP[[0, 2]]))
    h.close()


def test_pred_past_the_exp_range_gives_e_numeric():
    """P0 scaled so that pred > 710: exp(pred) = Inf, uexp = Inf, B = NaN"""
    cells = [(0, 0, 2.0), (0, 1, 1.0), (1, 1, 4.0), (1, 2, 3.0)]
    P0, Q0 = np.full((2, 4), 20.0), np.full((3, 4), 10.0)          # pred = 800
    h = instance(4, 2, 3, cells, P0, Q0)
    with pytest.raises(capi.CmiError) as e:
        h.iterate(LR, REG_U, REG_I)
    assert e.value.code == capi.E_NUMERIC
    P, Q = P0.copy(), Q0.copy()
    loss, _ = lref.LRMF(2, 3, cells).epoch_np(P, Q, LR, REG_U, REG_I)
    assert np.isnan(loss)
    gP, gQ = h.model()
    assert same_bits(gP, P) and same_bits(gQ, Q)
    h.close()


# ---- prediction, top-N, refusals ---------------------------------------------------------------------------------------------------------
def test_predict_batch_equals_row_mult():
    rng = np.random.default_rng(20270370)
    nu, ni, k = 9, 11, 17
    P, Q = rng.normal(size=(nu, k)), rng.normal(size=(ni, k))
    h = instance(k, nu, ni, [(0, 0, 1.0)], P, Q)
    tu, tj = all_tuples(nu, ni)
    assert same_bits_exact(h.predict(tu, tj).reshape(nu, ni), lref.scores(P.tolist(), Q.tolist()))
    h.close()


# (these golden models have k = 3 and 10; the evaluation's k range up to 128 is held in tests/test_gpu_topn_score_edges.py)
@pytest.mark.parametrize("name,seed", [("knn_matrix k=3", 11), ("knn_matrix k=10", 11)])
def test_eval_rankings_on_golden_models(name, seed):
    run = next(r for r in RUNS if r["name"] == name)
    h = instance(run["k"], run["n_users"], run["n_items"], run["cells"], run["iters"][-1]["P"], run["iters"][-1]["Q"])
    scores = run["predict"]
    with pytest.raises(capi.CmiError) as e:
        h.last_iter_ms()
    assert e.value.code == capi.E_INVALID
    train, test = contextual_split(run["cells"], 4, seed)
    for kw in (dict(bin_thold=-1.0, num_recs=10), dict(bin_thold=-1.0, num_recs=5, strategy="uc"), dict(bin_thold=0.05, num_recs=10, num_ignore=3)):
        check_rankings(h, scores, train, test, **kw)
    ms = h.last_iter_ms()
    assert ms[:2] == (0.0, 0.0) and ms[2] > 0.0
    h.close()


def test_refusals():
    h = capi.LRMFInstance(4, 5, 6)
    with pytest.raises(capi.CmiError) as e:
        h.iterate(0.1, 0.1, 0.1)
    assert e.value.code == capi.E_INVALID and "no ratings" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        h.set_ratings([0, 5], [0, 1], [1.0, 1.0])
    assert e.value.code == capi.E_INVALID and "out of range" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        h.set_ratings([0, 0], [1, 1], [1.0, 2.0])
    assert e.value.code == capi.E_INVALID and "duplicate" in str(e.value)
    h.set_ratings([0, 1], [0, 1], [1.0, 2.0])
    with pytest.raises(capi.CmiError) as e:
        h.iterate(0.1, 0.1, 0.1)
    assert e.value.code == capi.E_INVALID and "no model" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        h.predict([0], [0])
    assert e.value.code == capi.E_INVALID
    h.set_ratings([], [], [])                                        # the empty matrix: an iteration visits no cell
    h.set_model(np.ones((5, 4)), np.ones((6, 4)))
    assert h.iterate(0.1, 0.1, 0.1) == 0.0 and h.last_schedule()["levels"] == 0
    h.close()


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_driver_parity_depaul_two_folds(tmp_path):
    """cv -k 2 --rand-seed 1, num.max.iter = 3 with the bold driver: the printed measures equal those of capi.LRMFInstance driven by
    hand over the same folds, from the same P.init() / Q.init() draw"""
    import os
    import re
    import shutil
    import subprocess

    from carskit_amd import dao
    from oracle import oracle_np
    from tests import bpr_ref as bref
    from tests.hostmirror import splitter
    from tests.util import to2d

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    k, iters = 10, 3
    shutil.copyfile(os.path.join(root, "tests", "golden", "depaul_ratings_compact.csv"), tmp_path / "ratings.txt")
    conf = open(os.path.join(root, "tests", "golden", "depaul_setting.conf")).read().replace("PLACEHOLDER_SET_BY_TEST", str(tmp_path / "ratings.txt"))
    assert "num.max.iter=100" in conf and "num.factors=10" in conf and "cv -k 5 -p off --rand-seed 1" in conf and "-threshold -1" in conf
    assert "learn.rate=2e-2 -max -1 -bold-driver" in conf and "reg.lambda=0.0001 -c 0.001" in conf
    conf = conf.replace("recommender=biasedmf", "recommender=lrmf").replace("num.max.iter=100", "num.max.iter=%d" % iters)
    conf = conf.replace("-threshold -1", "-threshold 0").replace("cv -k 5", "cv -k 2")
    (tmp_path / "lrmf.conf").write_text(conf)
    p = subprocess.run([os.path.join(root, "carskit_amd", "bin", "carskit-mi355x"), "-c", str(tmp_path / "lrmf.conf"), "--precise"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    m = re.search(r"PRECISE LRMF folds=2 Pre10=(\S+) Rec10=(\S+) AUC10=(\S+) MAP10=(\S+) NDCG10=(\S+) MRR10=(\S+)", p.stdout)
    assert m and "Final Results by LRMF, Pre5: " in p.stdout, p.stdout[-500:]
    dao.transform(str(tmp_path / "ratings.txt"), str(tmp_path / "train.csv"))
    d = dao.DataDAO(str(tmp_path / "train.csv")).rating_data()
    labels, nf = splitter.split_folds(d.n, 2, 1)
    lr0, reg = float(np.float32(2e-2)), float(np.float32(1e-4))
    want = {}
    for f in range(1, nf + 1):
        tr, te = splitter.kth_fold(d, labels, f)
        u, i, r = to2d(tr.u, tr.j, tr.r)
        P, Q = bref.init_model(oracle_np.JavaRandom(1), d.n_users, d.n_items, k)
        h = capi.LRMFInstance(k, d.n_users, d.n_items, flags=capi.LRMF_FLAG_STRICT)
        h.set_ratings(u, i, r)
        h.set_model(P, Q)
        lrate, last_loss = lr0, 0.0
        for it in range(1, iters + 1):
            loss = h.iterate(lrate, reg, reg)
            assert abs(loss) >= 1e-5                                 # isConverged: not converged; then updateLRate's bold driver
            if it > 1:
                lrate = lrate * 1.05 if abs(last_loss) > abs(loss) else lrate * 0.5
            last_loss = loss
        res = h.eval_rankings((tr.u, tr.j, tr.ctx, tr.r), (te.u, te.j, te.ctx, te.r), bin_thold=0.0, num_recs=10)
        h.close()
        for name in ("Pre10", "Rec10", "AUC10", "MAP10", "NDCG10", "MRR10"):
            want[name] = want.get(name, 0.0) + res[name] / nf
    for g, name in zip(m.groups(), ("Pre10", "Rec10", "AUC10", "MAP10", "NDCG10", "MRR10")):
        print(name, g, want[name])
        assert abs(float(g) - want[name]) <= 1e-12, (name, g, want[name])
