"""BPR on the GPU: the golden runs of the reference through the C ABI, the device probes of java_math.hpp against the host's, the
device sampler against the host walk (edges, powers of two, block borders, the fallbacks), the level epoch against tests/bpr_ref.py,
the two loss forms, and the top-N evaluation."""
import functools

import numpy as np
import pytest

from carskit_amd import capi
from tests import bpr_ref as bref
from tests.test_bpr_capi_cpu import cols, edge_cells, pow2_cells
from tests.test_gpu_rankals import all_tuples, check_rankings, contextual_split, edge_matrix
from tests.util import same_bits_exact

pytestmark = pytest.mark.gpu

RUNS = bref.golden_runs()
LR, REG_U, REG_I = 0.05, float(np.float32(0.02)), float(np.float32(0.03))    # distinct, loud regularisation


def instance(k, nu, ni, cells, P=None, Q=None, flags=capi.BPR_FLAG_STRICT, state=None):
    h = capi.BPRInstance(k, nu, ni, flags=flags)
    h.set_ratings(*cols(cells))
    if P is not None:
        h.set_model(P, Q)
    if state is not None:
        h.set_random_state(state)
    return h


@pytest.mark.parametrize("run", RUNS, ids=[r["name"] for r in RUNS])
def test_golden_runs_match_the_reference_run(run):
    nu, ni = run["n_users"], run["n_items"]
    h = instance(run["k"], nu, ni, run["cells"], run["P0"], run["Q0"], state=bref.random_state(run["seed"]))
    for n, it in enumerate(run["iters"]):
        u, i, j, after = h.sample()                                  # the iteration's triples; the stream state stays
        assert list(zip(u.tolist(), i.tolist(), j.tolist())) == it["triples"] and after == it["state"], n
        loss = h.iterate(run["lrate"], run["reg_u"], run["reg_i"])
        P, Q = h.model()
        assert same_bits_exact(P, it["P"]), (n, np.argwhere(P != it["P"])[:5])
        assert same_bits_exact(Q, it["Q"]), (n, np.argwhere(Q != it["Q"])[:5])
        assert same_bits_exact([loss], [it["loss"]]), (n, loss, it["loss"])
        assert h.random_state() == it["state"]
    tu, tj = all_tuples(nu, ni)
    assert same_bits_exact(h.predict(tu, tj).reshape(nu, ni), run["predict"])
    ms = h.last_iter_ms()
    assert len(ms) == 5 and all(x >= 0.0 for x in ms) and sum(ms[:4]) > 0.0
    h.close()


@pytest.mark.parametrize("bound", [1, 2, 64, 60, (1 << 30) + 1])
def test_device_next_int_equals_the_host(bound):
    n = 5000
    st = bref.random_state(20261230 + bound)
    hv, hs = capi.java_next_ints(st, bound, n)
    dv, ds = capi.java_next_ints(st, bound, n, on_device=True)
    assert np.array_equal(hv, dv) and hs == ds
    r = bref.JavaStream(st)
    assert dv.tolist() == [r.next_int(bound) for _ in range(n)] and ds == r.state
    if bound == (1 << 30) + 1:
        assert r.draws > n + n // 4                                  # the rejection branch was taken, about once a value


def test_device_exp_log_equal_the_host():
    inf, nan = float("inf"), float("nan")
    xs = np.concatenate([np.random.default_rng(20261231).uniform(-40.0, 40.0, 50000),
                         np.random.default_rng(20261232).uniform(-750.0, 720.0, 20000),
                         [0.0, -0.0, inf, -inf, nan, 709.782712893384, 709.7827128933841, -745.1332191019411, -745.1332191019412, -710.0,
                          1e-10, -1e-10, 0.3, -0.3, 0.4, 1.0, -1.0, 1.03, 5e-324, 1e-310, 2.2250738585072014e-308, -2.5, 1e300]])
    he, hl = capi.java_exp_log(xs)
    de, dl = capi.java_exp_log(xs, on_device=True)
    for a, b in ((he, de), (hl, dl)):
        assert np.array_equal(np.isnan(a), np.isnan(b))              # where a NaN stands, not which NaN
        ok = ~np.isnan(a)
        assert same_bits_exact(a[ok], b[ok])


def sampled(h, on_device):
    u, i, j, st = h.sample(on_device=on_device)
    return list(zip(u.tolist(), i.tolist(), j.tolist())), st


def test_device_sampler_edges_empty_single_and_nearly_full_user():
    """37 x 60 with an empty user, a one-entry user, a stored-zero user and a user holding 59 of 60 items, whose contains() runs are
    long: either the draw cap's overflow sent the iteration to the host walk (counted) or the device list carried it"""
    nu, ni, cells = edge_cells()
    h = instance(4, nu, ni, cells, flags=0, state=bref.random_state(20270101))
    fell = 0
    for _ in range(4):                                               # four iterations' worth, on one continued stream
        before = h.last_schedule()["sampler_fallbacks"]
        dev, dst = sampled(h, True)
        host, hst = sampled(h, False)                                # the host form is no fallback: it never counts
        assert dev == host and dst == hst
        fell += h.last_schedule()["sampler_fallbacks"] - before
        h.set_random_state(hst)
    print("37 x 60: the device list carried %d iterations, the overflow fallback took %d" % (4 - fell, fell))
    users = {t[0] for t in host}
    assert 0 not in users and 3 not in users and {1, 2} <= users
    assert any(t[0] == 2 and t[2] != 31 for t in host)               # contains() misses entries of the long row: not only the item it lacks
    h.close()


def test_device_sampler_power_of_two_bounds():
    nu, ni, cells = pow2_cells()
    h = instance(4, nu, ni, cells, flags=0, state=bref.random_state(20270102))
    dev, dst = sampled(h, True)
    host, hst = sampled(h, False)
    assert dev == host and dst == hst and h.last_schedule()["sampler_fallbacks"] == 0
    h.close()


@functools.lru_cache(maxsize=None)
def long_cells():
    """700 x 300: 70 000 samples, a list several ranking blocks long"""
    rng = np.random.default_rng(20270103)
    cells = []
    for u in range(700):
        if u % 50 == 7:
            continue                                                 # some empty users
        for j in rng.choice(300, size=1 + (u * 3) % 40, replace=False):
            cells.append((u, int(j), float(1 + (u + j) % 5)))
    return 700, 300, cells


def test_device_sampler_across_ranking_blocks():
    nu, ni, cells = long_cells()
    st = bref.random_state(20270104)
    h = instance(4, nu, ni, cells, flags=0, state=st)
    dev, dst = sampled(h, True)
    host, hst = sampled(h, False)
    assert dev == host and dst == hst and h.last_schedule()["sampler_fallbacks"] == 0
    # from the exported block constant: where every sample's draws lie in the stream
    B = capi.lib().cmi_bpr_rank_block()
    m, r = bref.BPR(nu, ni, cells), bref.JavaStream(st)
    starts, ends = [], []
    for t in host:
        starts.append(r.draws)
        assert m.sample(r) == t
        ends.append(r.draws - 1)
    assert r.state == hst
    assert ends[-1] // B >= 3                                        # the list crosses block borders
    assert any(a // B != b // B for a, b in zip(starts, ends))       # and a sample's draws straddle one
    h.close()


def test_device_sampler_with_minimal_slack_falls_back_to_the_host_walk():
    """3 draws a sample reserved and no more: the last sample may start up to two positions late and still lie inside the reservation,
    so the third redraw of an iteration makes the list leave it (6 400 samples over rows that hold up to 19 of 128 items redraw far
    more often than that)"""
    nu, ni, cells = pow2_cells()
    h = instance(4, nu, ni, cells, flags=capi.BPR_FLAG_MIN_SLACK, state=bref.random_state(20270102))
    dev, dst = sampled(h, True)
    host, hst = sampled(h, False)
    assert dev == host and dst == hst and h.last_schedule()["sampler_fallbacks"] == 1
    h.close()


def test_device_sampler_draw_cap_overflow_falls_back_to_the_host_walk():
    """3 x 513: user 0 holds 512 of the 513 items, a power of two, so contains() finds every one of them and a j draw is accepted once
    in 513: most of its samples take more than the 255 draws a device lane may consume.  The overflow mark on the list sends the
    iteration to the host walk, which is counted; the triples are the restatement's"""
    nu, ni = 3, 513
    cells = [(0, j, 1.0 + j % 5) for j in range(512)] + [(1, 7, 2.0), (1, 300, 4.0), (2, 512, 3.0)]
    st = bref.random_state(20270105)
    m, r = bref.BPR(nu, ni, cells), bref.JavaStream(st)
    assert all(m.found[0][:512]) and not m.found[0][512]
    want, longest = [], 0
    for _ in range(nu * 100):
        d0 = r.draws
        want.append(m.sample(r))
        longest = max(longest, r.draws - d0)
    assert longest > 255                                             # a sample on the list is past the cap
    h = instance(4, nu, ni, cells, flags=0, state=st)
    dev, dst = sampled(h, True)
    assert dev == want and dst == r.state and h.last_schedule()["sampler_fallbacks"] == 1
    assert all(t[2] == 512 for t in dev if t[0] == 0)
    P0, Q0 = np.random.default_rng(1).random((nu, 4)), np.random.default_rng(2).random((ni, 4))
    h.set_model(P0, Q0)
    h.iterate(LR, REG_U, REG_I)                                      # an iteration falls back the same way, and goes on from there
    assert h.last_schedule()["sampler_fallbacks"] == 2 and h.random_state() == r.state
    P, Q = P0.copy(), Q0.copy()
    bref.epoch_by_levels(P, Q, want, LR, REG_U, REG_I)
    gP, gQ = h.model()
    assert same_bits_exact(gP, P) and same_bits_exact(gQ, Q)
    h.close()


# ---- the epoch ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def epoch_reference(k):
    """two iterations of the restatement on the 300 x 260 edge matrix: per iteration (P, Q, strict loss, terms, state)"""
    nu, ni, cells = edge_matrix()
    rng = np.random.default_rng(20270110 + k)
    P0, Q0 = rng.random((nu, k)), rng.random((ni, k))
    st = bref.random_state(20270111)
    u, i, j, after = capi.bpr_sample_host(nu, ni, *cols(cells), st, nu * 100)     # the host walk, equal to the restatement's (CPU tests)
    P, Q = P0.copy(), Q0.copy()
    out = []
    for _ in range(2):
        tri = list(zip(u.tolist(), i.tolist(), j.tolist()))
        loss, terms = bref.epoch_by_levels(P, Q, tri, LR, REG_U, REG_I)
        out.append((P.copy(), Q.copy(), loss, terms, after, tri))
        u, i, j, after = capi.bpr_sample_host(nu, ni, *cols(cells), after, nu * 100)
    return P0, Q0, st, out


@pytest.mark.parametrize("k", [1, 16, 17, 128])
def test_epoch_matches_the_restatement(k):
    nu, ni, cells = edge_matrix()
    P0, Q0, st, ref = epoch_reference(k)
    h = instance(k, nu, ni, cells, P0, Q0, state=st)
    for n, (P, Q, loss, _, after, tri) in enumerate(ref):
        got = h.iterate(LR, REG_U, REG_I)
        gP, gQ = h.model()
        assert same_bits_exact(gP, P), (n, np.argwhere(gP != P)[:5])
        assert same_bits_exact(gQ, Q), (n, np.argwhere(gQ != Q)[:5])
        assert same_bits_exact([got], [loss]), (n, got, loss)
        assert h.random_state() == after
        s = h.last_schedule()
        lv = bref.levels(nu, ni, tri)
        assert s["levels"] == max(lv) and s["widest"] == np.bincount(lv).max()
        assert s["alone"] >= 1 and s["runs"] >= 1, s                 # both launch shapes: a level alone and a run of narrow levels
        widths = np.bincount(lv)[1:]
        assert s["alone"] == int(np.sum(widths > 16))
        narrow = widths <= 16
        assert s["runs"] == int(np.sum(narrow[1:] & ~narrow[:-1]) + narrow[0])
        assert np.any(narrow[1:] & narrow[:-1])                      # a run holds more than one level
    h.close()


def test_default_loss_within_the_derived_bound_and_reproducible():
    """the fixed tree against the strict chain: every term is >= 0, so both lie within n * 2^-53 * loss of the exact sum (first
    order), and within 2 * n * 2^-53 * loss of each other, n = S (k + 1); two identical runs give identical bits"""
    k = 17
    nu, ni, cells = edge_matrix()
    P0, Q0, st, ref = epoch_reference(k)
    outs = []
    for _ in range(2):
        h = instance(k, nu, ni, cells, P0, Q0, flags=0, state=st)
        losses = [h.iterate(LR, REG_U, REG_I) for _ in range(2)]
        outs.append((losses, h.model(), h.random_state()))
        assert h.last_schedule()["sampler_fallbacks"] == 0           # the device sampler carried both iterations
        h.close()
    (la, (Pa, Qa), sa), (lb, (Pb, Qb), sb) = outs
    assert same_bits_exact(la, lb) and same_bits_exact(Pa, Pb) and same_bits_exact(Qa, Qb) and sa == sb
    assert same_bits_exact(Pa, ref[1][0]) and same_bits_exact(Qa, ref[1][1]) and sa == ref[1][4]
    n = nu * 100 * (k + 1)
    for got, (_, _, strict, terms, _, _) in zip(la, ref):
        assert np.all(terms >= 0.0)
        print("default loss %r strict %r bound %r" % (got, strict, 2 * n * 2.0 ** -53 * strict))
        assert abs(got - strict) <= 2 * n * 2.0 ** -53 * strict


def test_host_sampler_flag_gives_the_same_run():
    k = 16
    nu, ni, cells = edge_matrix()
    P0, Q0, st, ref = epoch_reference(k)
    h = instance(k, nu, ni, cells, P0, Q0, flags=capi.BPR_FLAG_STRICT | capi.BPR_FLAG_HOST_SAMPLER, state=st)
    loss = h.iterate(LR, REG_U, REG_I)
    P, Q = h.model()
    assert same_bits_exact(P, ref[0][0]) and same_bits_exact(Q, ref[0][1]) and same_bits_exact([loss], [ref[0][2]])
    assert h.last_schedule()["sampler_fallbacks"] == 0               # chosen, not fallen back to
    h.sample(on_device=True)                                         # the device form is switched off on this handle: the host walk
    assert h.last_schedule()["sampler_fallbacks"] == 0               # answers, and nothing fell back
    h.close()


# ---- top-N and refusals ---------------------------------------------------------------------------------------------------------------
# (these golden models have k = 2, 3 and 10; the evaluation's k range up to 128 is held in tests/test_gpu_topn_score_edges.py)
@pytest.mark.parametrize("name,seed", [("knn_matrix k=3", 11), ("knn_matrix k=10", 11), ("handmade k=2", 14)])
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
    assert ms[:4] == (0.0, 0.0, 0.0, 0.0) and ms[4] > 0.0
    h.close()


def test_refusals():
    h = capi.BPRInstance(4, 5, 6)
    with pytest.raises(capi.CmiError) as e:
        h.iterate(0.1, 0.1, 0.1)
    assert e.value.code == capi.E_INVALID and "no ratings" in str(e.value)
    with pytest.raises(capi.CmiError) as e:
        h.set_ratings([0] * 6, list(range(6)), [1.0] * 6)            # a user who holds every item
    assert e.value.code == capi.E_INVALID and "holds every item" in str(e.value)
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
        h.set_random_state(1 << 48)
    assert e.value.code == capi.E_INVALID
    with pytest.raises(capi.CmiError) as e:
        h.predict([0], [0])
    assert e.value.code == capi.E_INVALID
    h.close()


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_driver_parity_depaul(tmp_path):
    """cv -k 5 --rand-seed 1, num.max.iter = 3 with the bold driver.  The reference's first Recommender constructor seeds happy.coding's
    Randoms again after the splitter has drawn (Recommender.java:194-234 under resetStatics, CARSKit.java:150, 393-399), so fold 1
    samples from the seed's own state and folds 2..5 go on where the fold before stopped: the run equals the restatement over the same
    folds on that stream; --save-model leaves the last fold's P and Q"""
    import os
    import re
    import shutil
    import subprocess

    from carskit_amd import dao
    from oracle import oracle_np, rank_oracle
    from tests.hostmirror import splitter
    from tests.util import to2d

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    k, iters = 10, 3
    shutil.copyfile(os.path.join(root, "tests", "golden", "depaul_ratings_compact.csv"), tmp_path / "ratings.txt")
    conf = open(os.path.join(root, "tests", "golden", "depaul_setting.conf")).read().replace("PLACEHOLDER_SET_BY_TEST", str(tmp_path / "ratings.txt"))
    assert "num.max.iter=100" in conf and "num.factors=10" in conf and "cv -k 5 -p off --rand-seed 1" in conf and "-threshold -1" in conf
    assert "learn.rate=2e-2 -max -1 -bold-driver" in conf and "reg.lambda=0.0001 -c 0.001" in conf
    conf = conf.replace("recommender=biasedmf", "recommender=bpr").replace("num.max.iter=100", "num.max.iter=%d" % iters)
    conf = conf.replace("-threshold -1", "-threshold 0").replace("-verbose off", "-verbose off --save-model").replace("-p off", "-p on")
    (tmp_path / "bpr.conf").write_text(conf)                         # `-p on`: BPR's folds still run in sequence
    p = subprocess.run([os.path.join(root, "carskit_amd", "bin", "carskit-mi355x"), "-c", str(tmp_path / "bpr.conf"), "--precise"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    m = re.search(r"PRECISE BPR folds=5 Pre10=(\S+) Rec10=(\S+) AUC10=(\S+) MAP10=(\S+) NDCG10=(\S+) MRR10=(\S+)", p.stdout)
    assert m and "Final Results by BPR, Pre5: " in p.stdout, p.stdout[-500:]
    dao.transform(str(tmp_path / "ratings.txt"), str(tmp_path / "train.csv"))
    d = dao.DataDAO(str(tmp_path / "train.csv")).rating_data()
    labels, nf = splitter.split_folds(d.n, 5, 1)
    state = bref.random_state(1)                                     # new java.util.Random(1): the splitter's draws are forgotten
    lr0, reg = float(np.float32(2e-2)), float(np.float32(1e-4))
    want = {}
    for f in range(1, nf + 1):
        tr, te = splitter.kth_fold(d, labels, f)
        u, i, r = to2d(tr.u, tr.j, tr.r)
        P, Q = bref.init_model(oracle_np.JavaRandom(1), d.n_users, d.n_items, k)
        lrate, last_loss = lr0, 0.0
        for it in range(1, iters + 1):
            su, si, sj, state = capi.bpr_sample_host(d.n_users, d.n_items, u, i, r, state, d.n_users * 100)
            loss, _ = bref.epoch_by_levels(P, Q, list(zip(su.tolist(), si.tolist(), sj.tolist())), lrate, reg, reg)
            assert abs(loss) >= 1e-5                                 # isConverged: not converged; then updateLRate's bold driver
            if it > 1:
                lrate = lrate * 1.05 if abs(last_loss) > abs(loss) else lrate * 0.5
            last_loss = loss
        scores = bref.scores(P.tolist(), Q.tolist())
        tup = lambda x: list(zip(x.u.tolist(), x.j.tolist(), x.ctx.tolist(), x.r.tolist()))  # noqa: E731
        res, _ = rank_oracle.eval_rankings(lambda a, b, c: float(scores[a, b]), tup(tr), tup(te), bin_thold=0.0, num_recs=10)
        for name in ("Pre10", "Rec10", "AUC10", "MAP10", "NDCG10", "MRR10"):
            want[name] = want.get(name, 0.0) + res[name] / nf
    for g, name in zip(m.groups(), ("Pre10", "Rec10", "AUC10", "MAP10", "NDCG10", "MRR10")):
        print(name, g, want[name])
        assert abs(float(g) - want[name]) <= 1e-12, (name, g, want[name])
    saved = tmp_path / "CARSKit.Workspace" / "BPR" / ("model fold [%d].cmi" % nf)          # the last fold's model: the stream reached it
    assert saved.exists(), os.listdir(tmp_path / "CARSKit.Workspace")
    pmf = capi.Instance("PMF", k, d.n_users, d.n_items, 0, flags=capi.FLAG_STATE_F64)
    pmf.load_model(str(saved))
    assert same_bits_exact(pmf.get_state("P").reshape(P.shape), P) and same_bits_exact(pmf.get_state("Q").reshape(Q.shape), Q)
    pmf.close()
