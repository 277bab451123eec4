"""tests/nmf_ref.py (the CPU restatement the GPU tests compare against) equals the run of the reference's own NMF source
(tests/golden/reference_nmf.json.gz, minted by tests/tools/mint_reference_nmf.py) bit for bit: W, H and the loss of every iteration,
the predictions, and initModel()'s draws.  Its restatement of the device's loss order (loss_cells, loss_tree) is pinned on inputs
where every order is exact and on inputs where only the device's order gives the expected double.  The fixtures of
tests/test_gpu_nmf_anchor.py (tests/nmf_fixtures.py) are held to their conditions here, without a GPU."""
import numpy as np
import pytest

from tests import nmf_fixtures as fx, nmf_ref as nref
from tests.hostmirror.javarand import JavaRandom
from tests.util import same_bits_exact


def test_iterations_and_predictions_match_the_reference_run():
    runs = nref.golden_runs()
    assert [r["name"] for r in runs] == ["knn_matrix k=3", "knn_matrix k=10", "handmade k=2"]
    for run in runs:
        nu, ni = run["n_users"], run["n_items"]
        rows, cols = nref.rows_of(run["u"], run["i"], run["r"], nu), nref.cols_of(run["u"], run["i"], run["r"], ni)
        W, Ht = run["W0"].copy(), np.ascontiguousarray(run["H0"].T)
        assert len(run["iters"]) == 3
        for n, it in enumerate(run["iters"]):
            loss = nref.iterate(W, Ht, rows, cols)
            assert same_bits_exact(W, it["W"]), (run["name"], n)
            assert same_bits_exact(Ht.T, it["H"]), (run["name"], n)
            assert same_bits_exact([loss], [it["loss"]]), (run["name"], n, loss, it["loss"])
        lo, hi = run["min_rate"], run["max_rate"]
        pred = [[nref.predict(W, Ht, u, j) for j in range(ni)] for u in range(nu)]
        bounded = [[nref.predict(W, Ht, u, j, True, lo, hi) for j in range(ni)] for u in range(nu)]
        assert same_bits_exact(pred, run["predict"]) and same_bits_exact(bounded, run["predict_bounded"]), run["name"]
        assert (run["predict"] < lo).any()           # the bound is at work


def test_rows_without_entries_stay_and_updates_move_the_rest():
    run = nref.golden_runs()[2]                      # handmade: user 5 has no ratings
    it = run["iters"][0]
    assert same_bits_exact(it["W"][5], run["W0"][5]) and not same_bits_exact(it["W"][0], run["W0"][0])


def test_init_model_draws():
    g = nref.golden()["init"]
    nu, ni, k = g["n_users"], g["n_items"], g["k"]
    W, Ht = nref.init_model(JavaRandom(g["seed"]), nu, ni, k)
    assert same_bits_exact(W, nref.unhex(g["W"], nu, k))
    assert same_bits_exact(Ht.T, nref.unhex(g["H"], k, ni))
    assert 0.0 <= W.min() and W.max() < 0.01


# ---- the device's loss order, restated --------------------------------------------------------------------------------------------------
def strict(terms):
    s = 0.0
    for t in np.asarray(terms).tolist():
        s += t
    return s * 0.5


def loss_bound(n, loss):
    """two orders of a sum of n non-negative doubles are each within a relative (n - 1) 2^-53 of the exact sum (to first order), hence
    within 2 n 2^-53 * loss of each other: the bound tests/test_gpu_nmf.py holds the device's loss to"""
    return 2 * n * 2.0 ** -53 * loss


def test_loss_tree_is_the_strict_chain_where_every_order_is_exact():
    rng = np.random.default_rng(7)
    for n in (0, 1, 63, 64, 65, 255, 256, 257, 1000, 16384, 16385, 16640):
        cells = rng.integers(0, 1000, n).astype(np.float64)          # every partial sum an integer below 2^53: no rounding anywhere
        assert len(nref.loss_partials(cells)) == -(-n // 256)
        assert nref.loss_tree(cells) == strict(cells) == cells.sum() * 0.5, n
    marks = np.zeros(600)
    marks[[0, 255, 256, 599]] = [1.0, 2.0, 4.0, 8.0]                 # the cells of a block stay in it, the last block is padded
    assert nref.loss_partials(marks).tolist() == [3.0, 4.0, 8.0]


def test_loss_tree_folds_a_wave_in_halves_and_the_waves_in_order():
    """2^53 + 1 + 1 is 2^53 + 2 only where the two ones meet first: an order that is not the device's gives another double"""
    big = 2.0 ** 53
    wave = np.zeros(64)
    wave[[0, 1, 33]] = [big, 1.0, 1.0]             # fold 32 adds lane 33 to lane 1 (2.0); fold 1 adds that to lane 0: big + 2
    assert nref.loss_tree(wave) * 2 == big + 2.0 and strict(wave) * 2 == big
    wave[[1, 33, 32]] = [0.0, 1.0, 1.0]            # lane 32 meets lane 0 in the first fold and is lost: big, then + 1 is lost too
    assert nref.loss_tree(wave) * 2 == big
    block = np.zeros(256)
    block[[0, 64, 128]] = [big, 1.0, 1.0]          # (w0 + w1) + w2: each 1 is lost on its own
    assert nref.loss_tree(block) * 2 == big
    block[[0, 64, 128]] = [1.0, 1.0, big]          # (1 + 1) + big
    assert nref.loss_tree(block) * 2 == big + 2.0
    two = np.zeros(512)
    two[[0, 256, 257]] = [big, 1.0, 1.0]           # the ones of the second block meet in its tree before the chain takes the partial
    assert nref.loss_tree(two) * 2 == big + 2.0


def test_loss_cells_keep_the_place_of_a_cell_that_is_not_positive():
    m = fx.ladder_matrix()
    _, _, steps = fx.ladder_run(63)
    cells, terms = steps[0].cells, nref.loss_terms(steps[0].W, steps[0].Ht, m.rows)
    r = np.concatenate([val for _, val in m.rows])
    assert len(cells) == len(m.r) and same_bits_exact(cells[r > 0], terms) and not cells[r < 0].any() and (cells[r > 0] > 0).all()
    assert steps[0].chain == strict(cells) == nref.loss_of(steps[0].W, steps[0].Ht, m.rows)      # + 0.0 changes no non-negative sum


def all_runs():
    for t in (False, True):
        for k in fx.ANCHOR_KS:
            yield "ladder k=%d transposed=%s" % (k, t), fx.ladder_matrix(t), fx.ladder_run(k, t)
    for n in fx.LOSS_CELLS:
        yield "loss %d cells" % n, fx.loss_matrix(n), fx.loss_run(n)


def test_loss_tree_is_within_the_derived_bound_of_the_strict_chain_on_the_fixtures():
    for name, m, (_, _, steps) in all_runs():
        for s in steps:
            assert np.isfinite(s.W).all() and np.isfinite(s.Ht).all() and s.chain > 0, name
            assert abs(s.tree - s.chain) <= loss_bound(len(m.r), s.chain), (name, s.tree, s.chain)


# ---- the fixtures of tests/test_gpu_nmf_anchor.py: what they hold, and that each can see the fault it is there for ----------------------
def test_ladder_matrix_has_the_ladder_on_either_side():
    for t in (False, True):
        m = fx.ladder_matrix(t)
        ladder = [len(x[0]) for x in (m.cols if t else m.rows)]
        assert ladder == list(range(1, 18)) + [63, 64, 65, 127, 128, 129]
        assert {n % 4 for n in ladder} == set(range(4)) and {n % 8 for n in ladder[:17]} == set(range(8))
        assert (m.nu, m.ni) == ((140, 23) if t else (23, 140)) and len(m.r) == sum(ladder) and (m.r != 0).all()
        assert 1 / 9 < np.mean(m.r < 0) < 1 / 5                      # about one value in seven is negative
        assert min(np.count_nonzero(val < 0) for _, val in (m.cols if t else m.rows)[17:]) >= 3


def test_loss_matrices_have_the_borders():
    for n, blocks, last in zip(fx.LOSS_CELLS, (65, 65, 64), (256, 1, 256)):
        m = fx.loss_matrix(n)
        _, _, steps = fx.loss_run(n)
        assert len(m.r) == len(steps[0].cells) == n and len(nref.loss_partials(steps[0].cells)) == blocks
        assert n - 256 * (blocks - 1) == last
        r = np.concatenate([val for _, val in m.rows])
        assert (r[6::7] < 0).all() and (np.delete(r, np.arange(6, n, 7)) > 0).all()      # every seventh value, in CRS order
    full, cut = fx.loss_matrix(16640), fx.loss_matrix(16384)
    assert same_bits_exact(full.r[:16384], cut.r) and (full.u[:16384] == cut.u).all() and (full.i[:16384] == cut.i).all()


def w_phase_without(k, dropped):
    """the first W phase on the ladder matrix by a row kernel that leaves the factors `dropped` out of step 2's two sums (a lane-per-
    factor group masked or dispatched wrongly); step 1's e_t is whole"""
    m = fx.ladder_matrix()
    W0, H0, _ = fx.ladder_run(k)
    W, Ht = W0.copy(), np.ascontiguousarray(H0.T)
    Hcut = Ht.copy()
    Hcut[:, dropped] = 0.0
    for u, (idx, val) in enumerate(m.rows):
        part, e = Hcut[idx], nref.products(W[[u] * len(idx)], Ht, np.arange(len(idx)), idx)
        real, estm = np.zeros(k), np.zeros(k)
        for t in range(len(idx)):
            real = real + val[t] * part[t]
            estm = estm + e[t] * part[t]
        W[u] = W[u] * (real / (estm + nref.EPS))
    return W


@pytest.mark.parametrize("k,dropped", [(129, slice(128, None)), (193, slice(192, None)), (129, slice(0, 0))], ids=["k129", "k193", "none"])
def test_ladder_sees_a_factor_group_left_out_of_step_two(k, dropped):
    want = fx.ladder_run(k)[2][0].W
    got = w_phase_without(k, dropped)
    if dropped == slice(0, 0):
        assert same_bits_exact(got, want)                            # nothing left out: the helper is the restatement
    else:
        assert same_bits_exact(got[:, :128], want[:, :128]) and not same_bits_exact(got, want)
        assert (got[:, dropped] != want[:, dropped]).all()           # every row of W shows it


def test_65_partials_see_a_final_chain_that_stops_after_64():
    for n in fx.LOSS_CELLS[:2]:
        for s in fx.loss_run(n)[2]:
            parts = nref.loss_partials(s.cells)
            assert len(parts) == 65 and parts[64] > 0
            assert strict(parts[:64]) != s.tree == strict(parts), n


def test_negative_cells_in_the_loss_would_break_the_bound():
    for name, m, (_, _, steps) in all_runs():
        r = np.concatenate([val for _, val in m.rows])
        u = np.concatenate([np.full(len(idx), a) for a, (idx, _) in enumerate(m.rows)])
        j = np.concatenate([idx for idx, _ in m.rows])
        for s in steps:
            e = nref.products(s.W, s.Ht, u, j) - r
            assert abs(strict(e * e) - s.chain) > 1e6 * loss_bound(len(r), s.chain), name


def test_a_loss_fixture_sees_negative_cells_compressed_out_before_the_tree():
    """a kernel that dropped the cells without r > 0 (as loss_terms does) instead of giving them a lane that adds + 0.0 would put every
    later term at another place of the tree: the same sum within the bound, other bits"""
    seen = []
    for n in fx.LOSS_CELLS:
        for it, s in enumerate(fx.loss_run(n)[2]):
            r = np.concatenate([val for _, val in fx.loss_matrix(n).rows])
            if nref.loss_tree(s.cells[r > 0]) != s.tree:
                seen.append((n, it))
    assert seen


def test_contained_fixture_keeps_what_is_injected_inside_its_component():
    m = fx.contained_matrix()
    W0, H0, steps = fx.contained_run()
    k, ladder = fx.CONTAINED_K, fx.ladder_matrix()
    assert (m.nu, m.ni) == (ladder.nu + 4, ladder.ni + 6)
    assert [len(x[0]) for x in m.rows] == [len(x[0]) for x in ladder.rows] + [3] * 4
    assert all(idx.tolist() == [140, 141, 142] for idx, _ in m.rows[23:25]) and all(idx.tolist() == [143, 144, 145] for idx, _ in m.rows[25:])
    assert all(len(x[0]) == 2 for x in m.cols[140:]) and max(idx.max() for idx, _ in m.rows[:23]) < 140
    assert (fx.INF_USER, fx.NAN_ITEM, fx.OVERFLOW_USER, fx.ZERO_ITEM) == (23, 141, 25, 144)
    assert np.isinf(W0[23]).sum() == 1 and np.isnan(H0[:, 141]).sum() == 1 and not H0[:, 144].any()
    assert np.isfinite(W0[25]).all() and np.isfinite(np.delete(W0, 23, 0)).all() and np.isfinite(np.delete(H0, 141, 1)).all()
    # the overflow row, in the restatement: e_t is Inf at its first item, 0.0 at the zero item and finite above 1e308 at the third, so
    # estm is Inf for every factor
    idx, val = m.rows[25]
    with np.errstate(all="ignore"):
        e = nref.products(W0[[25] * 3], H0.T, np.arange(3), idx)
        estm = np.zeros(k)
        for t in range(3):
            estm = estm + e[t] * H0[:, idx[t]]
    assert e[0] == np.inf and e[1] == 0.0 and 1e308 < e[2] < np.inf and (estm == np.inf).all()
    for s in steps:
        assert not s.W[25].any() and not np.signbit(s.W[25]).any() and not s.Ht[144].any()
        bad_w, bad_h = ~np.isfinite(s.W).all(1), ~np.isfinite(s.Ht).all(1)
        assert np.flatnonzero(bad_w).tolist() == [23, 24] and np.flatnonzero(bad_h).tolist() == [140, 141, 142]
        assert 2 <= bad_w.sum() <= 0.1 * m.nu and 2 <= bad_h.sum() <= 0.1 * m.ni
        assert np.isnan(s.chain) and np.isnan(s.tree)
    assert not same_bits_exact(steps[0].W[26], steps[1].W[26])       # the rest of component B goes on moving
