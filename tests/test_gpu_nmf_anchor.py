"""The NMF training kernels at the instantiations, borders and values tests/test_gpu_nmf.py never launches, against the CPU restatement
(tests/nmf_ref.py) on the matrices of tests/nmf_fixtures.py, whose own conditions tests/test_nmf_ref.py holds on the CPU:

  (a) nmf_row_kernel<G> at k = 63, 127, 129, 192, 193 (the last lane masked; G = 3, partly masked and full; one factor in the top group) on
      a ladder of row lengths that takes every remainder of both look-ahead loops, in either phase, with negative values;
  (b) nmf_loss_final_kernel's second trip: 65 block partials with a full last block and with a last block of one cell, and exactly 64;
  (c) Inf, NaN, a zero item row and an overflowing e_t, each inside a component of the matrix that keeps it: E_NUMERIC, and the model the
      restatement's, NaN for NaN and every other double bit for bit.

W, H and the predictions are held bit for bit.  So is the loss, to the restatement of the kernels' own fixed order (nref.loss_tree), and
beside that to the strict chain within 2 n 2^-53 * loss, the bound that two orders of n non-negative terms allow."""
import numpy as np
import pytest

from carskit_amd import capi
from tests import nmf_fixtures as fx, nmf_ref as nref
from tests.util import same_bits, same_bits_exact

pytestmark = pytest.mark.gpu


def handle(m, k, W0, H0):
    h = capi.NMFInstance(k, m.nu, m.ni)
    h.set_ratings(m.u, m.i, m.r)
    h.set_model(W0, H0)
    return h


def check_run(m, k, W0, H0, steps, label):
    """every iteration's W and H bit for bit; the loss equal to the restated tree and within 2 n 2^-53 * loss of the strict chain"""
    h = handle(m, k, W0, H0)
    for it, s in enumerate(steps):
        loss = h.iterate()
        gW, gH = h.model()
        assert same_bits_exact(gW, s.W), (label, it, np.argwhere(gW != s.W)[:5])
        assert same_bits_exact(gH, s.Ht.T), (label, it, np.argwhere(gH != s.Ht.T)[:5])
        bound = 2 * len(m.r) * 2.0 ** -53 * s.chain
        assert same_bits_exact([loss], [s.tree]), (label, it, loss, s.tree)
        assert abs(loss - s.chain) <= bound, (label, it, loss, s.chain, bound)
    return h


@pytest.mark.parametrize("side", ["ladder_on_users", "ladder_on_items"])
@pytest.mark.parametrize("k", fx.ANCHOR_KS)
def test_every_instantiation_and_mask_on_the_ladder(k, side):
    transposed = side == "ladder_on_items"
    m = fx.ladder_matrix(transposed)
    W0, H0, steps = fx.ladder_run(k, transposed)
    h = check_run(m, k, W0, H0, steps, "k=%d %s" % (k, side))
    W, Ht = steps[-1].W, steps[-1].Ht
    rng = np.random.default_rng(k)
    tu, tj = rng.integers(0, m.nu, 500).astype(np.int32), rng.integers(0, m.ni, 500).astype(np.int32)
    want = nref.products(W, Ht, tu, tj)
    assert same_bits_exact(h.predict(tu, tj), want)
    assert (want > 5.0).any() and (want < 1.0).any()                                      # both sides of the bound are at work
    assert same_bits_exact(h.predict(tu, tj, True, 1.0, 5.0), np.where(want > 5.0, 5.0, np.where(want < 1.0, 1.0, want)))
    h.close()


@pytest.mark.parametrize("n_cells", fx.LOSS_CELLS)
def test_loss_borders(n_cells):
    W0, H0, steps = fx.loss_run(n_cells)
    check_run(fx.loss_matrix(n_cells), fx.LOSS_K, W0, H0, steps, "%d cells" % n_cells).close()


def test_contained_non_finite_and_degenerate_factors():
    m = fx.contained_matrix()
    W0, H0, steps = fx.contained_run()
    h = handle(m, fx.CONTAINED_K, W0, H0)
    for it, s in enumerate(steps):
        with pytest.raises(capi.CmiError) as e:
            h.iterate()
        assert e.value.code == capi.E_NUMERIC and "NaN" in str(e.value), it
        gW, gH = h.model()                                                                # the failed iteration is done all the same
        assert same_bits(gW, s.W), (it, np.argwhere(~((gW == s.W) | (np.isnan(gW) & np.isnan(s.W))))[:5])
        assert same_bits(gH, s.Ht.T), (it, np.argwhere(~((gH == s.Ht.T) | (np.isnan(gH) & np.isnan(s.Ht.T))))[:5])
        assert not gW[fx.OVERFLOW_USER].any() and not gH[:, fx.ZERO_ITEM].any()
        assert np.isnan(gW[fx.INF_USER]).any() and np.isnan(gH[:, fx.NAN_ITEM]).any()
    h.close()
