"""The two RankALS solves where the staged chunk is not RANKALS_CHUNK entries: per = min(RANKALS_CHUNK, stage / k) is 60 at k = 17, 32 at
k = 32 and 33 at k = 33 (and 64 at k = 8, inversion width 16).  On the per-border matrices of tests/rankals_fixtures.py a row and a column
of exactly per, per + 1 and 2 per entries meet each of them, and both moment kernels end on a full tile of RANKALS_TILE users and items
(conditions held on the CPU by tests/test_rankals_ref.py).  P and Q bit for bit against the restatement after one and two iterations.
The inversion layouts of these and the other widths alone: test_inversion_batch_matches_the_restatement in tests/test_gpu_rankals.py."""
import numpy as np
import pytest

from tests import rankals_fixtures as fx
from tests.test_gpu_rankals import instance
from tests.util import same_bits_exact

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sw", [True, False], ids=["sw_on", "sw_off"])
@pytest.mark.parametrize("k", fx.BORDER_KS)
def test_staging_borders(k, sw):
    nu, ni, cells = fx.per_border_matrix(k)
    P0, Q0, want = fx.per_border_run(k, sw)
    h = instance(k, nu, ni, cells, P0, Q0)
    for n, (Pw, Qw) in enumerate(want):
        h.iterate(sw)
        P, Q = h.model()
        assert same_bits_exact(P, Pw), (n, np.argwhere(P != Pw)[:5])
        assert same_bits_exact(Q, Qw), (n, np.argwhere(Q != Qw)[:5])
    h.close()
