"""svdpp_team (carskit_amd/csrc/svdpp_team.hip) at the borders tests/test_gpu_svdpp_team.py never reaches.  That module's users have 1
to 30 rated items or several hundred: nobody has more than 64 rows on the team path (a 16-lane group never takes a second row), nobody
sits at the LDS budget or one past it, k stops at 300 (r_step = 1024 / k stays above 1, f_step never 0), and the cap of 4096 rows never
binds.  Here every border is taken from capi.svdpp_team_rows, the launcher's own arithmetic:

  the row ladder     k = 64: users with 1, 8, 9, 16, 63, 64, 65, 128, 129, R - 1, R and R + 1 items, an ordinary user between every
                     two, all drawing from one pool of R + 8 items (the Y rows one user writes back are gathered by the next; the
                     fallback user R + 1 sits between two team users)
  the factor ladder  k = 511, 512, 513, 1000, 1024: r_step = 2 with f_step = 2, r_step = 2 / f_step = 0, r_step = 1, and every thread
                     a factor thread with f_step = 0; the row counts again on the budget
  the row cap        k = 1: a user with 4096 items on the team path
  stream shapes      a single rating; a fallback user first; a fallback user last; user ids with gaps; a user whose run is A, B, A

against the sequential fp64 C restatement, in test_gpu_svdpp_team._check's shape: fp64 state every epoch's loss to 1e-11 relative and
every state array to 1e-10; fp32 state (the cases that run it) 3e-5 and 3e-4, the north_star tolerance.  A, B, A is not a train matrix
(the restatement counts |N(u)| differently there): the team kernel is held to the single-wave kernel it replaces, as
test_a_user_in_several_runs_and_a_repeated_pair does.  Every case prints its figures before it asserts."""
import os

import numpy as np
import pytest

from carskit_amd import capi
from tests import border_data as bd
from tests import util
from tests.test_gpu_svdpp_team import _pair

pytestmark = pytest.mark.gpu
F64 = capi.FLAG_STATE_F64
LR = util.LR / 4


def _check(orc, inst, flags, epochs=2):
    rel = []
    for _ in range(epochs):
        lo, lg = orc.epoch(LR), inst.train_epoch(LR)
        rel.append(abs(lo - lg) / abs(lo))
    dist = {name: float(np.max(np.abs(orc.state[name].reshape(a.shape) - a))) for name, a in inst.get_states().items()}
    print("loss relative", ["%.3g" % x for x in rel], "state", {n: "%.3g" % v for n, v in dist.items()})
    assert max(rel) <= (1e-11 if flags else 3e-5), rel
    for name, v in dist.items():
        assert v <= (1e-10 if flags else 3e-4), (name, v)


def _run(case, k, flags):
    u, j, r, nu, ni = case[:5]
    orc, inst = _pair(u, j, r, nu, ni, k, flags)
    _check(orc, inst, flags)


@pytest.mark.parametrize("flags", [F64, 0])
def test_row_count_ladder(flags):
    case = bd.svdpp_row_ladder(64, bool(flags))
    R = capi.svdpp_team_rows(64, bool(flags))
    assert np.bincount(case[0]).tolist()[::2] == [1, 8, 9, 16, 63, 64, 65, 128, 129, R - 1, R, R + 1]
    _run(case, 64, flags)


@pytest.mark.parametrize("k,flags", [(511, F64), (512, F64), (512, 0), (513, F64), (1000, F64), (1024, F64), (1024, 0)])
def test_factor_count_ladder(k, flags):
    case = bd.svdpp_factor_ladder(k, bool(flags))
    R = capi.svdpp_team_rows(k, bool(flags))
    assert {1, R - 1, R, R + 1} <= set(case[5])
    _run(case, k, flags)


@pytest.mark.parametrize("flags", [F64, 0])
def test_row_cap_at_one_factor(flags):
    case = bd.svdpp_row_cap(bool(flags))
    assert max(case[5]) == capi.svdpp_team_rows(1, bool(flags)) == 4096
    _run(case, 1, flags)


@pytest.mark.parametrize("k", [17, 64])
@pytest.mark.parametrize("kind", bd.STREAMS)
def test_stream_shapes(kind, k):
    _run(bd.svdpp_stream(kind, k, True), k, F64)


@pytest.mark.parametrize("k", [17, 64])
def test_a_pair_that_recurs_with_another_rating_between(k):
    """A, B, A in one user's run: the request for the second A's itemBias and Q row follows their store by one link"""
    u, j, r, nu, ni = bd.svdpp_aba(k)
    assert "CMI_NO_SVDPP_TEAM" not in os.environ
    for flags in (F64, 0):
        _, a = _pair(u, j, r, nu, ni, k, flags)
        la = [a.train_epoch(LR) for _ in range(3)]

        def single_wave():
            _, b = _pair(u, j, r, nu, ni, k, flags)
            return b, [b.train_epoch(LR) for _ in range(3)]

        b, lb = util.with_env(single_wave, CMI_NO_SVDPP_TEAM="1")
        dist = {name: float(np.max(np.abs(x - b.get_state(name)))) for name, x in a.get_states().items()}
        print("fp64" if flags else "fp32", "losses", la, lb, "state", dist)
        np.testing.assert_allclose(la, lb, rtol=1e-11 if flags else 3e-5)
        for name, v in dist.items():
            assert v <= (1e-10 if flags else 3e-4), (name, v)
