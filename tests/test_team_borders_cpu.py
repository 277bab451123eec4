"""Without a GPU: the SVD++ team kernel's row budget (cmi_svdpp_team_rows) against the kernel's LDS layout restated here, and the
assertions of the data builders the border tests of svdpp_team and sgd_camfc_blocks rest on (tests/border_data.py)."""
import numpy as np
import pytest

from carskit_amd import capi
from tests import border_data as bd

BUDGET = 144 * 1024          # svdpp_team.hip: of the CU's 160 KB
CU_LDS = 160 * 1024
STATIC = 16 * 8              # svdpp_team's s_loss[16]


def layout_bytes(k, esize, rows):
    """svdpp_team's carve-up of its dynamic LDS: s_Y[rows][k] | s_p[k] | s_q[k] | s_part[66] | s_rr[rows] (T) | s_items[rows] |
    s_j[rows] (int32) -- the end of the last array"""
    s_y = 0
    s_p = s_y + rows * k * esize
    s_q = s_p + k * esize
    s_part = s_q + k * esize
    s_rr = s_part + 66 * esize
    s_items = s_rr + rows * esize
    assert s_items % 4 == 0 and s_rr % esize == 0
    s_j = s_items + rows * 4
    return s_j + rows * 4


@pytest.mark.parametrize("f64", [False, True])
def test_svdpp_team_rows_fit_the_launch_and_fill_the_budget(f64):
    esize = 8 if f64 else 4
    rows = [capi.svdpp_team_rows(k, f64) for k in range(1, 1025)]
    assert rows[0] == 4096 and rows[-1] >= 1
    assert all(a >= b for a, b in zip(rows, rows[1:]))                 # monotone in k
    assert any(a > b for a, b in zip(rows, rows[1:])) and min(rows) >= 1
    for k, r in zip(range(1, 1025), rows):
        lds = capi.svdpp_team_lds(k, f64)
        assert layout_bytes(k, esize, r) <= lds, (k, r, lds)           # the arrays end inside what the launch asks for
        assert lds + STATIC <= CU_LDS and lds <= BUDGET + 16, (k, lds)
        assert r == 4096 or layout_bytes(k, esize, r + 1) > BUDGET, (k, r)     # and no user that would fit is sent through memory
    assert capi.svdpp_team_rows(0, f64) == 0 and capi.svdpp_team_rows(1025, f64) == 0 and capi.svdpp_team_lds(1025, f64) == 0
    # what the issue of the border tests read off the code: at k = 1024, 33 fp32 rows or 15 fp64 rows
    assert rows[-1] == (15 if f64 else 33)


def test_fp64_rows_never_exceed_fp32_rows():
    assert all(capi.svdpp_team_rows(k, True) <= capi.svdpp_team_rows(k, False) for k in range(1, 1025))


# ---- the builders ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True])
def test_svdpp_row_ladder_has_exactly_its_counts(f64):
    R = capi.svdpp_team_rows(64, f64)
    u, j, r, nu, ni, counts = bd.svdpp_row_ladder(64, f64)
    got = np.bincount(u, minlength=nu).tolist()
    assert got == list(counts) and got[::2] == [1, 8, 9, 16, 63, 64, 65, 128, 129, R - 1, R, R + 1] and ni == R + 8 and nu == 24
    for x in range(nu):                                                 # row-major, items ascending and distinct: a train matrix
        assert np.all(np.diff(j[u == x]) > 0)
    assert np.all(np.diff(u) >= 0) and len(set(j.tolist())) == ni       # every user draws from the one pool, all of it rated


@pytest.mark.parametrize("k", [511, 512, 513, 1000, 1024])
@pytest.mark.parametrize("f64", [False, True])
def test_svdpp_factor_ladder_sits_on_the_budget(k, f64):
    R = capi.svdpp_team_rows(k, f64)
    u, j, r, nu, ni, counts = bd.svdpp_factor_ladder(k, f64)
    got = np.bincount(u, minlength=nu).tolist()
    assert got == list(counts) and {1, R - 1, R, R + 1} <= set(got) and max(got) == R + 1 and nu == 20
    assert any(c not in (1, R - 1, R, R + 1) and c < R - 1 for c in got)


@pytest.mark.parametrize("f64", [False, True])
def test_svdpp_row_cap_user_has_the_capped_count(f64):
    u, j, r, nu, ni, counts = bd.svdpp_row_cap(f64)
    assert max(counts) == capi.svdpp_team_rows(1, f64) == 4096 and np.bincount(u).tolist() == list(counts)
    assert counts[0] < 4096 > counts[-1]


@pytest.mark.parametrize("k", [17, 64])
def test_svdpp_streams(k):
    R = capi.svdpp_team_rows(k, True)
    for kind in bd.STREAMS:
        u, j, r, nu, ni, counts = bd.svdpp_stream(kind, k, True)
        seen = np.bincount(u, minlength=nu)
        assert seen[seen > 0].tolist() == list(counts)
    assert bd.svdpp_stream("single", k, True)[5] == (1,)
    assert bd.svdpp_stream("fallback_first", k, True)[5][0] == R + 1 and bd.svdpp_stream("fallback_last", k, True)[5][-1] == R + 1
    u = bd.svdpp_stream("gaps", k, True)[0]
    assert sorted(set(u.tolist())) == [2, 3, 7, 8, 15, 40]
    u, j, r, nu, ni = bd.svdpp_aba(k)
    run = np.flatnonzero(u == 5)
    assert j[run[0]] == j[run[2]] and j[run[1]] != j[run[0]] and len(set(j[run].tolist())) == len(run) - 1


def test_camfc_stream_has_the_chosen_blocks():
    u, j, want = bd.camfc_stream()
    assert 2500 <= len(u) <= 4500 and len(u) == sum(bd.STRETCHES)
    lens = np.diff(capi.conflict_free_blocks(u, j, bd.POOL, bd.POOL)).tolist()
    assert lens == list(want) and lens.count(64) >= 20 and lens.count(1) >= 5 and 63 in lens and lens[-1] == 5
    assert any(lens[i:i + 3] == [64, 64, 64] for i in range(len(lens)))


@pytest.mark.parametrize("n_dims,cpd,ragged", bd.CAMFC_CONTEXTS)
def test_camfc_contexts(n_dims, cpd, ragged):
    d = bd.camfc_data(n_dims, cpd, ragged)
    pb = bd.check_camfc_data(d, ragged)
    assert d.n_conds == n_dims * cpd and pb.dmax == n_dims
    if (n_dims, cpd) in ((4, 16), (8, 8), (16, 4)):
        assert d.n_conds == 64 and np.any(pb.conds == 63)                # condition id 63: lane 63 of the register chain
    if ragged:
        assert np.any(pb.conds == -1) and np.any(np.all(pb.conds == -1, axis=1))


def test_camfc_cases_cross_every_nv_with_every_chain_form():
    from tests import sgd_f32_ref as ref
    assert [bd.chain_form(nd, nd * c) for nd, c, _ in bd.CAMFC_CONTEXTS] == [1, 1, 2, 1, 2, 0, 0, 1, 2, 0]
    assert tuple(c[:3] for c in bd.CAMFC_CASES) == bd.CAMFC_CONTEXTS
    met = {(ref.camfc_layouts(k)["blocks"][1], bd.chain_form(nd, nd * c)) for nd, c, _, k in bd.CAMFC_CASES}
    assert met == {(nv, ch) for nv in (4, 8, 16) for ch in (0, 1, 2)}
    assert {k for _, _, _, k in bd.CAMFC_CASES} == {1, 17, 64, 65, 128, 129, 256}
