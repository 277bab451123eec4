"""Host-only checks of the refined cut of the hub-chain level schedule (carskit_amd/csrc/chain_refine.hpp, applied by
level_schedule.cpp build_chain_schedule after the greedy walk).  The greedy walk places every tuple as early as possible and closes a
unit whenever the spoke row's previous tuple sits at the unit's level or later; the refinement moves tuples UP into the following unit
of their hub row where the spoke row's next tuple lies later still.  What must hold afterwards is exactly what held before -- the
invariants of tests/test_chain_schedule.py, reused here -- with fewer units, no more levels, and the same epoch bit for bit.
CMI_CHAIN_REFINE=0 gives the greedy cut."""
import os

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from carskit_amd import capi, synth

from tests.test_chain_schedule import _check_chain
from tests.util import LR, REG, REGC


def _greedy(fn):
    old = os.environ.get("CMI_CHAIN_REFINE")
    os.environ["CMI_CHAIN_REFINE"] = "0"
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["CMI_CHAIN_REFINE"]
        else:
            os.environ["CMI_CHAIN_REFINE"] = old


def _both(u, j, nu, ni, hub, max_chain):
    """(greedy, refined), each with every invariant checked; levels and units never grow, the hub side does not change."""
    g = _greedy(lambda: _check_chain(u, j, nu, ni, hub, max_chain))
    r = _check_chain(u, j, nu, ni, hub, max_chain)
    assert r[3] == g[3]
    assert len(r[2]) <= len(g[2])
    assert len(r[1]) <= len(g[1])
    return g, r


def _units(sched):
    """{first tuple: (level, tuples)} of a schedule"""
    perm, unit_off, level_off, _ = sched
    out = {}
    for l in range(len(level_off) - 1):
        for q in range(level_off[l], level_off[l + 1]):
            seg = perm[unit_off[q]:unit_off[q + 1]]
            out[int(seg[0])] = (l, seg.tolist())
    return out


@pytest.mark.parametrize("hub", [-1, 0, 1])
@pytest.mark.parametrize("max_chain", [1, 2, 16])
def test_refined_schedule_small(hub, max_chain):
    d = synth.generate(37, 13, 2, 3, 600, seed=5)
    g, r = _both(d.u, d.j, d.n_users, d.n_items, hub, max_chain)
    if max_chain == 1:  # nothing can merge, so nothing moves: the plain level schedule, as before
        for a, b in zip(g[:3], r[:3]):
            assert np.array_equal(a, b)
        _, off = capi.level_schedule(d.u, d.j, d.n_users, d.n_items, 0)
        assert np.array_equal(np.diff(r[2]), np.diff(off))


@settings(max_examples=60, deadline=None)
@given(nu=st.integers(1, 9), ni=st.integers(1, 9), n=st.integers(0, 90), seed=st.integers(0, 1000), hub=st.integers(-1, 1),
       max_chain=st.integers(1, 16))
def test_refined_schedule_property(nu, ni, n, seed, hub, max_chain):
    rng = np.random.default_rng(seed)
    u = rng.integers(0, nu, n).astype(np.int32)
    j = rng.integers(0, ni, n).astype(np.int32)
    g, r = _both(u, j, nu, ni, hub, max_chain)
    if max_chain == 1:
        assert np.array_equal(g[0], r[0]) and np.array_equal(g[2], r[2])


def test_refinement_cuts_a_fifth_of_the_units_on_c3_like_data():
    d = synth.generate_fast(20000, 2000, 4, 8, 1_000_000, seed=3)
    g = _greedy(lambda: capi.chain_schedule(d.u, d.j, d.n_users, d.n_items, -1, 16))
    r = capi.chain_schedule(d.u, d.j, d.n_users, d.n_items, -1, 16)
    ug, ur = len(g[1]) - 1, len(r[1]) - 1
    print("units greedy %d refined %d (%.1f %% fewer), levels %d -> %d" % (ug, ur, 100.0 * (ug - ur) / ug, len(g[2]) - 1, len(r[2]) - 1))
    assert r[3] == g[3] and r[3]
    assert len(r[2]) <= len(g[2])
    assert ur <= 0.8 * ug
    assert np.all(np.diff(r[2]) > 0)
    assert sorted(r[0].tolist()) == list(range(len(d.u)))
    # every unit: one hub row, distinct spokes, CRS order, longest first inside a level (vectorised: 1 M tuples)
    perm, unit_off, level_off, _ = r
    lens = np.diff(unit_off)
    assert lens.min() >= 1 and lens.max() <= 16
    unit_id = np.repeat(np.arange(len(lens)), lens)
    hj, su = d.j[perm], d.u[perm]
    inner = unit_id[1:] == unit_id[:-1]
    assert np.all(hj[1:][inner] == hj[:-1][inner]) and np.all(np.diff(perm)[inner] > 0)
    pair = np.unique(unit_id.astype(np.int64) * d.n_users + su)
    assert len(pair) == len(perm)
    level_of_unit = np.repeat(np.arange(len(level_off) - 1), np.diff(level_off))
    same_level = level_of_unit[1:] == level_of_unit[:-1]
    assert np.all(np.diff(lens)[same_level] <= 0)
    # per user and per item the (level, position) order is the CRS order
    lev_t, pos_t = np.empty(len(perm), np.int64), np.empty(len(perm), np.int64)
    lev_t[perm] = level_of_unit[unit_id]
    pos_t[perm] = np.arange(len(perm)) - unit_off[:-1][unit_id]
    key = lev_t * 16 + pos_t
    for row in (d.u, d.j):
        order = np.argsort(row, kind="stable")
        same = row[order][1:] == row[order][:-1]
        assert np.all(np.diff(key[order])[same] > 0)


def test_refined_order_replay_equals_sequential_epoch_bitwise():
    """Oracle replay, as tests/test_chain_schedule.py does it for the greedy cut: the oracle's single-tuple update applied in REFINED
    schedule order gives the sequential epoch's model bit for bit (fp64)."""
    from oracle import oracle_c
    d = synth.generate(60, 25, 2, 3, 1500, seed=11)
    k = 6
    gm = oracle_c.global_mean(d.r)
    for model in ("CAMF_CUCI", "CAMF_CI", "CAMF_CU"):
        state = synth.init_state(model, d, k, seed=3)
        mk = lambda u, j, c, r: oracle_c.Oracle(model, k, d.n_users, d.n_items, d.n_conds, u, j, c, r, d.ctx_ptr, d.ctx_conds,
                                                {n: a.copy() for n, a in state.items()}, gm, REG, REG, REG, REGC)
        seq = mk(d.u, d.j, d.ctx, d.r)
        seq.epoch(LR)
        for hub in (0, 1):
            perm, unit_off, _, _ = capi.chain_schedule(d.u, d.j, d.n_users, d.n_items, hub, 16)
            greedy = _greedy(lambda: capi.chain_schedule(d.u, d.j, d.n_users, d.n_items, hub, 16))
            assert len(unit_off) < len(greedy[1])             # the refinement did something here
            rep = mk(d.u[perm], d.j[perm], d.ctx[perm], d.r[perm])
            rep.epoch(LR)
            for name, a in seq.state.items():
                if a is not None:
                    assert np.array_equal(a, rep.state[name]), (model, hub, name)


# Crafted cases, written by hand from the rule; a third kind, a data set on which a level empties, does not exist (last test).
def _case(nu, ni, n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, nu, n).astype(np.int32), rng.integers(0, ni, n).astype(np.int32)


def test_a_merge_lands_exactly_on_sixteen_and_one_is_refused_at_seventeen():
    """Item 0 is rated by users 1..17 in turn, all of them for the last time.  User 9 rated item 1 before (level 1) and user 17 items 3
    and 2 (levels 1, 2), so greedy cuts item 0's chain into users 1-8 (level 1), 9-16 (level 2) and 17 (level 3).  Nothing follows any of
    them on their users' rows: walking back from user 17 the refinement takes 16 tuples into the level-3 unit and refuses the 17th (user
    1, the cap), which stays where it was; with room for 17 the whole chain is one unit."""
    u = np.array([9, 17, 17] + list(range(1, 18)), np.int32)
    j = np.array([1, 3, 2] + [0] * 17, np.int32)
    g, r = _both(u, j, 18, 4, 1, 16)
    row = lambda s: sorted((l, t) for l, t in _units(s).values() if j[t[0]] == 0)
    assert [(l, len(t)) for l, t in row(g)] == [(0, 8), (1, 8), (2, 1)]
    assert [(l, len(t)) for l, t in row(r)] == [(0, 1), (2, 16)]
    assert row(r)[0][1] == [3] and row(r)[1][1] == list(range(4, 20))
    _, r17 = _both(u, j, 18, 4, 1, 17)
    assert [(l, len(t)) for l, t in row(r17)] == [(2, 17)]


def test_a_hub_row_whose_whole_chain_becomes_one_unit():
    """Item 0: users 0, 1, 2, 3 with item 1 in between making user 2 late -- greedy cuts item 0's chain at user 2; nothing follows the
    first two tuples on their users' rows, so they rise and the row is one unit."""
    u = np.array([0, 1, 4, 2, 2, 3], np.int32)
    j = np.array([0, 0, 1, 1, 0, 0], np.int32)
    g, r = _both(u, j, 5, 2, 1, 16)
    row_g = [t for _, t in _units(g).values() if j[t[0]] == 0]
    row_r = [t for _, t in _units(r).values() if j[t[0]] == 0]
    assert len(row_g) == 2 and row_r == [[0, 1, 4, 5]]


def test_no_level_empties_under_this_rule():
    """A data set on which a level empties could NOT be found (seeded search, 300 random id sets at three densities), and with the rule
    as it stands there is none: a unit's level is the old level of its last member, and along a longest dependency path every level keeps
    one -- the tuple whose spoke successor opens a unit one level up cannot rise (its bound is its own level), and where a unit was
    opened one level up by the cap alone, the full unit before it cannot move into it whole.  So the refined schedule has exactly the
    greedy levels; the builders still drop an empty level should the rule ever leave one (level_off must stay strictly increasing)."""
    for seed in range(300):
        nu, ni, n = ((6, 4, 14), (9, 5, 40), (30, 6, 200))[seed % 3]
        u, j = _case(nu, ni, n, seed)
        for hub in (0, 1):
            g = _greedy(lambda: capi.chain_schedule(u, j, nu, ni, hub, 1 + seed % 16))
            r = capi.chain_schedule(u, j, nu, ni, hub, 1 + seed % 16)
            assert len(r[2]) == len(g[2]) and np.all(np.diff(r[2]) > 0), (seed, hub)
