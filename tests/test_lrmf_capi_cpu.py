"""LRMF without a GPU: the C ABI symbols (header, binding table, library), the refusals that answer before any device call, the LDS
bound, and the host-only unit schedule (cmi_lrmf_levels) against a brute-force schedule and tests/lrmf_ref.py."""
import os
import re

import numpy as np
import pytest

from carskit_amd import capi
from tests import lrmf_ref as lref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("cmi_lrmf_create", "cmi_lrmf_destroy", "cmi_lrmf_last_error", "cmi_lrmf_set_ratings", "cmi_lrmf_set_model",
           "cmi_lrmf_get_model", "cmi_lrmf_iterate", "cmi_lrmf_predict_batch", "cmi_lrmf_eval_rankings", "cmi_lrmf_last_iter_ms",
           "cmi_lrmf_last_schedule", "cmi_lrmf_levels", "cmi_lrmf_lds_rows", "cmi_lrmf_block")


def cols(cells):
    return ([c[0] for c in cells], [c[1] for c in cells], [c[2] for c in cells])


def test_lrmf_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "carskit_mi355x.h")).read()
    assert sorted(set(re.findall(r"\b(cmi_lrmf_\w+)\(", header))) == sorted(SYMBOLS)
    L = capi.lib()
    bound = {name for name, _, _ in capi.SYMBOLS}
    assert {n for n in bound if n.startswith("cmi_lrmf_")} == set(SYMBOLS)
    for s in SYMBOLS:
        assert getattr(L, s) is not None
    assert L.cmi_abi_version() == 5
    for m in ("set_ratings", "set_model", "model", "iterate", "predict", "eval_rankings", "last_iter_ms", "last_schedule", "close"):
        assert callable(getattr(capi.LRMFInstance, m))


def test_lds_bound_follows_from_the_kernels_lds_use():
    """160 KiB hold P[u] (128 doubles), two buffers of one pass's exps, the cell's scalars (8 doubles), and the rows at an odd stride"""
    B = capi.lrmf_block()
    assert B == 256
    fixed = 128 + 2 * B + 8
    for k in (1, 2, 3, 10, 16, 17, 64, 128):
        stride = k if k % 2 else k + 1
        rows = capi.lrmf_lds_rows(k)
        assert rows == (160 * 1024 // 8 - fixed) // stride, k
        assert (fixed + rows * stride) * 8 <= 160 * 1024 < (fixed + (rows + 1) * stride) * 8
    assert capi.lrmf_lds_rows(16) == capi.lrmf_lds_rows(17)          # both at 17 doubles a row
    assert capi.lrmf_lds_rows(0) == 0 and capi.lrmf_lds_rows(129) == 0


def test_argument_checks_answer_before_any_device_call():
    with pytest.raises(capi.CmiError) as e:
        capi.LRMFInstance(129, 10, 10)
    assert e.value.code == capi.E_UNSUPPORTED and "cmi_lrmf_create" in str(e.value) and "k <= 128" in str(e.value)
    for k, nu, ni, flags in ((0, 10, 10, 0), (4, 0, 10, 0), (4, 10, -1, 0), (4, 10, 10, 0x4)):
        with pytest.raises(capi.CmiError) as e:
            capi.LRMFInstance(k, nu, ni, flags=flags)
        assert e.value.code == capi.E_INVALID, (k, nu, ni, flags)
    L = capi.lib()
    assert L.cmi_lrmf_create(4, 10, 10, 0, 0, None) == capi.E_INVALID
    for call in (lambda: L.cmi_lrmf_iterate(None, 0.1, 0.1, 0.1, None), lambda: L.cmi_lrmf_set_ratings(None, 0, None, None, None),
                 lambda: L.cmi_lrmf_set_model(None, None, None), lambda: L.cmi_lrmf_get_model(None, None, None),
                 lambda: L.cmi_lrmf_predict_batch(None, 0, None, None, None), lambda: L.cmi_lrmf_last_iter_ms(None, None),
                 lambda: L.cmi_lrmf_last_schedule(None, None)):
        assert call() == capi.E_INVALID
    assert L.cmi_lrmf_destroy(None) == capi.OK


def test_lrmf_instance_without_device():
    if capi.device_count() > 0:
        pytest.skip("GPU present")
    with pytest.raises(capi.CmiError) as e:
        capi.LRMFInstance(10, 10, 10)
    assert e.value.code == capi.E_NO_DEVICE and "cmi_lrmf_create" in str(e.value) and "no CPU fallback" in str(e.value)


def brute_force_levels(n_users, cells):
    """level(u) = 1 + the largest level of an EARLIER user that shares a stored column with u (any earlier one, not only the last:
    the same number, since the last earlier user of a column lies above every one before it)"""
    stored = [set() for _ in range(n_users)]
    for u, j, _ in cells:
        stored[u].add(j)
    lv = [0] * n_users
    for u in range(n_users):
        if stored[u]:
            lv[u] = 1 + max([lv[v] for v in range(u) if stored[v] & stored[u]], default=0)
    return lv, stored


def check_schedule(n_users, n_items, cells):
    order, level_of, n_levels, max_chain = capi.lrmf_levels(n_users, n_items, *cols(cells)[:2])
    want, stored = brute_force_levels(n_users, cells)
    assert level_of.tolist() == want == lref.levels(n_users, n_items, cells)
    assert n_levels == max(want, default=0)
    units = [u for u in range(n_users) if stored[u]]
    assert sorted(order.tolist()) == units
    assert order.tolist() == sorted(units, key=lambda u: (want[u], u))   # by level, ascending inside a level
    for l in range(1, n_levels + 1):                                 # every level row-disjoint
        seen = set()
        for u in units:
            if want[u] == l:
                assert not (seen & stored[u]), (l, u)
                seen |= stored[u]
    for u in units:                                                  # every unit after its predecessors
        for v in range(u):
            if stored[v] & stored[u]:
                assert want[v] < want[u], (v, u)
    chain = max((sum(1 for u in units if j in stored[u]) for j in range(n_items)), default=0)
    assert max_chain == chain and n_levels >= max_chain
    return level_of.tolist(), n_levels, max_chain


@pytest.mark.parametrize("seed", range(8))
def test_levels_against_a_brute_force_schedule(seed):
    rng = np.random.default_rng(20270220 + seed)
    nu, ni = int(rng.integers(1, 61)), int(rng.integers(1, 41))
    cells = []
    for u in range(nu):
        cnt = int(rng.integers(0, min(ni, 9) + 1)) if seed % 2 else int(rng.integers(0, 3))
        for j in rng.choice(ni, size=cnt, replace=False):
            cells.append((u, int(j), float(rng.integers(0, 4))))     # a quarter of the cells are stored zeros
    perm = rng.permutation(len(cells))                               # the cells arrive in any order
    check_schedule(nu, ni, [cells[p] for p in perm])


def test_levels_edge_cases():
    assert check_schedule(3, 4, [])[1:] == (0, 0)                     # the empty matrix
    assert check_schedule(1, 5, [(0, 1, 2.0), (0, 4, 1.0)]) == ([1], 1, 1)          # a single user
    lv, nl, chain = check_schedule(9, 3, [(u, 1, 1.0 + u) for u in range(9)])       # all users on one item
    assert lv == list(range(1, 10)) and nl == chain == 9
    lv, nl, chain = check_schedule(6, 12, [(u, 2 * u + d, 1.0) for u in range(6) for d in (0, 1)])   # disjoint users
    assert lv == [1] * 6 and nl == chain == 1
    # a stored zero is a unit's only link to an earlier user: the row is written all the same
    lv, nl, _ = check_schedule(3, 4, [(0, 0, 3.0), (0, 1, 2.0), (1, 1, 0.0), (1, 2, 4.0), (2, 3, 1.0)])
    assert lv == [1, 2, 1] and nl == 2
    lv, _, _ = check_schedule(3, 4, [(0, 0, 3.0), (0, 1, 2.0), (1, 2, 4.0), (2, 3, 1.0)])               # without it: one level
    assert lv == [1, 1, 1]


def test_levels_refusals():
    for args in ((0, 3, [], []), (3, 0, [], []), (2, 3, [0, 2], [0, 1]), (2, 3, [0, 1], [0, 3]), (2, 3, [0, -1], [0, 1])):
        with pytest.raises(capi.CmiError) as e:
            capi.lrmf_levels(*args)
        assert e.value.code == capi.E_INVALID, args
    with pytest.raises(capi.CmiError) as e:
        capi.lrmf_levels(2, 3, [1, 0, 1], [2, 0, 2])
    assert e.value.code == capi.E_INVALID and "duplicate cell (user 1, item 2)" in str(e.value)
