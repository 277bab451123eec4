"""The matrices and restated runs of tests/test_gpu_nmf_anchor.py.  They are built here, from seeded generators, so that
tests/test_nmf_ref.py can hold each of them to its conditions on the CPU (what edges it has, and that it can see the fault it is there
for) while the GPU tests compare the kernels with the very same arrays.  Every run is restated once per process and never changed.

    ladder_matrix(transposed)       the row kernel's look-ahead remainders and chunk borders, with negative values
    loss_matrix(n_cells)            65 loss blocks with a full last block, 65 with a last block of one cell, exactly 64
    contained_matrix()              the ladder plus two components of their own, which keep what is injected into them"""
import collections
import functools

import numpy as np

from tests import nmf_ref as nref

Matrix = collections.namedtuple("Matrix", "nu ni u i r rows cols")
Step = collections.namedtuple("Step", "W Ht cells chain tree")   # after one iteration: the model, loss_cells, the strict chain, the tree

LADDER = list(range(1, 18)) + [63, 64, 65, 127, 128, 129]   # entries of user 0, 1, ...: every remainder of the look-ahead loops of 4 and
LADDER_ITEMS = 140                                          # of 8 entries, and the borders of one and of two chunks of 64, each +- 1
ANCHOR_KS = (63, 127, 129, 192, 193)                        # the last lane masked, G = 3 partly masked and full, one factor in the top group
LOSS_SHAPE, LOSS_K = (260, 64), 3
LOSS_CELLS = (16640, 16385, 16384)                          # 65 blocks of 256, the last full; 65, the last of one cell; exactly 64


def _matrix(nu, ni, cells):
    keys = sorted(cells)
    u, i = np.array([c[0] for c in keys], np.int32), np.array([c[1] for c in keys], np.int32)
    r = np.array([cells[c] for c in keys])
    return Matrix(nu, ni, u, i, r, nref.rows_of(u, i, r, nu), nref.cols_of(u, i, r, ni))


def _ladder_cells():
    """user a has exactly LADDER[a] entries among LADDER_ITEMS items; values m / 3, about one in seven negative"""
    rng = np.random.default_rng(20261201)
    cells = {}
    for a, cnt in enumerate(LADDER):
        for j in rng.choice(LADDER_ITEMS, cnt, replace=False).tolist():
            v = float(rng.integers(3, 16)) / 3.0
            cells[(a, j)] = -v if rng.integers(0, 7) == 0 else v
    return cells


@functools.lru_cache(maxsize=None)
def ladder_matrix(transposed=False):
    """23 users x 140 items with the ladder of lengths on the users (the W phase), or its transpose with the ladder on the items (the H
    phase)"""
    cells = _ladder_cells()
    if transposed:
        return _matrix(LADDER_ITEMS, len(LADDER), {(j, a): v for (a, j), v in cells.items()})
    return _matrix(len(LADDER), LADDER_ITEMS, cells)


def _run(m, W0, H0, iters=2):
    W, Ht, steps = W0.copy(), np.ascontiguousarray(H0.T), []
    with np.errstate(all="ignore"):
        for _ in range(iters):
            chain = nref.iterate(W, Ht, m.rows, m.cols)
            cells = nref.loss_cells(W, Ht, m.rows)
            steps.append(Step(W.copy(), Ht.copy(), cells, chain, nref.loss_tree(cells)))
    return steps


@functools.lru_cache(maxsize=None)
def ladder_run(k, transposed=False):
    """(W0, H0, the restatement's two iterations) on the ladder matrix from a seeded start"""
    m = ladder_matrix(transposed)
    rng = np.random.default_rng(1000 + k)
    W0, H0 = rng.random((m.nu, k)), rng.random((k, m.ni))
    return W0, H0, _run(m, W0, H0)


@functools.lru_cache(maxsize=None)
def loss_matrix(n_cells):
    """the first n_cells cells (in CRS order) of a dense 260 x 64 matrix, values m / 3, every seventh negative"""
    nu, ni = LOSS_SHAPE
    rng = np.random.default_rng(20261202)
    v = rng.integers(3, 16, nu * ni).astype(np.float64) / 3.0
    v[6::7] = -v[6::7]
    return _matrix(nu, ni, {(q // ni, q % ni): float(v[q]) for q in range(n_cells)})


@functools.lru_cache(maxsize=None)
def loss_run(n_cells):
    m = loss_matrix(n_cells)
    rng = np.random.default_rng(2000)                        # one start for the three: they differ in their last cells alone
    W0, H0 = rng.random((m.nu, LOSS_K)), rng.random((LOSS_K, m.ni))
    return W0, H0, _run(m, W0, H0)


# ---- contained non-finite and degenerate factors ---------------------------------------------------------------------------------------
CONTAINED_K = 5
N_LADDER = len(LADDER)
INF_USER, NAN_ITEM = N_LADDER, LADDER_ITEMS + 1              # in component A: users 23, 24 on items 140, 141, 142
OVERFLOW_USER, ZERO_ITEM = N_LADDER + 2, LADDER_ITEMS + 4    # in component B: users 25, 26 on items 143, 144, 145


@functools.lru_cache(maxsize=None)
def contained_matrix():
    """the ladder matrix and two components of two users on three items each, every cell of a component stored and positive: no entry
    joins a component to the ladder or to the other component, so no value injected into one can reach a row outside it"""
    rng = np.random.default_rng(20261203)
    cells = _ladder_cells()
    for c in range(2):
        for a in range(2):
            for j in range(3):
                cells[(N_LADDER + 2 * c + a, LADDER_ITEMS + 3 * c + j)] = float(rng.integers(3, 16)) / 3.0
    return _matrix(N_LADDER + 4, LADDER_ITEMS + 6, cells)


@functools.lru_cache(maxsize=None)
def contained_run():
    """(W0, H0, two iterations).  Component A takes an Inf in a user's row and a NaN in an item's row.  Component B takes an item's row of
    zeros and a user's finite row so large that e_t = product(W, u, H, j) overflows: estm is Inf, real / estm is 0 and the new row 0."""
    m = contained_matrix()
    rng = np.random.default_rng(3000)
    W0, H0 = rng.random((m.nu, CONTAINED_K)), rng.random((CONTAINED_K, m.ni))
    W0[INF_USER, 2] = np.inf
    H0[1, NAN_ITEM] = np.nan
    H0[:, ZERO_ITEM] = 0.0
    W0[OVERFLOW_USER] = 1.5e308 * (0.5 + 0.5 * W0[OVERFLOW_USER])
    return W0, H0, _run(m, W0, H0)
