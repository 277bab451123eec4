"""Hand-built data for the border tests of the two one-workgroup epoch kernels (tests/test_gpu_svdpp_team_borders.py,
tests/test_gpu_camfc_blocks_borders.py): every size a kernel decides on is chosen here, not left to a random draw, and every builder
asserts what it promises (tests/test_border_data.py runs the builders without a GPU).

SVD++: 2-D train matrices whose users rate exactly the listed numbers of items; the borders come from capi.svdpp_team_rows (the most
rows the team path keeps in LDS), none is written down here.

CAMF_C: a tuple stream of "diagonal" stretches (u0 + i, j0 + i), i < L, over a pool of users and items that wraps around.  A stretch has
no user and no item twice, and the next stretch starts with this stretch's last user, so the conflict-free CRS blocks are exactly the
stretches cut at 64: a stretch of L tuples gives L // 64 blocks of 64 and one of L % 64."""
import functools

import numpy as np

from carskit_amd import capi, synth

# ---- SVD++ -------------------------------------------------------------------------------------------------------------------------


def svdpp_from_counts(counts, n_items, seed, ids=None):
    """a 2-D train matrix in row-major order: user ids[x] (default x) rates counts[x] distinct items, ascending; ratings 1 .. 5.
    -> (u, j, r, n_users)"""
    rng = np.random.default_rng(seed)
    ids = list(range(len(counts))) if ids is None else list(ids)
    assert len(ids) == len(counts) and all(a < b for a, b in zip(ids, ids[1:])) and max(counts) <= n_items and min(counts) >= 1
    u, j = [], []
    for x, m in zip(ids, counts):
        u += [x] * m
        j += np.sort(rng.choice(n_items, size=m, replace=False)).tolist()
    r = rng.integers(1, 6, size=len(u)).astype(np.float64)
    u, j = np.array(u, np.int32), np.array(j, np.int32)
    n_users = ids[-1] + 1
    got = np.bincount(u, minlength=n_users)
    assert got[ids].tolist() == list(counts) and got.sum() == sum(counts)          # exactly these row counts, nobody else rates
    return u, j, r, n_users


def _ordinary(rng, rows, hi=25):
    """a row count well inside the team path: 5 .. 25 where that many rows fit, else 2 .. rows - 2"""
    top = min(hi, rows - 2)
    return int(rng.integers(min(5, max(top - 1, 1)), top + 1))


@functools.lru_cache(maxsize=None)
def svdpp_row_ladder(k, f64):
    """every row count at which the team path changes what it does, an ordinary user between every two: 8 / 9 rows (the column sum's
    batches of eight), 63 / 64 / 65 (one row per 16-lane group; a group takes a second row), 128 / 129 (a third), and the LDS border
    R - 1, R, R + 1 (R + 1: wave 0's walk through memory, between two team users).  -> (u, j, r, n_users, n_items, counts)"""
    R = capi.svdpp_team_rows(k, f64)
    special = [1, 8, 9, 16, 63, 64, 65, 128, 129, R - 1, R, R + 1]
    assert all(a < b for a, b in zip(special, special[1:])), (R, special)         # the budget lies above the fixed rungs
    rng = np.random.default_rng(1000 + k)
    counts = []
    for s in special:
        counts += [s, _ordinary(rng, R)]
    n_items = R + 8
    u, j, r, nu = svdpp_from_counts(counts, n_items, seed=2000 + k)
    assert counts[::2] == special and all(5 <= c <= 25 for c in counts[1::2]) and len(counts) == 24
    return u, j, r, nu, n_items, tuple(counts)


@functools.lru_cache(maxsize=None)
def svdpp_factor_ladder(k, f64):
    """about 20 users at a large k: 1 row, R - 1, R and R + 1 rows, ordinary users below them -- and a fallback user directly between
    two users at the budget.  -> (u, j, r, n_users, n_items, counts)"""
    R = capi.svdpp_team_rows(k, f64)
    assert R >= 6, (k, R)
    rng = np.random.default_rng(3000 + k)
    o = lambda: _ordinary(rng, R)
    counts = [o(), 1, o(), R - 1, o(), R, o(), R + 1, o(), o(), R, R + 1, R, o(), 1, R - 1, R + 1, o(), o(), R]
    n_items = R + 8
    u, j, r, nu = svdpp_from_counts(counts, n_items, seed=4000 + k)
    assert {1, R - 1, R, R + 1} <= set(counts) and len(counts) == 20
    return u, j, r, nu, n_items, tuple(counts)


@functools.lru_cache(maxsize=None)
def svdpp_row_cap(f64):
    """k = 1: the cap on the rows, not the bytes, decides -- one user with as many items as the team path takes, small users around"""
    R = capi.svdpp_team_rows(1, f64)
    counts = [3, 7, 1, R, 2, 9, 5]
    n_items = R + 8
    u, j, r, nu = svdpp_from_counts(counts, n_items, seed=77)
    return u, j, r, nu, n_items, tuple(counts)


STREAMS = ("single", "fallback_first", "fallback_last", "gaps")


@functools.lru_cache(maxsize=None)
def svdpp_stream(kind, k, f64):
    """-> (u, j, r, n_users, n_items, counts)"""
    R = capi.svdpp_team_rows(k, f64)
    rng = np.random.default_rng(5000 + k)
    o = lambda: _ordinary(rng, R)
    ids = None
    if kind == "single":
        return np.array([1], np.int32), np.array([2], np.int32), np.array([4.0]), 3, 5, (1,)
    if kind == "fallback_first":
        counts = [R + 1, o(), o(), o(), 1, o()]
    elif kind == "fallback_last":
        counts = [o(), 1, o(), o(), o(), R + 1]
    elif kind == "gaps":                       # users 0, 1, 4 .. 6, 9 .. 14, 16 .. 39 have no rating; user 40 is the last id
        ids = [2, 3, 7, 8, 15, 40]
        counts = [o(), R, o(), R + 1, 1, o()]
    else:
        raise ValueError(kind)
    n_items = R + 8
    u, j, r, nu = svdpp_from_counts(counts, n_items, seed=6000 + k, ids=ids)
    if kind == "gaps":
        assert nu == 41 and np.count_nonzero(np.bincount(u, minlength=nu) == 0) == 35
    if kind == "fallback_first":
        assert np.count_nonzero(u == u[0]) == R + 1
    if kind == "fallback_last":
        assert np.count_nonzero(u == u[-1]) == R + 1
    return u, j, r, nu, n_items, tuple(counts)


@functools.lru_cache(maxsize=None)
def svdpp_aba(k):
    """a user whose run is A, B, A, C, ...: the pair (user, A) a second time with another rating in between (not a train matrix)"""
    rng = np.random.default_rng(7000 + k)
    counts = [int(rng.integers(5, 20)) for _ in range(12)]
    n_items = 40
    u, j, r, nu = svdpp_from_counts(counts, n_items, seed=8000 + k)
    at = int(np.flatnonzero(u == 5)[0])
    assert u[at + 1] == 5 and u[at + 2] == 5
    u = np.insert(u, at + 2, 5)
    j = np.insert(j, at + 2, j[at])
    r = np.insert(r, at + 2, 1.0 if r[at] != 1.0 else 5.0)
    run = np.flatnonzero(u == 5)
    assert np.all(np.diff(run) == 1) and j[run[0]] == j[run[2]] != j[run[1]] and r[run[0]] != r[run[2]]
    return u, j, r, nu, n_items


# ---- CAMF_C ------------------------------------------------------------------------------------------------------------------------
POOL = 300
STRETCHES = (1, 2, 63, 64, 65, 200, 5, 40, 64, 64, 1, 128, 33, 192, 17, 64, 3, 100, 64, 63, 1, 1, 256, 9, 70, 129, 64, 2, 191, 50,
             64, 64, 64, 1, 31, 127, 66, 12, 193, 8, 64, 5)
# (n_dims, conds_per_dim, ragged): launch_camfc_blocks' chain form is RC (condBias in a register: <= 64 conditions, <= 8 dimensions),
# CH 2 (lean LDS chain: more conditions) or CH 0 (more than 8 dimensions)
CAMFC_CONTEXTS = ((1, 5, False), (4, 16, False), (5, 13, False), (8, 8, False), (8, 43, False), (9, 3, False), (16, 4, False),
                  (4, 16, True), (8, 43, True), (16, 4, True))


# (n_dims, conds_per_dim, ragged, k): k spread over the contexts so that NV = 4 (k <= 64), 8 (<= 128) and 16 each meet RC, CH 2 and CH 0
CAMFC_CASES = ((1, 5, False, 1), (4, 16, False, 128), (5, 13, False, 17), (8, 8, False, 256), (8, 43, False, 65), (9, 3, False, 64),
               (16, 4, False, 129), (4, 16, True, 64), (8, 43, True, 256), (16, 4, True, 128))


def chain_form(n_dims, n_conds):
    """launch_camfc_blocks' choice with no variable set, as read there"""
    return 0 if n_dims > 8 or n_dims < 1 else (1 if n_conds <= 64 else 2)


@functools.lru_cache(maxsize=None)
def camfc_stream():
    """(u, j, block lengths) of the stretches above"""
    rng = np.random.default_rng(91)
    u, j = [], []
    u0 = 0
    for L in STRETCHES:
        assert 1 <= L < POOL
        j0 = int(rng.integers(POOL))
        u += [(u0 + i) % POOL for i in range(L)]
        j += [(j0 + i) % POOL for i in range(L)]
        u0 = u[-1]                               # the next stretch starts with this user: the block ends here
    u, j = np.array(u, np.int32), np.array(j, np.int32)
    want = []
    for L in STRETCHES:
        want += [64] * (L // 64) + ([L % 64] if L % 64 else [])
    return u, j, tuple(want)


@functools.lru_cache(maxsize=None)
def camfc_data(n_dims, conds_per_dim, ragged):
    """the stream with one condition per dimension (condition id = dimension * conds_per_dim + choice), 400 context combinations that
    between them name the first and the last condition id; ragged: the last condition of every third combination dropped and one
    combination left with no condition at all (tests/test_gpu_camfc_pipe.py's builder)"""
    u, j, want = camfc_stream()
    n = len(u)
    rng = np.random.default_rng(100 * n_dims + conds_per_dim)
    n_conds = n_dims * conds_per_dim
    n_ctx = 400
    choice = rng.integers(0, conds_per_dim, (n_ctx, n_dims))
    choice[0, :] = 0
    choice[1, :] = conds_per_dim - 1             # ... the largest id of every dimension, n_conds - 1 among them
    conds = (np.arange(n_dims)[None, :] * conds_per_dim + choice).astype(np.int32)
    ptr, flat = [0], []
    for c in range(n_ctx):
        row = conds[c].tolist()
        if ragged and c % 3 == 0:
            row = row[:-1]
        if ragged and c == 7:
            row = []
        flat += row
        ptr.append(len(flat))
    ctx = rng.integers(0, n_ctx, n).astype(np.int32)
    ctx[:8] = np.arange(8)                       # combinations 0, 1 and 7 are used whatever the draw
    r = rng.integers(1, 6, n).astype(np.float64)
    d = synth.RatingData(POOL, POOL, n_conds, n_dims, u, j, ctx, r, np.asarray(ptr, np.int32), np.asarray(flat, np.int32))
    check_camfc_data(d, ragged)
    return d


def check_camfc_data(d, ragged):
    """what the block tests rely on, from the library's own block builder"""
    from tests import sgd_f32_ref as ref
    u, j, want = camfc_stream()
    off = capi.conflict_free_blocks(d.u, d.j, d.n_users, d.n_items)
    lens = np.diff(off)
    assert lens.tolist() == list(want)
    assert {1, 63, 64} <= set(lens.tolist())
    is64 = (lens == 64).astype(int)
    assert np.any(is64[:-2] + is64[1:-1] + is64[2:] == 3)                          # three 64-tuple blocks in a row
    assert lens[-1] < 64 and d.n / len(lens) >= 5                                   # a short last block; long enough to be chosen
    assert len(set(d.u.tolist())) == POOL and np.bincount(d.u).min() >= 2          # the pool wraps: every row comes back in a later block
    pb = ref.problem("CAMF_C", d)
    assert pb.dmax == d.n_dims and pb.conds.max() == d.n_conds - 1 and pb.conds[pb.conds >= 0].min() == 0
    if ragged:
        assert np.any(pb.conds == -1) and np.any(np.all(pb.conds == -1, axis=1)) and np.any(pb.conds[:, -1] >= 0)
        assert np.any((pb.conds[:, -1] == -1) & (pb.conds[:, 0] >= 0))
    else:
        assert np.all(pb.conds >= 0)
    return pb
