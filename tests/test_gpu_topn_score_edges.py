"""The top-N evaluation of the four factor models whose score is rowMult (RankALS, BPR, LRMF, RankSGD) at every factor count they accept.
All four fill the score slab of rank_run_device_slab with one kernel (rankals_launch_score), which keeps the user's row of P in an LDS
array of RANK_SCORE_MAX_K = 128 doubles; BPR, LRMF and RankSGD take k up to 128, RankALS up to 64.  Here an injected model (no
iteration) is evaluated at k on both sides of 64 and up to 128, at candidate counts on both sides of one 256-lane block of that kernel,
and at list lengths on both sides of the switch between the streaming selection (topn <= 64) and the pass-per-rank selection; predict
over every cell runs at the same k.  Everything is compared with tests/rankals_ref.scores, rowMult's chain, bit for bit: lists, score
bits and predictions exactly, the measures within the 1e-12 of check_rankings.

The premise, checked on the CPU before a case's first device call: for every k > 64 used and every cut c in {64, 80, 96} below k, the
scores of the model cut to its first c factors differ from the full scores in every entry of users 0-6 and give at least one query of
the case's split another list.  A kernel that dropped or zeroed any upper factors therefore cannot pass."""
import functools

import numpy as np
import pytest

from carskit_amd import capi
from tests import rankals_ref as rref
from tests.test_gpu_rankals import check_score_kernel_and_selection_edges, instance, score_model, score_split

pytestmark = pytest.mark.gpu

CUTS = (64, 80, 96)


def flagged(cls, flags):
    def factory(k, nu, ni, cells, P, Q):
        h = cls(k, nu, ni, flags=flags)
        h.set_ratings([c[0] for c in cells], [c[1] for c in cells], [c[2] for c in cells])
        h.set_model(P, Q)
        return h
    return factory


# (the default form of RankSGD refuses most matrices at set_ratings, see test_refusals of tests/test_gpu_ranksgd.py)
SGD_MODELS = {
    "bpr": flagged(capi.BPRInstance, capi.BPR_FLAG_STRICT),
    "lrmf": flagged(capi.LRMFInstance, capi.LRMF_FLAG_STRICT),
    "ranksgd": flagged(capi.RankSGDInstance, capi.RANKSGD_FLAG_STRICT | capi.RANKSGD_FLAG_NUM_RATES_SIZE),
}
SHAPES = [(255, 64), (256, 65), (257, 64), (513, 70)]      # one block less a lane, one block, one block and a lane, three blocks;
#                                                            lists of 64 (streaming), 65 and 70 (a pass per rank)


@functools.lru_cache(maxsize=None)
def premise(k, n_cand, num_recs):
    """the upper factors matter (host only): per cut below k, (entries of users 0-6 that differ, queries of users 0-6 whose list differs)"""
    nu, ni, _, P, Q, full = score_model(k)
    train, test, _ = score_split(n_cand)
    cand, queries = capi.rank_plan(nu, ni, train, test, -1e9, 0)
    want = rref.top_lists(cand, queries, full, -1e9, num_recs)
    out = {}
    for c in (c for c in CUTS if c < k):
        cut = rref.scores(P[:, :c], Q[:, :c])
        lists = rref.top_lists(cand, queries, cut, -1e9, num_recs)
        assert lists.keys() == want.keys()
        differ = int(np.count_nonzero(cut[:7].view(np.int64) != full[:7].view(np.int64)))
        moved = sum(1 for key in want if key[0] != 7 and [i for i, _ in lists[key]] != [i for i, _ in want[key]])
        print("k %d cut %d: %d of %d entries differ, %d lists differ" % (k, c, differ, 7 * ni, moved))
        assert differ == 7 * ni and moved >= 1, (k, c, differ, moved)
        out[c] = (differ, moved)
    assert len(out) == sum(1 for c in CUTS if c < k)
    return out


def run_case(factory, k, n_cand, num_recs):
    if k > 64:
        assert premise(k, n_cand, num_recs)
    check_score_kernel_and_selection_edges(factory, k, n_cand, num_recs)


@pytest.mark.parametrize("k", [1, 63, 64, 65, 100, 127, 128])
@pytest.mark.parametrize("model", sorted(SGD_MODELS))
def test_factor_counts_up_to_128(model, k):
    """k = 1; 63, 64, 65: around RankALS's own limit, which the score kernel's row once had; 100; 127, 128: the models' limit.  257
    candidates (a block and a lane), lists of 10"""
    run_case(SGD_MODELS[model], k, 257, 10)


@pytest.mark.parametrize("n_cand,num_recs", SHAPES)
@pytest.mark.parametrize("model", sorted(SGD_MODELS))
def test_block_border_and_selection_switch_at_128_factors(model, n_cand, num_recs):
    run_case(SGD_MODELS[model], 128, n_cand, num_recs)


@pytest.mark.parametrize("k", [1, 63, 64])
def test_rankals_factor_counts_up_to_64(k):
    run_case(instance, k, 257, 10)


@pytest.mark.parametrize("n_cand,num_recs", SHAPES[:3])
def test_rankals_block_border_and_selection_switch_at_64_factors(n_cand, num_recs):
    run_case(instance, 64, n_cand, num_recs)
