"""Top-N evaluation of ItemKNN, UserKNN, SlopeOne and NMF without a GPU: the C ABI symbols are exported and bound, and a NULL handle is
CMI_E_INVALID."""
import ctypes as C
import os
import re

import pytest

from carskit_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("cmi_knn_ranking_batch", "cmi_knn_eval_rankings", "cmi_slope_eval_rankings", "cmi_topn_nmf_eval_rankings")
TIMERS = ("cmi_knn_last_rank_ms", "cmi_slope_last_rank_ms", "cmi_topn_nmf_last_rank_ms")


def test_symbols_exported_bound_and_declared():
    L = capi.lib()
    bound = {name for name, _, _ in capi.SYMBOLS}
    hdr = open(os.path.join(ROOT, "include", "carskit_mi355x.h")).read()
    for s in NEW_SYMBOLS + TIMERS:
        assert s in bound and getattr(L, s) is not None
        assert re.search(r"\bint %s\(" % s, hdr), s


def test_eval_rankings_signatures_follow_slim():
    """each takes its leading arguments and then the argument list of cmi_slim_eval_rankings"""
    sig = {name: args for name, _, args in capi.SYMBOLS}
    slim = sig["cmi_slim_eval_rankings"]
    assert sig["cmi_knn_eval_rankings"] == [slim[0], C.c_int, C.c_double] + slim[1:]
    assert sig["cmi_slope_eval_rankings"] == [slim[0], C.c_double] + slim[1:]
    assert sig["cmi_topn_nmf_eval_rankings"] == slim


@pytest.mark.parametrize("name", NEW_SYMBOLS + TIMERS)
def test_null_handle_is_invalid(name):
    args = next(a for n, _, a in capi.SYMBOLS if n == name)
    zero = [None if a in (C.c_void_p,) or hasattr(a, "contents") else 0 for a in args]
    assert getattr(capi.lib(), name)(*zero) == capi.E_INVALID


def test_python_methods_exist():
    for cls, names in ((capi.KNNInstance, ("ranking", "eval_rankings", "last_rank_ms")), (capi.SlopeOneInstance, ("eval_rankings", "last_rank_ms")),
                       (capi.NMFInstance, ("eval_rankings", "last_rank_ms"))):
        for n in names:
            assert callable(getattr(cls, n))
