"""sgd_camfc_blocks (carskit_amd/csrc/mf_sgd_kernels.hip) at the borders the random data of the older tests never reaches: blocks of
exactly 64 tuples (every 16-lane group live, the whole of wave 0 holding a tuple), three of them in a row (the next block's ids are
requested while this block's rows are written), blocks of 1 and of 63 and a short last block; the register chain at 64 conditions
(condition id 63 in lane 63) and with more than four dimensions (the upper half of the packed ids, the DM = 8 arm); the lean LDS chain
chosen by the condition count (65, 344) and the round-2 chain chosen by the dimension count (9, 16); ragged contexts -- the last
dimension absent, and a context with no condition at all -- in each of the three forms.  Every form is the launcher's own choice: no
variable is set.  The stream is built by hand (tests/border_data.py), its block lengths asserted with the library's block builder.

fp32 state: bit for bit the restatement tests/sgd_f32_ref.epoch_camfc after each of three epochs, the loss to 1e-12 (the bar of
tests/test_gpu_sgd_f32_bitexact.py; the restatement is held to the oracle on these data in tests/test_sgd_f32_ref.py).
fp64 state: the sequential oracle, loss to 1e-10 relative and state to 1e-9, the bar of test_camf_c_conflict_free_blocks."""
import os

import numpy as np
import pytest

from carskit_amd import capi
from tests import border_data as bd
from tests import sgd_f32_ref as ref
from tests import util
from tests.test_gpu_parity import assert_state_equal, make_pair
from tests.test_gpu_sgd_f32_bitexact import hold

pytestmark = pytest.mark.gpu
F64, SERIAL = capi.FLAG_STATE_F64, capi.FLAG_SCHED_SERIAL


def _no_knobs():
    """the chain form and the kernel are the library's default choice"""
    knobs = [v for v in os.environ if v.startswith("CMI_CAMFC_") or v.startswith("CMI_NO_CAMFC_")]
    assert not knobs, knobs


def _blocks_chosen(inst, d):
    info = inst.schedule_info()
    lens = np.diff(capi.conflict_free_blocks(d.u, d.j, d.n_users, d.n_items))
    assert info["kind"] == "serial" and info["flow_blocks"] == len(lens) > 0 and d.n / len(lens) >= 5, info


@pytest.mark.parametrize("n_dims,cpd,ragged,k", bd.CAMFC_CASES)
def test_camf_c_blocks_borders_f32_bit_identical_to_the_restatement(n_dims, cpd, ragged, k):
    _no_knobs()
    d = bd.camfc_data(n_dims, cpd, ragged)
    pb = bd.check_camfc_data(d, ragged)
    assert pb.dmax == n_dims and d.n_conds == n_dims * cpd
    inst = hold("CAMF_C", d, k, SERIAL, ref.camfc_layouts(k)["blocks"], "serial")
    _blocks_chosen(inst, d)


@pytest.mark.parametrize("n_dims,cpd,ragged,k", bd.CAMFC_CASES)
def test_camf_c_blocks_borders_f64_match_the_sequential_oracle(n_dims, cpd, ragged, k):
    _no_knobs()
    d = bd.camfc_data(n_dims, cpd, ragged)
    orc, inst = make_pair("CAMF_C", d, k, SERIAL | F64)
    _blocks_chosen(inst, d)
    for epoch in range(3):
        lo, lg = orc.epoch(util.LR), inst.train_epoch(util.LR)
        print("epoch %d: loss %.17g, oracle %.17g, relative %.3g" % (epoch + 1, lg, lo, abs(lo - lg) / abs(lo)))
        assert abs(lo - lg) <= 1e-10 * abs(lo), (epoch, lo, lg)
    assert_state_equal(orc, inst, exact=False, atol=1e-9)
