"""Every SGD kernel family trained with loud, pairwise-distinct regU / regI / regB / regC (tests/hparam_anchor.py) against the fp64
oracle given the same four values.  Everywhere else in the suite regU == regI == regB, so a swapped regulariser computes the same
bits, and all of them are so small that a dropped term stays under the fp32 state bars; here tests/test_hparam_separation.py has
shown on the CPU that every swap and every dropped term moves state and loss by 10 x the bars below or more.

Bars (hparam_anchor.BARS, all taken from the existing tests of the families): strict fp64 -- state bit-identical, loss bit-identical
under the serial schedule and 1e-12 otherwise; fp64 -- state 1e-11, loss 1e-10; fp32 -- state 3e-4, loss 3e-5.  Each case forces its
path the way that family's own tests do and asserts what schedule_info() reports about it.  The plumbing between a setting.conf and
the kernels (model file, shard group, the two hosts' parsers) carries the same values through at the end of the module."""
import re
import subprocess

import numpy as np
import pytest

from carskit_amd import capi
from tests import hparam_anchor as ha
from tests import util
from tests.test_gpu_parity import make_pair

pytestmark = pytest.mark.gpu


def _build(case):
    regs = ha.regs_for(case.model)
    if case.key == "sim":
        from tests import test_gpu_sim_models as sim
        d, empty = ha.data(case.key)
        return sim.make(case.model, d, empty, case.k, case.flags, regs=regs)[1]
    if case.key.startswith("svdpp-"):
        from tests import test_gpu_svdpp_team as team
        return team._pair(*ha.data(case.key), case.k, case.flags, regs=regs)[1]
    return make_pair(case.model, ha.data(case.key), case.k, case.flags, seed=ha.INIT_SEED, regs=regs)[1]


def _assert_path(case, inst):
    """What schedule_info() / schedule_traffic() can tell, which is what the families' own tests assert.  It does not name the kernel:
    fast against small against generic on the levels (chosen by k and the state type), the lanes per tuple of the small kernels (by k
    and the number of dimensions), the CAMF_C pipe against the one-ahead wave, the ext kernels and the SVD++ team kernel against its
    fallback (by the CMI_* variables and the LDS budget) are taken from those rules as read in the sources, not observed here."""
    info, want = inst.schedule_info(), case.expect
    if "kind" in want:
        assert info["kind"] == want["kind"], info
    if info["kind"] == "level":
        assert info["levels"] >= 1
    if want.get("tail"):         # as test_heavy_tailed_items_use_the_tail_launch: thousands of levels, walked by far fewer launches
        d = ha.data(case.key)
        u, j, _, _ = util.tuples_for(case.model, d)
        n_levels = len(capi.level_schedule(u, j, d.n_users, d.n_items)[1]) - 1
        assert n_levels > 1000 and info["levels"] < n_levels // 4, (n_levels, info["levels"])
    if "arena" in want:
        assert inst.schedule_traffic()["spoke_arena"] == want["arena"]
    if "teams" in want:
        assert (info["teams"] > 0) == want["teams"], info
    if "blocks" in want:
        assert (info["flow_blocks"] > 0) == want["blocks"], info
        if want["blocks"]:
            assert ha.data(case.key).n / info["flow_blocks"] >= 3


def _anchor(case, inst):
    losses, ref = ha.reference(case.model, case.key, case.k)
    state_bar, loss_bar = ha.BARS[case.prec]
    lr = ha.learn_rate(case.key)
    got = [inst.train_epoch(lr) for _ in range(ha.EPOCHS)]
    state = inst.get_states()
    loss_dev = max(abs(a - b) / abs(a) for a, b in zip(losses, got))
    state_dev = {n: float(np.max(np.abs(ref[n].reshape(a.shape) - a))) for n, a in state.items()}
    print("ANCHOR %s %s k=%d %s state %.3e loss %.3e" % (case.family, case.model, case.k, case.prec, max(state_dev.values()), loss_dev))
    assert np.isfinite(got).all()
    if loss_bar is None:
        assert list(losses) == got
    else:
        assert loss_dev <= loss_bar, (loss_dev, loss_bar)
    for name, a in state.items():
        if state_bar is None:
            assert np.array_equal(ref[name].reshape(a.shape), a), name
        else:
            assert state_dev[name] <= state_bar, (name, state_dev[name], state_bar)


@pytest.mark.parametrize("case", ha.CASES, ids=ha.case_id)
def test_kernel_family_holds_its_bar_at_loud_distinct_regularisers(case):
    def run():
        inst = _build(case)
        _assert_path(case, inst)
        _anchor(case, inst)
    util.with_env(run, **case.env)


def test_model_file_carries_each_regulariser_in_its_own_field(tmp_path):
    """One epoch, save; load into a handle that was given a permutation of the four values and another global mean; one more epoch on
    both handles is the oracle's second epoch, bit for bit."""
    case = ha.PLUMBING[0]
    d = ha.data(case.key)
    orc, a = make_pair(case.model, d, case.k, case.flags, seed=ha.INIT_SEED, regs=ha.LOUD_REGS)
    _assert_path(case, a)
    regU, regI, regB, regC = ha.LOUD_REGS
    _, b = make_pair(case.model, d, case.k, case.flags, seed=77, regs=(regC, regU, regI, regB))
    b.set_hparams(regC, regU, regI, regB, 1.0)
    lo, la = orc.epoch(util.LR), a.train_epoch(util.LR)
    assert abs(lo - la) <= 1e-12 * abs(lo)
    a.save_model(tmp_path / "m.cmi")
    b.load_model(tmp_path / "m.cmi")
    lo = orc.epoch(util.LR)
    for inst in (a, b):
        lg = inst.train_epoch(util.LR)
        assert abs(lo - lg) <= 1e-12 * abs(lo)
        for name, arr in inst.get_states().items():
            assert np.array_equal(orc.state[name].reshape(arr.shape), arr), name
    ref_losses, ref = ha.reference(case.model, case.key, case.k)          # (and that second epoch is the shared reference's)
    assert lo == ref_losses[1]


def test_group_set_hparams_gives_every_shard_the_four_values_in_order():
    from tests.test_gpu_group import check_fp64_shards_equal_merged_oracles
    check_fp64_shards_equal_merged_oracles(ha.LOUD_REGS)


STRICT_SERIAL = capi.FLAG_STATE_F64 | capi.FLAG_STRICT | capi.FLAG_SCHED_SERIAL


def test_setting_conf_to_kernel_through_the_python_host(tmp_path):
    """`reg.lambda=0.05 -u 0.03 -i 0.07 -b 0.15 -c 0.31` (CAMF_CU names all four; the main value is none of them) through the host
    mirror with the GPU engine, strict fp64, against the oracle behind the same host: as test_c2_frappe_strict_fp64_bit_exact."""
    from tests.hostmirror import main
    conf = ha.depaul_conf(tmp_path, ha.CONF_ALGO)
    _, gpu, _ = main.run(conf, log=lambda *a: None, conf_overrides={"flags": STRICT_SERIAL, "num_iters": ha.CONF_ITERS})
    _, cpu, _ = main.run(conf, engine_factory=util.OracleEngine, log=lambda *a: None, conf_overrides={"num_iters": ha.CONF_ITERS})
    assert len(gpu) == 5
    for a, b in zip(gpu, cpu):
        assert (a.conf.regU, a.conf.regI, a.conf.regB, a.conf.regC) == ha.LOUD_REGS
        assert a.losses == b.losses and a.lrates == b.lrates and np.isfinite(a.losses).all()
        for name, arr in a.state.items():
            assert np.array_equal(arr, b.state[name].reshape(arr.shape)), name
        assert abs(a.measures["RMSE"] - b.measures["RMSE"]) <= 1e-12 and abs(a.measures["MAE"] - b.measures["MAE"]) <= 1e-12


def test_setting_conf_to_kernel_through_the_cpp_host(tmp_path):
    """the same file through carskit-mi355x (its own Conf parser, cmi_set_hparams call): the oracle's numbers, as
    test_cpp_host_driver_c1_matches_oracle holds it"""
    from tests.test_host_layer import EXE, expected_from_oracle
    conf = ha.depaul_conf(tmp_path, ha.CONF_ALGO)
    p = subprocess.run([EXE, "-c", conf, "--iters", str(ha.CONF_ITERS), "--flags", str(STRICT_SERIAL), "--precise"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    m = re.search(r"PRECISE CAMF_CU folds=5 MAE=(\S+) RMSE=(\S+)", p.stdout)
    assert m, p.stdout[-500:]
    want = expected_from_oracle(conf, ha.CONF_ALGO, ha.CONF_ITERS)
    assert abs(float(m.group(1)) - want["MAE"]) <= 1e-12 and abs(float(m.group(2)) - want["RMSE"]) <= 1e-12
