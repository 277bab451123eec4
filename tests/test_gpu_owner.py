"""The owner (dataflow) epoch (carskit_amd/csrc/owner_kernels.hip, CMI_FLAG_SCHED_OWNER) on the GPU.

One persistent launch; rows of the heavy side owned by wavefronts, the other side's rows handed between owners as tagged records.
Bars: fp64 state -- the order-exact epoch, so state within 1e-11 of the oracle and loss to 1e-10 relative (a stale or torn record
would be off by ~lrate * error, eight orders above); fp32 state -- the north_star bar (loss 3e-5 relative, state 3e-4).
Every case runs with few owners (long lists, many rows per owner) and with as many owners as the chip holds (most lists short, the
hand-offs cross XCDs), on uniform and on heavy-tailed items, for both hub sides.
"""
import os

import numpy as np
import pytest

from carskit_amd import capi, synth
from tests import util
from tests.test_gpu_parity import assert_state_equal, make_pair

pytestmark = pytest.mark.gpu

OWNER, F64 = capi.FLAG_SCHED_OWNER, capi.FLAG_STATE_F64
LEVEL_MODELS = [m for m in util.MODELS if m != "CAMF_C"]

_env = util.with_env


def _run(model, data, k, flags, hub, waves, epochs=3, loss_tol=1e-10, exact=False, atol=1e-11, team=None):
    orc, inst = _env(lambda: make_pair(model, data, k, flags | OWNER), CMI_OWNER_HUB=hub, CMI_OWNER_WAVES=waves, CMI_OWNER_TEAM=team)
    info = inst.schedule_info()
    assert info["kind"] == "owner-" + hub
    for _ in range(epochs):
        lo, lg = orc.epoch(util.LR), inst.train_epoch(util.LR)
        assert abs(lo - lg) <= loss_tol * abs(lo), (lo, lg)
    assert_state_equal(orc, inst, exact=exact, atol=atol)
    return inst


@pytest.mark.parametrize("model", LEVEL_MODELS)
@pytest.mark.parametrize("hub", ["item", "user"])
@pytest.mark.parametrize("k", [10, 64, 100, 128])
def test_owner_f64_vs_oracle(model, hub, k):
    data = synth.generate(500, 60, 3, 4, 12000, seed=70 + k, item_zipf=1.1)
    for waves in (5, None):
        _run(model, data, k, F64, hub, waves)


@pytest.mark.parametrize("model", LEVEL_MODELS)
@pytest.mark.parametrize("hub", ["item", "user"])
@pytest.mark.parametrize("k", [3, 10, 64, 70, 128])
def test_owner_strict_f64_state_bit_identical_to_oracle(model, hub, k):
    """CMI_FLAG_STRICT with the owner epoch: the reference's operation order inside every update (left-to-right dot product, deviations
    added condition by condition) -- the model state after three epochs over heavy-tailed items is BIT-IDENTICAL to the sequential
    oracle's, whatever the number of owners; the loss (same terms, per-owner partial sums) to 1e-12."""
    data = synth.generate(500, 60, 3, 4, 12000, seed=270 + k, item_zipf=1.3)
    for waves in (3, None):
        _run(model, data, k, F64 | capi.FLAG_STRICT, hub, waves, loss_tol=1e-12, exact=True)


@pytest.mark.parametrize("model", LEVEL_MODELS)
@pytest.mark.parametrize("hub", ["item", "user"])
@pytest.mark.parametrize("k", [10, 64, 128, 200, 256])
def test_owner_f32_vs_oracle_north_star_bar(model, hub, k):
    data = synth.generate(800, 90, 4, 4, 20000, seed=170 + k, item_zipf=0.8)
    for waves in (16, None):
        _run(model, data, k, 0, hub, waves, loss_tol=3e-5, atol=3e-4)


@pytest.mark.parametrize("model", LEVEL_MODELS)
@pytest.mark.parametrize("hub", ["item", "user"])
@pytest.mark.parametrize("k,flags", [(10, F64), (64, F64), (128, F64), (64, 0), (200, 0)])
def test_owner_team_form(model, hub, k, flags):
    """The team form (a workgroup of three wavefronts per owner: loader -> LDS ring -> compute -> LDS ring -> storer), which
    cmi_set_ratings gives to the hottest single-row owners, forced on EVERY owner here (CMI_OWNER_TEAM=all), lists with many rows
    included: same bars as the one-wavefront form."""
    data = synth.generate(600, 70, 3, 4, 15000, seed=370 + k, item_zipf=1.1)
    for waves in (8, None):
        if flags:
            _run(model, data, k, flags, hub, waves, team="all")
        else:
            _run(model, data, k, flags, hub, waves, loss_tol=3e-5, atol=3e-4, team="all")


def test_owner_team_form_is_picked_for_the_hottest_rows():
    """Every instantiation gets automatic teams again (round 5 withheld them from fp64 at k <= 64, the instantiation measured inexact
    beside another owner epoch; the cause -- a store-data hazard in the record stores -- is fixed, tests/test_gpu_soak.py)."""
    data = synth.generate(20000, 2000, 4, 8, 600000, seed=91, item_zipf=1.1)
    for k in (128, 64):
        for team, expect in ((None, True), ("0", False)):
            orc, inst = _env(lambda: make_pair("CAMF_CI", data, k, F64 | OWNER), CMI_OWNER_TEAM=team, CMI_OWNER_TEAM_MIN=4096)
            info = inst.schedule_info()
            assert info["kind"] == "owner-item" and (info["teams"] > 0) == expect, info
            for _ in range(2):
                lo, lg = orc.epoch(util.LR), inst.train_epoch(util.LR)
                assert abs(lo - lg) <= 1e-10 * abs(lo)
            assert_state_equal(orc, inst, exact=False, atol=1e-11)
    # an instance that shares its device (cmi_set_device_share) keeps its teams too
    orc, inst = _env(lambda: make_pair("CAMF_CI", data, 64, F64 | OWNER, before_ratings=lambda i: i.set_device_share(2)), CMI_OWNER_TEAM=None,
                     CMI_OWNER_TEAM_MIN=4096)
    assert inst.schedule_info()["teams"] > 0


@pytest.mark.parametrize("model", LEVEL_MODELS)
@pytest.mark.parametrize("team", ["0", "all"])
def test_owner_f32_twenty_epochs_bold_driver_north_star_bar(model, team):
    """The north_star bar for the fp32 owner epoch on heavy-tailed items: 20 epochs under the bold driver take the same learning-rate
    decisions as the fp64 oracle, the loss trajectory agrees to 3e-5 and RMSE / MAE on held-out ratings to 1e-5."""
    data = synth.generate(3000, 400, 4, 4, 60000, seed=24, item_zipf=1.1)
    train, test = synth.split(data, 0.2)
    orc, inst = _env(lambda: make_pair(model, train, 128, OWNER), CMI_OWNER_TEAM=team)
    assert inst.schedule_info()["kind"].startswith("owner")
    o_losses, o_lrs, _ = orc.build_model(20, util.LR, bold_driver=True)
    g_losses, g_lrs = inst.train(20, util.LR, bold_driver=True)
    assert g_lrs.tolist() == o_lrs.tolist()
    np.testing.assert_allclose(g_losses, o_losses, rtol=3e-5)
    tctx = None if model in util.TWO_D else test.ctx
    oe = orc.eval_ratings(test.u, test.j, tctx, test.r, 1.0, 5.0)
    ge = inst.eval_ratings(test.u, test.j, tctx, test.r, 1.0, 5.0)
    assert abs(oe["RMSE"] - ge["RMSE"]) <= 1e-5 and abs(oe["MAE"] - ge["MAE"]) <= 1e-5


@pytest.mark.parametrize("zipf", [None, 1.5])
def test_owner_uniform_and_very_hot_items(zipf):
    data = synth.generate(3000, 200, 4, 4, 80000, seed=81, item_zipf=zipf)
    for model in ("CAMF_CI", "CAMF_CUCI", "BiasedMF"):
        _run(model, data, 64, F64, "item", None, epochs=2)


def test_owner_repeated_pairs_in_many_contexts():
    """DePaulMovie-like: the same (user, item) pair in several contexts = consecutive list entries sharing BOTH rows (the spoke row
    is taken over in registers, its record still goes out with every tag)."""
    data = synth.generate(40, 30, 2, 3, 6000, seed=43)
    for model in ("CAMF_CI", "CAMF_CU", "CAMF_CUCI"):
        for hub in ("item", "user"):
            _run(model, data, 64, F64, hub, 7)
            _run(model, data, 64, F64, hub, None)


def test_owner_64_conditions_and_the_unsupported_shapes():
    data = synth.generate(300, 50, 4, 16, 9000, seed=44)          # 64 conditions: lane c carries condition c, none to spare
    assert data.n_conds == 64
    _run("CAMF_CUCI", data, 32, F64, "item", None)
    _run("CAMF_CUCI", data, 32, F64, "user", 9)
    huge = synth.generate(300, 50, 5, 80, 9000, seed=45)          # 400 conditions: more than 6 words of 64
    with pytest.raises(capi.CmiError):
        make_pair("CAMF_CI", huge, 32, OWNER)
    _run("BiasedMF", huge, 32, F64, "item", None)                 # ... which a model without context does not care about
    with pytest.raises(capi.CmiError):
        make_pair("CAMF_CI", data, 300, OWNER)
    with pytest.raises(capi.CmiError):
        make_pair("CAMF_CI", data, 200, OWNER | F64)              # fp64 records: k <= 128
    with pytest.raises(capi.CmiError):
        make_pair("CAMF_C", data, 32, OWNER | capi.FLAG_SCHED_SERIAL)


@pytest.mark.parametrize("model", ["CAMF_CI", "CAMF_CU", "CAMF_CUCI"])
@pytest.mark.parametrize("dims,cpd", [(4, 25), (7, 49)])
def test_owner_more_than_64_conditions(model, dims, cpd):
    """100 conditions (two 64-condition words per context-bias row and per tuple mask; BASELINE C5 has 128) and 343 (six words;
    Frappe's count): lane l carries conditions l, l + 64, ...  fp64 vs the oracle for both hub sides, few / all owners, the team form
    forced on every owner, strict fp64 bit-identical, and fp32 at the north_star bar."""
    data = synth.generate(500, 60, dims, cpd, 12000, seed=500 + dims, item_zipf=1.1)
    assert data.n_conds == dims * cpd
    for hub in ("item", "user"):
        _run(model, data, 64, F64, hub, 6)
        _run(model, data, 100, F64, hub, None, team="all")
        _run(model, data, 10, F64 | capi.FLAG_STRICT, hub, None, loss_tol=1e-12, exact=True)
        _run(model, data, 128, 0, hub, None, loss_tol=3e-5, atol=3e-4)
        _run(model, data, 200, 0, hub, 11, loss_tol=3e-5, atol=3e-4, team="all")


def test_owner_many_epochs_under_uneven_load_stays_exact():
    """Heavy-tailed items at a size where the hottest owner walks tens of thousands of tuples while most owners wait on it:
    the hand-offs happen under load, consumer caches warm.  Ten epochs, checked against the serial fp64 walk on the GPU."""
    data = synth.generate(20000, 2000, 4, 8, 600000, seed=91, item_zipf=1.1)
    _, own = _env(lambda: make_pair("CAMF_CI", data, 128, F64 | OWNER), CMI_OWNER_HUB=None, CMI_OWNER_WAVES=None)
    _, ser = make_pair("CAMF_CI", data, 128, F64 | capi.FLAG_SCHED_SERIAL)
    assert own.schedule_info()["kind"] == "owner-item"
    for _ in range(10):
        lo, ls = own.train_epoch(util.LR), ser.train_epoch(util.LR)
        assert abs(lo - ls) <= 1e-10 * abs(ls)
    so, ss = own.get_states(), ser.get_states()
    for name in ss:
        assert np.max(np.abs(so[name] - ss[name])) <= 1e-11, name


def test_owner_epoch_leaves_the_tables_usable_by_the_other_paths():
    """The untag pass writes the records back: evaluation (plain table reads) after an owner epoch sees the trained model."""
    data = util.small_data(n_users=600, n_items=80, n_dims=3, conds_per_dim=4, n=15000, seed=33)
    train, test = synth.split(data, 0.2)
    orc, inst = make_pair("CAMF_CI", train, 64, F64 | OWNER)
    for _ in range(3):
        orc.epoch(util.LR)
        inst.train_epoch(util.LR)
    oe = orc.eval_ratings(test.u, test.j, test.ctx, test.r, 1.0, 5.0)
    ge = inst.eval_ratings(test.u, test.j, test.ctx, test.r, 1.0, 5.0)
    assert abs(oe["RMSE"] - ge["RMSE"]) <= 1e-9 and abs(oe["MAE"] - ge["MAE"]) <= 1e-9


def test_owner_is_picked_for_large_heavy_tailed_data_and_not_for_uniform():
    """>= 2^16 tuples whose levels are narrow: the owner epoch is the default; CMI_FLAG_NO_OWNER keeps the plain levels (same model to
    fp32 rounding: the owner kernel's fp32 update is the fused two-operation form).  Uniform data of the same size stays on the hub-chain
    levels."""
    data = synth.generate(50_000, 5_000, 4, 8, 2_000_000, seed=17, item_zipf=1.0)
    state = synth.init_state("CAMF_CI", data, 64, dtype=np.float32)
    insts = []
    for flags in (0, capi.FLAG_NO_OWNER):
        inst = capi.Instance("CAMF_CI", 64, data.n_users, data.n_items, data.n_conds, flags=flags)
        inst.set_hparams(util.REG, util.REG, util.REG, util.REGC, 3.0)
        inst.set_ratings(data.u, data.j, data.ctx, data.r, data.ctx_ptr, data.ctx_conds)
        inst.set_states(state)
        insts.append(inst)
    assert insts[0].schedule_info()["kind"] == "owner-item"
    assert insts[1].schedule_info()["kind"] == "level"
    for _ in range(2):
        lo, lp = insts[0].train_epoch(util.LR), insts[1].train_epoch(util.LR)
        assert abs(lo - lp) <= 2e-5 * abs(lp)
    so, sp = insts[0].get_states(), insts[1].get_states()
    for name in sp:
        # two different fp32 roundings of a ~400 000-step recurrence along the hottest item's row (values ~1): 2.5e-4 apart
        assert np.max(np.abs(so[name] - sp[name])) <= 1e-3, name
    wide = synth.generate_fast(100_000, 10_000, 4, 8, 2_000_000, seed=3)
    inst = capi.Instance("CAMF_CI", 64, wide.n_users, wide.n_items, wide.n_conds)
    inst.set_hparams(util.REG, util.REG, util.REG, util.REGC, 3.0)
    inst.set_ratings(wide.u, wide.j, wide.ctx, wide.r, wide.ctx_ptr, wide.ctx_conds)
    assert inst.schedule_info()["kind"].startswith("chain-")


def test_owner_epochs_of_concurrent_folds_do_not_starve_each_other():
    """`cv -p on`: several folds train from their own threads on one GPU.  An owner epoch needs every one of its workgroups resident,
    so two of them in flight at once could wait for each other forever; the library runs them one at a time.  Three instances, three
    threads, three epochs each: all finish and each matches its own oracle."""
    from concurrent.futures import ThreadPoolExecutor
    pairs = []
    for seed in (1, 2, 3):
        data = synth.generate(3000, 300, 3, 4, 120000, seed=400 + seed, item_zipf=1.2)
        pairs.append(make_pair("CAMF_CI", data, 64, F64 | OWNER))

    def work(pair):
        orc, inst = pair
        return [inst.train_epoch(util.LR) for _ in range(3)]

    with ThreadPoolExecutor(max_workers=3) as pool:
        losses = list(pool.map(work, pairs))
    for (orc, inst), ls in zip(pairs, losses):
        for lg in ls:
            lo = orc.epoch(util.LR)
            assert abs(lo - lg) <= 1e-10 * abs(lo)
        assert_state_equal(orc, inst, exact=False, atol=1e-11)


def test_schedule_note_when_owner_limits_force_the_level_walk():
    """outside the owner epoch's limits (here: more than 384 conditions) heavy-tailed data silently got the 10x slower level
    walk; cmi_schedule_note now says so (and is empty when nothing is lost)."""
    data = synth.generate(3000, 400, 4, 100, 70_000, seed=21, item_zipf=1.1)      # 400 conditions > 384
    st = synth.init_state("CAMF_CI", data, 64, seed=3, dtype=np.float32)
    inst = capi.Instance("CAMF_CI", 64, data.n_users, data.n_items, data.n_conds)
    inst.set_hparams(util.REG, util.REG, util.REG, util.REGC, 3.0)
    inst.set_ratings(data.u, data.j, data.ctx, data.r, data.ctx_ptr, data.ctx_conds)
    inst.set_states(st)
    assert inst.schedule_info()["kind"] == "level" and "level walk" in inst.schedule_note()
    l0 = inst.train_epoch(util.LR)
    assert np.isfinite(l0)
    small = util.small_data(n_users=50, n_items=20, n=800, seed=2)                # tiny uniform data: nothing to report
    i2 = capi.Instance("CAMF_CI", 8, small.n_users, small.n_items, small.n_conds)
    i2.set_ratings(small.u, small.j, small.ctx, small.r, small.ctx_ptr, small.ctx_conds)
    assert i2.schedule_note() == ""


def test_device_share_runs_owner_epochs_side_by_side_and_changes_nothing():
    """cmi_set_device_share (`cv -p on`: F folds on one GPU): an instance that declares F sharers sizes its persistent owner launch to
    1 / F of the device, and the library lets such epochs run concurrently (their workgroups fit the device together) instead of one at
    a time.  The schedule stays order-exact, so the model is bit for bit what the instance without the hint computes; three sharing
    instances trained from three threads each match their own oracle."""
    from concurrent.futures import ThreadPoolExecutor
    data = synth.generate(3000, 300, 3, 4, 120000, seed=77, item_zipf=1.2)
    st = synth.init_state("CAMF_CI", data, 64, seed=5, dtype=np.float32)

    def make(share):
        inst = capi.Instance("CAMF_CI", 64, data.n_users, data.n_items, data.n_conds, flags=OWNER)
        inst.set_hparams(util.REG, util.REG, util.REG, util.REGC, 3.0)
        if share:
            inst.set_device_share(share)
        inst.set_ratings(data.u, data.j, data.ctx, data.r, data.ctx_ptr, data.ctx_conds)
        inst.set_states(st)
        return inst

    whole, part = make(0), make(5)
    assert part.schedule_info()["kind"] == whole.schedule_info()["kind"] == "owner-item"
    assert 0 < part.schedule_info()["flow_blocks"] <= whole.schedule_info()["flow_blocks"] // 4
    for _ in range(3):
        lw, lp = whole.train_epoch(util.LR), part.train_epoch(util.LR)
        assert abs(lw - lp) <= 1e-9 * abs(lw)   # (the epoch loss is a sum of per-owner partial sums: other owners, another association)
    for name in ("P", "Q", "userBias", "icBias"):
        np.testing.assert_array_equal(whole.get_state(name), part.get_state(name))
    with pytest.raises(capi.CmiError):
        whole.set_device_share(0)

    pairs = []
    for seed in (1, 2, 3):
        d = synth.generate(3000, 300, 3, 4, 120000, seed=500 + seed, item_zipf=1.2)
        orc, inst = make_pair("CAMF_CI", d, 64, F64 | OWNER, before_ratings=lambda i: i.set_device_share(3))
        pairs.append((orc, inst))
    with ThreadPoolExecutor(max_workers=3) as pool:
        losses = list(pool.map(lambda p: [p[1].train_epoch(util.LR) for _ in range(3)], pairs))
    for (orc, inst), ls in zip(pairs, losses):
        for lg in ls:
            lo = orc.epoch(util.LR)
            assert abs(lo - lg) <= 1e-10 * abs(lo)
        assert_state_equal(orc, inst, exact=False, atol=1e-11)


def test_owner_epochs_of_two_processes_on_one_gpu_take_turns_and_stay_exact():
    """Two PROCESSES (two folds started as two programs) train owner-schedule instances on the same GPU.  Their persistent launches must
    not be in flight together (each could hold part of the compute units and wait for the rest): the per-device file lock makes them take
    turns, a process holding it while any of its owner epochs runs.  Both finish, both match their own oracle."""
    import subprocess
    import sys
    import textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r)
        import numpy as np
        from carskit_amd import capi, synth
        from tests import util
        from tests.test_gpu_parity import make_pair
        seed = int(sys.argv[1])
        d = synth.generate(3000, 300, 3, 4, 120000, seed=seed, item_zipf=1.2)
        orc, inst = make_pair("CAMF_CI", d, 64, capi.FLAG_STATE_F64 | capi.FLAG_SCHED_OWNER)
        assert inst.schedule_info()["kind"] == "owner-item"
        worst = 0.0
        for _ in range(6):
            lo, lg = orc.epoch(util.LR), inst.train_epoch(util.LR)
            worst = max(worst, abs(lo - lg) / abs(lo))
        err = max(float(np.max(np.abs(orc.state[n].reshape(a.shape) - a))) for n, a in inst.get_states().items())
        print("RESULT %%.3e %%.3e" %% (worst, err))
    """ % root)
    procs = [subprocess.Popen([sys.executable, "-c", prog, str(700 + i)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=root)
             for i in range(2)]
    for p in procs:
        out, errs = p.communicate(timeout=600)
        assert p.returncode == 0, errs[-2000:]
        line = [ln for ln in out.splitlines() if ln.startswith("RESULT")][-1].split()
        assert float(line[1]) <= 1e-10 and float(line[2]) <= 1e-11, line


def test_owner_epoch_is_refused_when_the_lock_file_cannot_be_opened():
    """The cross-process owner-epoch lock: a lock file that cannot be opened used to mean "launch unprotected"; since
    round 6 the epoch is refused with CMI_E_BUSY (model untouched) unless CMI_OWNER_NO_LOCK=1 declares the process the GPU's only user.
    Run in child processes: the gate caches the lock file's descriptor per process."""
    import subprocess
    import sys
    import textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    prog = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r)
        import numpy as np
        from carskit_amd import capi, synth
        from tests import util
        d = synth.generate(1500, 200, 3, 4, 30000, seed=7, item_zipf=1.2)
        st = synth.init_state("CAMF_CI", d, 16, seed=5, dtype=np.float32)
        inst = capi.Instance("CAMF_CI", 16, d.n_users, d.n_items, d.n_conds, flags=capi.FLAG_SCHED_OWNER)
        inst.set_hparams(util.REG, util.REG, util.REG, util.REGC, 3.0)
        inst.set_ratings(d.u, d.j, d.ctx, d.r, d.ctx_ptr, d.ctx_conds)
        inst.set_states(st)
        try:
            loss = inst.train_epoch(util.LR)
            print("RESULT ok", np.isfinite(loss))
        except capi.CmiError as e:
            same = all(np.array_equal(a, st[n].reshape(a.shape)) for n, a in inst.get_states(np.float32).items())
            print("RESULT error", e.code, "untouched" if same else "CHANGED", "|", e)
    """ % root)
    def run(**env):
        p = subprocess.run([sys.executable, "-c", prog], capture_output=True, text=True, cwd=root, timeout=600,
                           env=dict(os.environ, CMI_OWNER_LOCK_DIR="/proc/definitely/not/a/directory", **env))
        assert p.returncode == 0, p.stderr[-2000:]
        return [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][-1]
    refused = run()
    assert refused.startswith("RESULT error %d untouched" % capi.E_BUSY) and "cannot be opened" in refused, refused
    assert run(CMI_OWNER_NO_LOCK="1") == "RESULT ok True"
