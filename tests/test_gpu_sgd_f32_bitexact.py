"""The fp32 SGD kernels against tests/sgd_f32_ref.py, the fp32 restatement of the same update: model state BIT-IDENTICAL after each of
three epochs, each epoch's loss within 1e-12 relative of the restatement's math.fsum (same terms, another summation tree -- the bar of
test_level_strict_f64_state_bit_exact, for the same reason).

Why the bits can be asked for: csrc/Makefile builds with -ffp-contract=off, so every fp32 operation is rounded on its own; the level
schedule is order-exact, so the state after an epoch does not depend on which wave ran which tuple; and the only order inside a tuple --
the dot product's and the context sum's -- is a fixed function of the lane layout, which sgd_f32_ref restates per kernel family.  The
restatement itself is held to the fp64 oracle on the host (tests/test_sgd_f32_ref.py).  The aggregate fp32 bars of the older tests
(state 2e-4 .. 3e-4, about 10^4 ulps) stay; these cases see a parameter moved by one ulp.

Which kernel a case runs -- fast against small against generic, VPL x RAGGED, the lanes per tuple -- is taken from level_kernel,
with_fast_shape and small_lpt as READ in mf_sgd_kernels.hip (sgd_f32_ref.level_layout / small_lpt), not observed: schedule_info() names
the schedule, not the kernel.  Every path is forced with the flags and variables the older tests of that path use.

When a case fails it prints where: the epoch, and among the entries that differ the one whose last writer comes first in the stream
-- that tuple's level, its position in the level, both values and their distance in ulps."""
import functools

import numpy as np
import pytest

from carskit_amd import capi, synth
from oracle import oracle_c
from tests import hparam_anchor as ha
from tests import sgd_f32_ref as ref
from tests import util

pytestmark = pytest.mark.gpu

EPOCHS = 3
REGS = ha.LOUD_REGS
NOCHAIN, CHAIN, SERIAL, OWNER = capi.FLAG_NO_CHAIN, capi.FLAG_SCHED_CHAIN, capi.FLAG_SCHED_SERIAL, capi.FLAG_SCHED_OWNER
FAST_TPG = SMALL_TPG = 2          # mf_sgd_kernels.hip: tuples per lane group of a level launch
ALL = ref.MODELS
CTX3 = ("CAMF_CI", "CAMF_CU", "CAMF_CUCI")


def _models(i, n=2):
    """n models, rotating through the five so that every model meets every kernel family"""
    return [ALL[(i + s) % len(ALL)] for s in range(n)]


# ---- data --------------------------------------------------------------------------------------------------------------------------
SHAPES = ((600, 60, 6000), (900, 100, 7000), (1200, 150, 8000), (1500, 200, 9000), (2000, 300, 12000))


def _level_widths(model, d):
    u, j, _, _ = util.tuples_for(model, d)
    return np.diff(capi.level_schedule(u, j, d.n_users, d.n_items)[1])


@functools.lru_cache(maxsize=None)
def level_data(two_d, n_dims, per):
    """The smallest of SHAPES (users x items x tuples, three conditions per dimension) whose level schedule has a level with more tuples
    than one workgroup takes (`per`) and a level that ends in a partial group."""
    model = "PMF" if two_d else "CAMF_CI"
    for nu, ni, n in SHAPES:
        d = util.small_data(n_users=nu, n_items=ni, n_dims=n_dims, conds_per_dim=3, n=n, seed=61)
        w = _level_widths(model, d)
        if np.any(w > per) and np.any(w % per != 0):
            return d
    raise AssertionError("no shape of SHAPES fills a workgroup of %d tuples" % per)


def _per_workgroup(layout):
    if layout[0] == "fast":
        return 16 * FAST_TPG
    if layout[0] == "small":
        return (256 // layout[1]) * SMALL_TPG
    return 4                      # sgd_level_generic: a wave per tuple, four to the workgroup


@functools.lru_cache(maxsize=None)
def ragged_data():
    """the data of test_ragged_and_empty_contexts: contexts with 0 .. 4 conditions"""
    rng = np.random.default_rng(3)
    nu, ni, nc, n = 40, 15, 7, 700
    ctx_lists = [[], [0], [1, 4], [0, 2, 5], [3, 4, 5, 6], [6]]
    ctx_ptr = np.cumsum([0] + [len(c) for c in ctx_lists]).astype(np.int32)
    ctx_conds = np.array([c for cl in ctx_lists for c in cl], dtype=np.int32)
    return synth.RatingData(nu, ni, nc, 4, rng.integers(0, nu, n).astype(np.int32), rng.integers(0, ni, n).astype(np.int32),
                            rng.integers(0, len(ctx_lists), n).astype(np.int32), rng.integers(1, 6, n).astype(np.float64), ctx_ptr, ctx_conds)


@functools.lru_cache(maxsize=None)
def tail_data():
    """The zipf recipe of test_heavy_tailed_items_use_the_tail_launch at a sixth of its size: on a grid of 1000 requested tuples (users in
    proportion) the smallest for which that test's assertion -- more than 1000 levels, walked by fewer than a quarter as many launches --
    still holds for the contextual models (the 2-D matrix of BiasedMF / PMF has too few tuples per item at any such size)."""
    d = util.small_data(n_users=420, n_items=300, n_dims=3, conds_per_dim=3, n=5000, seed=31, item_zipf=1.3)
    return synth.split(d, 0.2)[0]


@functools.lru_cache(maxsize=None)
def serial_data():
    return ha.data("serial")      # test_serial_strict_f64_bit_exact's 60 x 25 x 900


# ---- one case ----------------------------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return all(np.array_equal(np.asarray(a[n], np.float32).view(np.int32), b[n].view(np.int32)) for n in b)


def hold(model, d, k, flags, layout, kind, env=None, loss_rtol=1e-12):
    """three epochs on the GPU and in the restatement from the same fp32 start; -> the instance (for further path assertions)"""
    pb = ref.problem(model, d)
    gm = oracle_c.global_mean(d.r)
    hp = ref.hparams(model, util.LR, REGS, gm)
    st = ref.start_state(model, d, k, seed=ha.INIT_SEED)
    if model == "CAMF_C":          # one chain in CRS order: the "levels" of a failure report are its conflict-free blocks
        sched = (np.arange(pb.n), ref.camfc_blocks(pb))
    else:
        sched = ref.schedule(pb)

    def run():      # the CMI_* variables are read when the schedule is chosen AND when an epoch is launched: set for the whole case
        inst = capi.Instance(model, k, d.n_users, d.n_items, d.n_conds, flags=flags)
        inst.set_hparams(*REGS, gm)
        if model in util.TWO_D:
            inst.set_ratings(pb.u, pb.j, None, util.tuples_for(model, d)[3])
        else:
            inst.set_ratings(d.u, d.j, d.ctx, d.r, d.ctx_ptr, d.ctx_conds)
        inst.set_states(st)
        info = inst.schedule_info()
        assert info["kind"] == kind and info["dmax"] == pb.dmax, info
        for epoch in range(EPOCHS):
            got_loss = inst.train_epoch(util.LR)
            got = inst.get_states(np.float32)
            want_loss = ref.epoch_camfc(st, pb, hp, layout, sched[1]) if model == "CAMF_C" else ref.epoch(st, pb, hp, layout, sched)[0]
            if not _same_bits(got, st):
                where = ref.first_difference(pb, sched, got, st)
                print(where)
                pytest.fail("%s k=%d %r: state differs after epoch %d; %s" % (model, k, layout, epoch + 1, where))
            assert abs(got_loss - want_loss) <= loss_rtol * abs(want_loss), (epoch, got_loss, want_loss)
        return inst

    return util.with_env(run, **(env or {}))


# ---- the level kernels -------------------------------------------------------------------------------------------------------------
FAST_KS = (64, 128, 256, 68, 100, 124, 132, 188, 192, 200, 252)       # every VPL x RAGGED instance, both ends of each ragged range
SMALL = ((1, 1), (3, 2), (10, 4), (16, 4), (17, 3), (20, 6), (32, 8), (33, 2), (50, 5), (63, 12), (10, 16))   # test_small_k_path_f32's
EVERY_MODEL_AT = (10, 64, 100)


def _level_cases():
    out = []
    for i, k in enumerate(FAST_KS):
        out += [(m, k, 4) for m in (ALL if k in EVERY_MODEL_AT else _models(i))]
    for i, (k, nd) in enumerate(SMALL):
        out += [(m, k, nd) for m in (ALL if (k, nd) == (10, 4) else _models(i + 1))]
    for i, k in enumerate((70, 130)):                                  # sgd_level_generic<float>
        out += [(m, k, 3) for m in _models(2 * i + 3)]
    return out


def test_the_fast_ks_reach_every_shape_of_with_fast_shape():
    assert {ref.level_layout(k, 4)[1:] for k in FAST_KS} == {(v, False) for v in (1, 2, 4)} | {(v, True) for v in (2, 3, 4)}
    assert {ref.level_layout(k, nd)[1] for k, nd in SMALL} == {4, 8, 16}
    assert [ref.small_lpt(k, nd) for k, nd in SMALL] == [4, 4, 4, 4, 8, 8, 8, 16, 16, 16, 16]


@pytest.mark.parametrize("model,k,n_dims", _level_cases())
def test_level_kernels_bit_identical_to_the_restatement(model, k, n_dims):
    two_d = model in util.TWO_D
    layout = ref.level_layout(k, 0 if two_d else n_dims)
    per = _per_workgroup(layout)
    d = level_data(two_d, n_dims, per)
    w = _level_widths(model, d)
    assert np.any(w > per) and np.any(w % per != 0), (w.max(), per)    # more than one workgroup; a partial group at a level's end
    if layout[0] == "small":                                           # the rule as read from small_lpt, not observed
        dmax = 0 if two_d else n_dims
        want = 4 if (k <= 16 and dmax <= 4) else (8 if (k <= 32 and dmax <= 8) else 16)
        assert layout[1] == want and want >= dmax and 4 * want >= k
    hold(model, d, k, NOCHAIN, layout, "level")


@pytest.mark.parametrize("model", CTX3)
@pytest.mark.parametrize("k", [64, 10])
def test_ragged_and_empty_condition_lists(model, k):
    """contexts with 0 .. 4 conditions: the padded condition lanes of the fast and the small kernel"""
    d = ragged_data()
    assert ref.problem(model, d).dmax == 4 and np.any(ref.problem(model, d).conds[:, 0] < 0)
    hold(model, d, k, NOCHAIN, ref.level_layout(k, 4), "level")


# ---- narrow runs, chains, the serial schedule ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,k", [("CAMF_CI", 10), ("CAMF_CU", 10), ("CAMF_CU", 128), ("CAMF_CUCI", 128), ("CAMF_CI", 100), ("CAMF_CUCI", 100)])
def test_narrow_run_launches_bit_identical_to_the_restatement(model, k):
    """sgd_tail_small_f32 (k = 10), sgd_tail_fast_f32 exact (128) and ragged (100)"""
    d = tail_data()
    n_levels = len(_level_widths(model, d))
    inst = hold(model, d, k, 0, ref.level_layout(k, 3), "level")
    launches = inst.schedule_info()["levels"]
    assert n_levels > 1000 and launches < n_levels // 4, (n_levels, launches)


@pytest.mark.parametrize("model,k,hub", [("CAMF_CI", 128, "item"), ("CAMF_CU", 100, "user"), ("BiasedMF", 10, "item"), ("CAMF_CUCI", 20, "user")])
def test_forced_chain_bit_identical_to_the_restatement(model, k, hub):
    """sgd_chain_level (k >= 64) and sgd_chain_small, forced as tests/test_gpu_chain.py forces them: their bitwise equality to the plain
    level kernels is anchored here, not only relative"""
    two_d = model in util.TWO_D
    n_dims = 6 if k == 20 else 4
    layout = ref.level_layout(k, 0 if two_d else n_dims)
    d = level_data(two_d, n_dims, _per_workgroup(layout))
    hold(model, d, k, CHAIN, layout, "chain-" + hub, env={"CMI_CHAIN_HUB": hub})


@pytest.mark.parametrize("model,k", [(m, k) for i, k in enumerate((10, 64, 128, 260)) for m in _models(i, 3)])
def test_serial_schedule_bit_identical_to_the_restatement(model, k):
    """FLAG_SCHED_SERIAL, fp32: sgd_serial_fast (k <= 256) and sgd_serial<float> (k = 260), one wave in CRS order; the restatement runs its
    levels, which give the CRS loop's bits (test_level_order_and_crs_order_give_the_same_bits)"""
    hold(model, serial_data(), k, SERIAL, ref.serial_layout(k), "serial")


# ---- second tier: the owner epoch ------------------------------------------------------------------------------------------------------
def _owner_cases():
    out = []
    for i, k in enumerate((10, 64, 128, 200, 256)):                    # test_owner_f32_vs_oracle_north_star_bar's k
        out += [(m, k, ("item", "user")[(i + s) % 2], None) for s, m in enumerate(_models(i))]
    for i, k in enumerate((64, 200)):                                  # test_owner_team_form's fp32 k
        out += [(m, k, ("user", "item")[(i + s) % 2], "all") for s, m in enumerate(_models(i + 2))]
    return out


@functools.lru_cache(maxsize=None)
def owner_data(k, team):
    if team:
        return synth.generate(600, 70, 3, 4, 15000, seed=370 + k, item_zipf=1.1)      # test_owner_team_form's
    return synth.generate(800, 90, 4, 4, 20000, seed=170 + k, item_zipf=0.8)          # test_owner_f32_vs_oracle_north_star_bar's


@pytest.mark.parametrize("model,k,hub,team", _owner_cases())
def test_owner_epoch_state_bit_identical_to_the_restatement(model, k, hub, team):
    """owner_update (owner_kernels.hip), the wave-per-owner step and the team form's compute wave: the fp32 update written with fused
    multiply-adds, restated as such (sgd_f32_ref's "owner" layout).  Its sums are a fixed function of the lane layout -- an owner walks its
    list in order, whoever else runs -- so the STATE is held bit for bit.  The loss is a per-lane fp32 sum of squares over at most 16 steps
    of an owner's list before it is widened: n = 16 max(VPL, 2 NCW) + 1 fp32 additions of non-negative terms, so it is held to
    gamma_n = n u / (1 - n u) of the restatement's exact sum of the same terms (4e-6 at VPL = 4; the old bar is 3e-5)."""
    d = owner_data(k, team)
    layout = ref.owner_layout(k)
    ncw = (d.n_conds + 63) // 64
    n = 16 * max(layout[1], 2 * ncw) + 1
    u = 2.0 ** -24
    inst = hold(model, d, k, OWNER, layout, "owner-" + hub, env={"CMI_OWNER_HUB": hub, "CMI_OWNER_WAVES": None, "CMI_OWNER_TEAM": team},
                loss_rtol=n * u / (1 - n * u))
    assert (inst.schedule_info()["teams"] > 0) == (team == "all")


# ---- second tier: CAMF_C ---------------------------------------------------------------------------------------------------------------
CAMFC_BLOCKS = {0: {"CMI_CAMFC_LDS_CHAIN": "1", "CMI_CAMFC_NO_RC": None}, 1: {"CMI_CAMFC_LDS_CHAIN": None, "CMI_CAMFC_NO_RC": None},
                2: {"CMI_CAMFC_LDS_CHAIN": None, "CMI_CAMFC_NO_RC": "1"}}     # launch_camfc_blocks' chain form, as read there


@pytest.mark.parametrize("k,ch", [(64, 1), (64, 0), (100, 2), (130, 1), (256, 2), (256, 0)])
def test_camf_c_blocks_bit_identical_to_the_restatement(k, ch):
    """sgd_camfc_blocks, NV = 4 / 8 / 16 and the three forms of its scalar chain (12 conditions: the register chain is the default), on the
    data of test_camf_c_conflict_free_blocks: the chain's values do not depend on its form, the dot is a fixed 16-lane tree"""
    d = ha.data("camfc-blocks")
    env = dict(CAMFC_BLOCKS[ch], CMI_NO_CAMFC_BLOCKS=None)
    inst = hold("CAMF_C", d, k, SERIAL, ref.camfc_layouts(k)["blocks"], "serial", env=env)
    assert inst.schedule_info()["flow_blocks"] > 0 and d.n_conds <= 64


@pytest.mark.parametrize("k", [10, 64, 200, 256])
def test_camf_c_pipe_bit_identical_to_the_restatement(k):
    """sgd_camfc_pipe (condBias in a register: 12 conditions), MAXC = 1 / 4, FULL and masked rows, on the data of tests/test_gpu_camfc_pipe.py's
    recipe in hparam_anchor"""
    d = ha.data("camfc-pipe")
    inst = hold("CAMF_C", d, k, SERIAL, ref.camfc_layouts(k)["pipe"], "serial", env={"CMI_NO_CAMFC_BLOCKS": "1", "CMI_NO_CAMFC_PIPE": None})
    assert inst.schedule_info()["flow_blocks"] == 0


@pytest.mark.parametrize("k", [10, 128])
def test_camf_c_serial_fast_bit_identical_to_the_restatement(k):
    """sgd_serial_fast with condBias in LDS: the one-ahead wave, both newer forms switched off"""
    inst = hold("CAMF_C", serial_data(), k, SERIAL, ref.camfc_layouts(k)["serial_fast"], "serial",
                env={"CMI_NO_CAMFC_BLOCKS": "1", "CMI_NO_CAMFC_PIPE": "1"})
    assert inst.schedule_info()["flow_blocks"] == 0
