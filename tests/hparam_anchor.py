"""Loud, pairwise-distinct regularisers for the SGD kernels, the mutants that tell them apart, and the recipes shared by
tests/test_hparam_separation.py (CPU: the fp64 oracle separates every mutant from LOUD_REGS by 10 x the GPU bars) and
tests/test_gpu_hparam_anchor.py (GPU: every kernel family trained with LOUD_REGS against the same oracle runs).

The suite's default regularisers have regU == regI == regB and are so small that dropping one moves the model by less than the fp32
state bars: a swapped or missing term is invisible there.  Here each of the four has its own value, a factor of two or more from
the next, and large enough that three epochs separate every swap and every missing term far above the fp32 bars."""
import collections
import functools
import itertools

import numpy as np

from carskit_amd import capi, synth
from oracle import oracle_c
from tests import util

NAMES = ("regU", "regI", "regB", "regC")
LOUD_REGS = tuple(synth.java_float(x) for x in (0.03, 0.07, 0.15, 0.31))
# CAMF_ICS / LCS / MCS start from small user factors (P scaled by 0.3 / 0.02) at an eighth of the rate: regU and regC have to be louder
# still before three epochs move the state by 10 x the fp32 bar
SIM_REGS = tuple(synth.java_float(x) for x in (3.0, 0.07, 0.3, 1.4))
EPOCHS = 3


def regs_for(model):
    return SIM_REGS if model in ("CAMF_ICS", "CAMF_LCS", "CAMF_MCS") else LOUD_REGS


# which parameters each recommender's buildModel names (update and loss), read off the reference's sources:
#   BiasedMF.java:76-97 regB (bu, bj), regU, regI          PMF.java:67-70 regU, regI only
#   CAMF_C.java:95-127 regB (bu, bj, and the condBias LOSS term), regC (condBias update), regU, regI
#   CAMF_CI.java:95-120 regB (bu), regC (icBias)            CAMF_CU.java:92-117 regB (bj), regC (ucBias)
#   CAMF_CUCI.java:105-123 regC (ucBias, icBias), no scalar bias and no regB
#   SVDPlusPlus.java:77-114 regB (bu, bj), regU (P and Y), regI; no regC
#   CAMF_ICS.java:89-120, CAMF_LCS.java:113-136, CAMF_MCS.java:101-155: regC (similarity parameters), regU, regI; no regB
USES = {"BiasedMF": "UIB", "PMF": "UI", "CAMF_C": "UIBC", "CAMF_CI": "UIBC", "CAMF_CU": "UIBC", "CAMF_CUCI": "UIC",
        "SVD++": "UIB", "CAMF_ICS": "UIC", "CAMF_LCS": "UIC", "CAMF_MCS": "UIC"}

MUTANTS = [("swap", a, b) for a, b in itertools.combinations(range(4), 2)] + [("zero", a) for a in range(4)]


def mutant_id(m):
    return "%s-%s" % (m[0], "-".join(NAMES[i] for i in m[1:]))


def mutate(regs, m):
    regs = list(regs)
    if m[0] == "swap":
        regs[m[1]], regs[m[2]] = regs[m[2]], regs[m[1]]
    else:
        regs[m[1]] = 0.0
    return tuple(regs)


def applicable(model, m):
    """a swap is felt if the model names either of the two, a zero if it names that one"""
    return any("UIBC"[i] in USES[model] for i in m[1:])


# the bars of the GPU module, none of them new: (state atol, loss rtol); None = bit-identical.  (The fp32 pair is the aggregate bar against
# the fp64 oracle; tests/test_gpu_sgd_f32_bitexact.py holds the same fp32 kernels bit for bit to tests/sgd_f32_ref.py, their fp32 restatement.)
BARS = {"f32": (3e-4, 3e-5),              # test_owner_f32_vs_oracle_north_star_bar, test_chain_small_k_lane_layouts_bitwise_equal_plain
        "f64": (1e-11, 1e-10),            # test_owner_f64_vs_oracle
        "strict": (None, 1e-12),          # test_level_strict_f64_state_bit_exact, test_owner_strict_f64_state_bit_identical_to_oracle
        "strict-serial": (None, None)}    # test_serial_strict_f64_bit_exact
SEPARATION = 10.0                         # every applicable mutant moves state and loss by this many times the loosest bar


def _train_part(data):
    return synth.split(data, 0.2)[0]


DATA = {
    # plain level schedule, 3000 x 300: wide enough that the fp32 level kernels run many tuples per level
    "level-d4": lambda: util.small_data(n_users=3000, n_items=300, n_dims=4, conds_per_dim=3, n=30000, seed=27),
    "level-d5": lambda: util.small_data(n_users=3000, n_items=300, n_dims=5, conds_per_dim=3, n=30000, seed=27),
    "level-d6": lambda: util.small_data(n_users=3000, n_items=300, n_dims=6, conds_per_dim=3, n=30000, seed=27),
    "generic": lambda: util.small_data(n_users=300, n_items=40, n=4000, seed=22),                 # test_level_strict_f64_state_bit_exact
    "tail": lambda: _train_part(util.small_data(n_users=2500, n_items=300, n_dims=3, conds_per_dim=3, n=30000, seed=31,
                                                item_zipf=1.3)),                                  # test_heavy_tailed_items_use_the_tail_launch
    "chain": lambda: _train_part(util.small_data(n_users=1200, n_items=260, n_dims=3, conds_per_dim=4, n=24000, seed=41)),  # the spoke-arena test's
    "owner": lambda: synth.generate(500, 60, 3, 4, 12000, seed=271, item_zipf=1.3),               # the strict owner test's
    "serial": lambda: util.small_data(n_users=60, n_items=25, n=900, seed=21),                    # test_serial_strict_f64_bit_exact
    "camfc-blocks": lambda: _train_part(util.small_data(n_users=900, n_items=700, n_dims=4, conds_per_dim=3, n=9000, seed=33)),
    "camfc-pipe": lambda: util.small_data(n_users=300, n_items=120, n_dims=3, conds_per_dim=4, n=5064, seed=104),
    "sim": util.sim_data,               # (data, EmptyContextConditions) of tests/test_gpu_sim_models.py
    # (u, j, r, n_users, n_items) of tests/test_gpu_svdpp_team.py: every user's Y rows fit the LDS budget (svdpp_link_team) ...
    "svdpp-team": lambda: util.svdpp_matrix(120, 90, 25, seed=64) + (120, 90),
    # ... and test_users_beyond_the_lds_budget_are_walked_through_hbm's with lighter heavy users: at k = 256 the 144 KB budget holds
    # about 140 fp32 rows (70 in fp64), so users 3 and 40 are walked by svdpp_link_wave, which has its own update body.  (That test's
    # 400 / 200 / 150 rows cost the premise's eleven oracle runs four times as much: SVD++ is quadratic in a user's row count.)
    "svdpp-heavy": lambda: util.svdpp_matrix(60, 250, 30, seed=5, heavy={3: 180, 40: 150}) + (60, 250),
    "group": lambda: _train_part(util.small_data(n_users=300, n_items=90, n_dims=3, conds_per_dim=3, n=6000, seed=13)),   # test_gpu_group._problem
}


@functools.lru_cache(maxsize=None)
def data(key):
    return DATA[key]()


def learn_rate(key):
    """util.LR, except where the existing tests of that recipe train at a smaller rate because the reference's default diverges"""
    return {"sim": util.LR / 8, "svdpp-team": util.LR / 4, "svdpp-heavy": util.LR / 4}.get(key, util.LR)


INIT_SEED = 5      # make_pair's


def new_oracle(model, key, k, regs=None):
    """the fp64 oracle over recipe `key`, on the initial model the GPU side of that recipe injects"""
    regs = regs or regs_for(model)
    if key == "sim":
        d, empty = data(key)
        return util.sim_oracle(model, d, empty, k, regs=regs)
    if key.startswith("svdpp-"):
        return util.svdpp_oracle(*data(key), k, regs=regs)
    d = data(key)
    return util.c_oracle(model, d, k, synth.init_state(model, d, k, seed=INIT_SEED), oracle_c.global_mean(d.r), *regs)


def run_oracle(model, key, k, regs=None):
    """-> (the EPOCHS epoch losses, the final state arrays)"""
    orc = new_oracle(model, key, k, regs)
    lr = learn_rate(key)
    losses = [orc.epoch(lr) for _ in range(EPOCHS)]
    return losses, {n: a for n, a in orc.state.items() if a is not None}


@functools.lru_cache(maxsize=None)
def reference(model, key, k):
    """run_oracle with regs_for(model), computed once per (model, recipe, k) and shared read-only by every case that uses it"""
    losses, state = run_oracle(model, key, k)
    for a in state.values():
        a.setflags(write=False)
    return tuple(losses), state


# ---- the GPU module's cases ------------------------------------------------------------------------------------------------------
# env: the CMI_* variables the existing tests of that family set while the instance is built (None = unset)
# expect: what schedule_info() / schedule_traffic() must report, as the existing tests of that family assert it
Case = collections.namedtuple("Case", "family model key k flags prec env expect")

F64, STRICT, SERIAL, NOGRAPH = capi.FLAG_STATE_F64, capi.FLAG_STRICT, capi.FLAG_SCHED_SERIAL, capi.FLAG_NO_GRAPH
NOCHAIN, CHAIN, OWNER = capi.FLAG_NO_CHAIN, capi.FLAG_SCHED_CHAIN, capi.FLAG_SCHED_OWNER
ARENA, NOARENA = capi.FLAG_SPOKE_ARENA, capi.FLAG_NO_ARENA
LEVEL_MODELS = [m for m in util.MODELS if m != "CAMF_C"]
SIM_MODELS = ["SVD++", "CAMF_ICS", "CAMF_LCS", "CAMF_MCS"]


def _prec(flags):
    if flags & STRICT:
        return "strict-serial" if flags & SERIAL else "strict"
    return "f64" if flags & F64 else "f32"


def _cases():
    out = []

    def add(family, model, key, k, flags, env=None, **expect):
        out.append(Case(family, model, key, k, flags, _prec(flags), env or {}, expect))

    # sgd_level_fast_f32: exact rows (64, 128, 256) and the masked, ragged float4 form (68, 200).  Every model at k = 64, every k on two
    # or three models: the oracle runs of the premise at k >= 128 on 30 000 tuples are what the CPU suite pays for
    fast = {64: LEVEL_MODELS, 68: ("CAMF_CI", "CAMF_CUCI", "PMF"), 128: ("CAMF_CI", "BiasedMF"), 256: ("CAMF_CU", "PMF"),
            200: ("CAMF_CUCI", "BiasedMF")}
    for k, models in fast.items():
        for model in models:
            add("level-fast", model, "level-d4", k, NOCHAIN, kind="level")
    for model in LEVEL_MODELS:
        # sgd_level_generic: fp32 at a k no fast kernel takes, fp64, strict fp64; captured graph and plain launches
        for k, flags in ((70, 0), (70, NOGRAPH), (64, F64), (64, F64 | NOGRAPH), (5, F64 | STRICT), (130, F64 | STRICT | NOGRAPH)):
            add("level-generic", model, "generic", k, NOCHAIN | flags, kind="level")
    for model in ("CAMF_CI", "CAMF_CUCI", "BiasedMF", "PMF"):
        for k, nd in ((10, 4), (20, 6), (50, 5)):     # sgd_level_small_f32 with 4 / 8 / 16 lanes per tuple
            add("level-small", model, "level-d%d" % nd, k, NOCHAIN, kind="level")
    for model in ("CAMF_CI", "CAMF_CU", "BiasedMF"):
        for k, flags in ((128, 0), (10, 0), (70, 0), (8, F64 | STRICT)):    # tail_fast, tail_small, generic tail, strict
            add("tail", model, "tail", k, flags, tail=True)
    for model in ("CAMF_CI", "CAMF_CU", "CAMF_CUCI", "BiasedMF"):
        for hub in ("item", "user"):
            for k, flags in ((128, NOARENA), (128, ARENA), (10, NOARENA), (64, F64 | NOARENA), (64, F64 | ARENA)):
                add("chain", model, "chain", k, CHAIN | flags, {"CMI_CHAIN_HUB": hub}, kind="chain-" + hub, arena=bool(flags & ARENA))
    for model in LEVEL_MODELS:
        for hub in ("item", "user"):
            for team in (None, "all"):
                for k, flags in ((64, 0), (200, 0), (10, F64), (70, F64 | STRICT)):
                    if team and flags & STRICT:       # the strict owner epoch has no team form
                        continue
                    if k == 200 and model in ("CAMF_CUCI", "PMF"):
                        continue
                    add("owner", model, "owner", k, OWNER | flags, {"CMI_OWNER_HUB": hub, "CMI_OWNER_WAVES": None, "CMI_OWNER_TEAM": team},
                        kind="owner-" + hub, teams=team == "all")
    for model in util.MODELS:
        for k in (10, 64):
            for flags in (0, F64 | STRICT):           # sgd_serial_fast (fp32 tree dot), sgd_serial (the reference's operation order)
                add("serial", model, "serial", k, SERIAL | flags, {"CMI_NO_CAMFC_BLOCKS": "1", "CMI_NO_CAMFC_PIPE": "1"}, kind="serial")
    for k, flags in ((130, 0), (256, 0), (10, F64)):      # (at k = 64 the loss barely tells regU <-> regI apart on this data)
        add("camfc-blocks", "CAMF_C", "camfc-blocks", k, SERIAL | flags, kind="serial", blocks=True)
    for k, flags in ((64, 0), (200, 0), (10, F64), (128, F64)):
        add("camfc-pipe", "CAMF_C", "camfc-pipe", k, SERIAL | flags, {"CMI_NO_CAMFC_BLOCKS": "1", "CMI_NO_CAMFC_PIPE": None}, kind="serial",
            blocks=False)
    for model in SIM_MODELS:                          # ext_serial_strict; ext_serial_wave in fp64 and fp32
        env = {"CMI_NO_SVDPP_TEAM": "1"} if model == "SVD++" else {}
        add("ext", model, "sim", 10, SERIAL | F64 | STRICT, env)
        add("ext", model, "sim", 64, SERIAL | F64, env)
        add("ext", model, "sim", 64, SERIAL, env)
    for k, flags in ((64, 0), (64, F64), (100, 0)):   # svdpp_team: the workgroup-per-link kernel (the default for SVD++)
        add("svdpp-team", "SVD++", "svdpp-team", k, SERIAL | flags, {"CMI_NO_SVDPP_TEAM": None})
    for flags in (0, F64):                            # ... and its fallback for users beyond the LDS budget, with its own update body
        add("svdpp-team", "SVD++", "svdpp-heavy", 256, SERIAL | flags, {"CMI_NO_SVDPP_TEAM": None})
    return out


CASES = _cases()


def case_id(c):
    env = "-".join("%s" % v for v in c.env.values() if v is not None)
    return "%s-%s-k%d-%s-0x%x%s" % (c.family, c.model, c.k, c.prec, c.flags, "-" + env if env else "")


def premise_recipes():
    """every (model, data recipe, k) the GPU module trains, once, with the loosest bars among the cases that use it"""
    loosest = {}
    for c in CASES + PLUMBING:
        key = (c.model, c.key, c.k)
        state, loss = BARS[c.prec]
        old = loosest.get(key, (0.0, 0.0))
        loosest[key] = (max(old[0], state or 0.0), max(old[1], loss or 0.0))
    return sorted((m, key, k, bars) for (m, key, k), bars in loosest.items())


# the model-file case of the GPU module (strict fp64 on the plain levels; CAMF_CU names all four parameters) and the group case's data,
# model and k (the premise runs one oracle over the unsharded ratings; the GPU test merges one oracle per shard)
PLUMBING = [Case("model-file", "CAMF_CU", "generic", 10, NOCHAIN | F64 | STRICT, "strict", {}, {"kind": "level"}),
            Case("group", "CAMF_CI", "group", 32, F64, "f64", {}, {})]

CONF_LINE = "reg.lambda=0.05 -u 0.03 -i 0.07 -b 0.15 -c 0.31"     # the main value differs from all four options


def conf_line(regs, main="0.05"):
    return "reg.lambda=%s -u %s -i %s -b %s -c %s" % ((main,) + tuple(repr(float(np.float32(x))) if x else "0" for x in regs))


def depaul_conf(tmp_path, algo, line=CONF_LINE):
    """tests/golden/depaul_setting.conf for recommender `algo` with `line` as its reg.lambda line (the GPU module's config-to-kernel recipe)"""
    from tests.test_host_layer import _depaul_conf
    conf = _depaul_conf(tmp_path)
    txt = open(conf).read().replace("recommender=biasedmf", "recommender=" + algo)
    assert "reg.lambda=0.0001 -c 0.001" in txt
    open(conf, "w").write(txt.replace("reg.lambda=0.0001 -c 0.001", line))
    return conf


CONF_ALGO, CONF_ITERS = "camf_cu", 4      # CAMF_CU names all four parameters
