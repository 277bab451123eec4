#!/usr/bin/env python3
"""bench.py -- rating-updates/sec of the CAMF_CI k=128 SGD hot path on MI355X (BASELINE.json metric).

A "step" is one epoch of buildModel(): one pass of the fused gather-dot-AXPY update over every training
tuple, through the C ABI (libcarskit_mi355x.so), with tuples and model already resident in HBM.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--workload c3|northstar|c5|small] [--dump-outputs DIR] [--full]

N>1 is launched by the driver through torch.distributed.run (one rank per GPU): tuples are sharded by
user (each rank owns its own users and their ratings: weak scaling, per-GPU work fixed), the item-side
state (Q, icBias) is replicated and the mean of the ranks' per-epoch moves is applied after a reduce-scatter +
all-gather of one flat bucket over RCCL (carskit_amd/dist.py).  Prints ONE JSON line on rank 0: the BASELINE metric at fp32
state (`value`, `roofline` from the timed epochs' own HIP events).

A plain run does only what that line needs: set up, warm up, time the K steps, dump the outputs, print.  --full adds, after the
timed steps and the dump, every measurement that takes runs of its own: `cpu_baseline`; at N=1 a secondary `f64` object (the same
workload with the model kept in fp64, the reference's own precision), the part's measured ceilings (`roofline.peak_measured`), two
models side by side (`two_folds`), a `northstar` object (the shape BASELINE.json's north_star target sentence names: 10 M users x
1 M items x 64 conditions, 200 M ratings, timed the same way in the same run), the C5 / C4 / evalRankings objects and the box's
clocks; with --workload c4 the relaxed-sums form and the per-kernel roofline, with rank the one-stream kernel roofline, with
frappe / depaul one fold alone.

roofline.frac = HBM bytes the loaded SCHEDULE has to move (cmi_schedule_traffic: hub row / bias / context-bias row once per unit of
the hub-chain schedule, spoke row + tuple stream + scalar-bias sectors per tuple) / kernel time / 8 TB/s.  SURVEY 8(d)'s no-reuse
figure is kept beside it as `frac_algorithmic` (it can exceed 1 because the kernel keeps the hub row on chip); the committed
rocprofv3 PMC pass of the same command is the cross-check (`traffic`), and the run aborts if model and counters differ by > 5 %.
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from carskit_amd import capi, synth  # noqa: E402

# name -> (model, k, users, items, dims, conds/dim, ratings) ; per GPU
WORKLOADS = {
    # BASELINE.json configs[2]: the configuration the metric is quoted on that fits one GPU
    "c3": ("CAMF_CI", 128, 1_000_000, 100_000, 4, 8, 50_000_000),
    # BASELINE.json north_star target sentence: 10M users / 1M items / 64 conditions
    "northstar": ("CAMF_CI", 128, 10_000_000, 1_000_000, 4, 16, 200_000_000),
    "small": ("CAMF_CI", 128, 100_000, 10_000, 4, 8, 5_000_000),
    # BASELINE.json configs[4] per-GPU share: CAMF_CU k=256, 10M x 1M x 128 conditions, 500M ratings over 8 GPUs
    "c5": ("CAMF_CU", 256, 1_250_000, 1_000_000, 4, 32, 62_500_000),
}
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s measured achievable


def algorithmic_bytes(model, k, d, esize=4):
    """B = 16 + 4D + 16k + 8S + 8DT for fp32 state (int32 ids, compulsory traffic, no reuse).  With fp64
    state every model element and the rating double: B = 20 + 4D + 32k + 16S + 16DT."""
    s, t = {"BiasedMF": (2, 0), "PMF": (0, 0), "CAMF_C": (2, 1), "CAMF_CI": (1, 1), "CAMF_CU": (1, 1), "CAMF_CUCI": (0, 2)}[model]
    return 12 + esize + 4 * d + 4 * esize * k + 2 * esize * s + 2 * esize * d * t


def measured_traffic(workload, schedule):
    """HBM bytes per launch from the committed rocprofv3 PMC passes (profiles/<round>_<workload>_pmc.json, written
    by tools/pmc_summary.py from FETCH_SIZE/WRITE_SIZE runs of this same command); None if not collected for the schedule
    that is running."""
    import glob
    cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_%s_pmc.json" % workload)))
    for path in reversed(cands):
        d = json.load(open(path))
        if d.get("schedule", "level") == schedule:
            return d.get("hbm_bytes_per_launch"), os.path.relpath(path, ROOT)
    return None, None


def log(*a):
    print("[bench]", *a, file=sys.stderr, flush=True)


def cpu_baseline(model, k, data, state, gm, regs, lr, budget_tuples, rank_queries=None, fold_sets=None, sim=False):
    """The oracle (order-exact fp64 restatement of the Java loop, 1 thread) on a prefix of the same tuples; then five of them
    side by side = what the reference's `cv -k 5 -p on` (one Java thread per fold, CARSKit.java:395-412) gets out of the host.
    rank_queries = (test data, n): the evalRankings baseline instead -- the oracle's predict() per (query, candidate) pair + a stable sort."""
    from oracle import oracle_c
    if fold_sets is not None:
        # --workload frappe / depaul: the C restatement on the SAME folds -- fold 0 on one core, then all F folds on F threads
        def mk(tr, st, gm_):
            s64 = {n_: np.asarray(a, dtype=np.float64) for n_, a in st.items()}
            if sim:
                return oracle_c.SimOracle(model, k, tr.n_users, tr.n_items, tr.n_conds, tr.u, tr.j, tr.ctx, tr.r, tr.ctx_ptr, tr.ctx_conds,
                                          data.empty_conds, s64, gm_, *regs, n_ctx_dims=tr.n_dims)
            return oracle_c.Oracle(model, k, tr.n_users, tr.n_items, tr.n_conds, tr.u, tr.j, tr.ctx, tr.r, tr.ctx_ptr, tr.ctx_conds, s64, gm_, *regs)
        orcs = [mk(*fs) for fs in fold_sets]
        F, reps, n0 = len(orcs), 10, fold_sets[0][0].n
        t0 = time.perf_counter()
        for _ in range(reps):
            orcs[0].epoch(lr)
        one = (time.perf_counter() - t0) / reps
        ths = [threading.Thread(target=lambda o=o: [o.epoch(lr) for _ in range(reps)]) for o in orcs]      # the C call releases the GIL
        t0 = time.perf_counter()
        [t.start() for t in ths]
        [t.join() for t in ths]
        dtF = (time.perf_counter() - t0) / reps
        return {"value": n0 / one, "unit": "rating-updates/s", "cores": 1, "kind": "port",
                "sample": "%d epochs of fold 0 (%d tuples), fp64 order-exact C restatement, single thread (host has %d cores)" % (reps, n0, os.cpu_count() or 0),
                "five_fold": {"value": sum(fs[0].n for fs in fold_sets) / dtF, "cores": F, "seconds": dtF * reps,
                              "sample": "the same %d folds on %d threads, aggregate updates/s" % (F, F)}}
    if rank_queries is not None:
        test, nq = rank_queries
        orc = oracle_c.Oracle(model, k, data.n_users, data.n_items, data.n_conds, data.u, data.j, data.ctx, data.r, data.ctx_ptr,
                              data.ctx_conds, {n_: np.asarray(v, dtype=np.float64) for n_, v in state.items()}, gm, *regs)
        cand = np.unique(data.j).astype(np.int32)
        qs = list(zip(test.u[:nq].tolist(), test.ctx[:nq].tolist()))
        t0 = time.perf_counter()
        for (u, c) in qs:
            np.argsort(-orc.predict_items(u, c, cand), kind="stable")[:10]
        dt = time.perf_counter() - t0
        return {"value": len(qs) / dt, "unit": "queries/s", "cores": 1, "kind": "port",
                "sample": "%d queries x %d candidates: the C oracle's predict() per pair + a stable sort" % (len(qs), len(cand))}
    m = min(data.n, budget_tuples)

    def make():
        st = {n: np.asarray(a, dtype=np.float64) for n, a in state.items()}
        return oracle_c.Oracle(model, k, data.n_users, data.n_items, data.n_conds, data.u[:m], data.j[:m], data.ctx[:m],
                               data.r[:m], data.ctx_ptr, data.ctx_conds, st, gm, *regs)
    orc = make()
    t0 = time.perf_counter()
    orc.epoch(lr)
    dt = time.perf_counter() - t0
    out = {"value": m / dt, "unit": "rating-updates/s", "cores": 1, "kind": "port",
           "sample": "1 epoch over the first %d tuples of the same workload, fp64 order-exact C restatement of the "
                     "Java loop, single thread (host has %d cores; the reference loop is single-threaded per fold)"
                     % (m, os.cpu_count() or 0), "seconds": dt}
    folds = [orc] + [make() for _ in range(4)]
    ths = [threading.Thread(target=o.epoch, args=(lr,)) for o in folds]   # the C call releases the GIL
    t0 = time.perf_counter()
    [t.start() for t in ths]
    [t.join() for t in ths]
    dt5 = time.perf_counter() - t0
    out["five_fold"] = {"value": 5 * m / dt5, "cores": 5, "seconds": dt5,
                        "sample": "5 independent folds (5 threads) over the same prefix, aggregate updates/s"}
    return out


def make_instance(model, k, data, n_items, state, regs, gm, device, flags):
    inst = capi.Instance(model, k, data.n_users, n_items, data.n_conds, device=device, flags=flags)
    inst.set_hparams(*regs, gm)
    inst.set_ratings(data.u, data.j, data.ctx, data.r, data.ctx_ptr, data.ctx_conds)
    inst.set_states(state)
    return inst


def roofline(model, k, n_dims, data_n, info, sched, kern_ms, esize, workload):
    """HBM roofline of the epoch's dominant kernel.  Numerator = bytes the schedule that ran has to move (`sched`, from
    cmi_schedule_traffic, scattered scalars billed at their 64-byte sectors); SURVEY 8(d)'s no-reuse bytes ride along as
    `*_algorithmic`; the PMC pass committed under profiles/ for this workload + schedule + dtype is the cross-check."""
    bpu = algorithmic_bytes(model, k, n_dims, esize)
    launches = info["levels"]
    sec = kern_ms * 1e-3
    achieved = sched["sector"] / sec / 1e9
    chain = info["kind"].startswith("chain")
    tname = "float" if esize == 4 else "double"
    traffic, src = measured_traffic(workload + ("" if esize == 4 else "_f64"), info["kind"])
    avg_us = kern_ms * 1e3 / launches
    out = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
           "bytes_model": "schedule: per unit hub row + hub bias sector + hub context-bias row (r+w once), per tuple spoke row r+w + "
                          "tuple stream + 64-B sectors of the scattered scalars (cmi_schedule_traffic)" if sched["models_reuse"] else
                          "schedule: both rows r+w + tuple stream + 64-B sectors of the scattered scalars per tuple (cmi_schedule_traffic)",
           "bytes_per_epoch": sched["sector"], "bytes_per_launch": sched["sector"] / launches,
           "bytes_per_update": sched["sector"] / data_n, "bytes_per_update_own_size_scalars": sched["own"] / data_n,
           # both rows of every tuple from HBM, no reuse -- what round 1/2 priced the run at; NOT a bound for the chain kernel
           "bytes_per_update_algorithmic": bpu, "achieved_algorithmic": data_n * bpu / sec / 1e9,
           "frac_algorithmic": data_n * bpu / sec / 1e9 / HBM_PEAK_GBS,
           # rocprofv3 PMC (FETCH_SIZE x2 + WRITE_SIZE per launch, tools/pmc_summary.py) of the same command, committed under profiles/
           "traffic": traffic, "traffic_source": src,
           "traffic_GBps": (traffic / avg_us / 1e3) if traffic else None,
           "traffic_over_model": (traffic * launches / sched["sector"]) if traffic else None,
           "traffic_over_algorithmic": (traffic * launches / (data_n * bpu)) if traffic else None,
           "kernel": ("sgd_chain_level<%s,%s,hub=%s>" % (tname, model, info["kind"][6:]) if chain
                      else "sgd_owner<%s,%s,hub=%s> (latency-bound by the hottest row's chain, not by HBM)" % (tname, model, info["kind"][6:])
                      if info["kind"].startswith("owner") else "sgd_level_fast_f32<%s,%d>" % (model, k // 64) if esize == 4 else "sgd_level_generic<double,%s>" % model),
           "schedule": info["kind"], "spoke_arena": sched.get("spoke_arena", False), "launches_per_epoch": launches,
           "units_per_epoch": info["flow_blocks"] if chain else None,
           "avg_launch_us": avg_us}
    if traffic and abs(out["traffic_over_model"] - 1.0) > 0.05:
        raise SystemExit("bench: the schedule-derived HBM bytes (%.1f MB per launch) and the PMC pass %s (%.1f MB per launch) differ by "
                         "more than 5 %% -- the roofline numerator is not trustworthy, fix the model or re-profile"
                         % (sched["sector"] / launches / 1e6, src, traffic / 1e6))
    return out


_PEAK_MEASURED = {}


def peak_measured(device):
    """The part's measured ceilings beside the spec peak, once per run: a device-to-device copy and random 512-byte row read-modify-write
    (cmi_measure_hbm over a 4 GiB scratch buffer, best of 3 after warm-up).  Every SGD object of the line carries them, so a fraction
    can be read against the box's own pattern ceiling without opening profiles/."""
    if device not in _PEAK_MEASURED:
        try:
            cp, rw = capi.measure_hbm(device, 4 << 30)
            _PEAK_MEASURED[device] = {"copy_GBps": cp, "random_512B_row_rw_GBps": rw,
                                      "method": "cmi_measure_hbm over a 4 GiB scratch buffer, best of 3 after warm-up"}
        except Exception as e:
            _PEAK_MEASURED[device] = {"error": repr(e)}
    return _PEAK_MEASURED[device]


def with_measured(rf, device, enabled=True):
    """frac_of_measured_copy / _random_row: the same achieved GB/s against what this box's HBM delivers for a copy / for the row pattern."""
    if not enabled:
        return rf
    pm = peak_measured(device)
    rf["peak_measured"] = pm
    if "copy_GBps" in pm:
        rf["frac_of_measured_copy"] = rf["achieved"] / pm["copy_GBps"]
        rf["frac_of_measured_random_row"] = rf["achieved"] / pm["random_512B_row_rw_GBps"]
    return rf


def timed_epochs(inst, lr, steps, warmup):
    """W untimed + K timed epochs of one instance: (losses, wall seconds, mean HIP-event ms per epoch on the instance's stream)."""
    losses = [inst.train_epoch(lr) for _ in range(warmup)]
    inst.synchronize()
    t0 = time.perf_counter()
    ms = []
    for _ in range(steps):
        losses.append(inst.train_epoch(lr))
        ms.append(inst.last_epoch_ms())
    inst.synchronize()
    return losses, time.perf_counter() - t0, float(np.mean(ms))


DUMP_BUDGET = 64 << 20      # --dump-outputs: bytes written in all
DUMP_SEED = 12345           # the row sample of an output too large for its share of the budget


def dump_outputs(path, arrays, budget=DUMP_BUDGET):
    """--dump-outputs DIR: write what the timed path handed its caller after the last step, one DIR/<name>.npy per array (float32 or
    float64, as returned).  Smallest first, each array gets an equal share of what is left of the budget; one that does not fit is cut
    to a fixed, seeded sample of its rows (the same rows for the same shape), written with the row ids as DIR/<name>_rows.npy."""
    if not path:
        return
    os.makedirs(path, exist_ok=True)
    arrays = {n: np.atleast_1d(np.asarray(a)) for n, a in arrays.items()}
    for n, a in arrays.items():
        if a.dtype not in (np.float32, np.float64):
            arrays[n] = a.astype(np.float64)
    todo = sorted(arrays, key=lambda n: (arrays[n].nbytes, n))
    left = budget - 2 * 256 * len(todo)          # room for the .npy headers
    for i, name in enumerate(todo):
        a = arrays[name]
        share = left // (len(todo) - i)
        if a.nbytes > share:
            n_rows = max(1, share // (a.nbytes // a.shape[0] + 8))      # the rows and their float64 ids
            rows = np.sort(np.random.default_rng(DUMP_SEED).choice(a.shape[0], n_rows, replace=False))
            a = np.ascontiguousarray(a[rows])
            np.save(os.path.join(path, name + "_rows.npy"), rows.astype(np.float64))
            left -= rows.size * 8
        np.save(os.path.join(path, name + ".npy"), a)
        left -= a.nbytes
    log("dumped %d output(s) to %s" % (len(todo), path))


def secondary_workload(name, steps, warmup, device, flags, regs, lr, calibrate=True):
    """Another workload of WORKLOADS in the same run (the `northstar` object of the N=1 line): generated, scheduled, uploaded and
    timed exactly like the primary one, with its own roofline."""
    model, k, n_users, n_items, n_dims, cpd, n_ratings = WORKLOADS[name]
    t0 = time.perf_counter()
    data = synth.generate_fast(n_users, n_items, n_dims, cpd, n_ratings, seed=synth.DEFAULT_SEED)
    gm = float(data.r.sum() / np.count_nonzero(data.r))
    state = synth.init_state(model, data, k, seed=synth.DEFAULT_SEED + 2, dtype=np.float32)
    t1 = time.perf_counter()
    inst = make_instance(model, k, data, n_items, state, regs, gm, device, flags)
    setup_s = time.perf_counter() - t1     # cmi_create + cmi_set_ratings (schedule + tuple stream upload) + cmi_set_state
    info, sched = inst.schedule_info(), inst.schedule_traffic()
    log("%s: %d tuples generated in %.1fs, scheduled and uploaded in %.1fs: %s" % (name, data.n, t1 - t0, setup_s, info))
    del state
    losses, el, kern_ms = timed_epochs(inst, lr, steps, warmup)
    if not np.all(np.isfinite(losses)) or losses[-1] > losses[0]:
        raise SystemExit("bench: %s diverged (epoch losses %s)" % (name, losses))
    info, sched = inst.schedule_info(), inst.schedule_traffic()      # (the first epoch may have chosen table vs arena for this box)
    out = {"schedule_note": inst.schedule_note(),
           "workload": "%s: %s k=%d, %d users x %d items x %d conditions (%d dims), %d ratings, order-exact %s schedule"
                       % (name, model, k, data.n_users, n_items, data.n_conds, n_dims, data.n,
                          "hub-chain level" if info["kind"].startswith("chain") else "owner (dataflow)" if info["kind"].startswith("owner")
                          else "dependency-level"),
           "dtype": "f32", "value": data.n * steps / el, "unit": "rating-updates/s", "steps": steps, "warmup": warmup,
           "ms_per_step": el / steps * 1e3, "setup_s": setup_s, "levels_per_epoch": info["levels"], "first_loss": losses[0], "final_loss": losses[-1],
           "roofline": roofline(model, k, n_dims, data.n, info, sched, kern_ms, 4, name)}
    inst.close()
    with_measured(out["roofline"], device, calibrate)
    return out


def bench_fm(args):
    """--workload c4: one GPU's share of BASELINE configs[3] (FM k=64, 5 M users x 500 K items x 64 conditions, 200 M ratings over
    8 GPUs -> 625 K users / 25 M ratings per GPU).  A step = one ALS sweep (FM.java:148-218: 1 + 3 + 3k coordinate phases).  `value` is
    the DEFAULT form (fixed-order sums: two runs are bit-identical, like the reference's sweep); with --full, `relaxed_sums` beside it is the
    opt-in LDS-atomic form (CMI_FM_FLAG_RELAXED_SUMS) and `roofline` prices the dominant kernel, timed in runs of its own."""
    k, n_users, n_items, n = 64, 625_000, 500_000, 25_000_000
    data = synth.generate_fast(n_users, n_items, 4, 16, n)
    p = data.n_users + data.n_items + data.n_conds
    rng = np.random.default_rng(1)
    w_init, v_init = rng.random(p), 0.1 * rng.standard_normal((p, k))

    def timed(flags):
        g = capi.FMInstance(k, data.n_users, data.n_items, data.n_conds, data.n_dims, flags=flags)
        g.set_hparams(synth.java_float(0.01), synth.java_float(0.02))
        t_set = time.perf_counter()
        g.set_ratings(data.u, data.j, data.ctx, data.r)
        g.synchronize()
        setup_s = time.perf_counter() - t_set      # cmi_fm_set_ratings: the cell streams of both fields + the context order + uploads
        t_set = time.perf_counter()
        g.set_model(0.0, w_init, v_init)
        g.init()
        g.synchronize()
        model_s = time.perf_counter() - t_set      # cmi_fm_set_model + cmi_fm_init (the model's upload, err0 of every rating)
        for _ in range(args.warmup):
            g.sweep()
        g.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            g.sweep()
        g.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        if flags == 0 and args.dump_outputs:          # the default form's model after the last sweep
            w0, w, V = g.get_model()
            dump_outputs(args.dump_outputs, {"w0": np.float64(w0), "w": w, "V": V})
        ku = ki = lay = None
        if args.full:
            # the dominant kernel: the launch of a factor's user / item phase (65 + 65 of the ~390 launches of a sweep, 85 % of its time),
            # timed with HIP events on the instance's stream (in its non-updating form: it only writes scratch)
            ku, ki = g.time_reduce(4 + 3 * (k // 2) + 0, 10) * 1e-3, g.time_reduce(4 + 3 * (k // 2) + 1, 10) * 1e-3
            lay = g.layout()
        g.close()
        return dt, ku, ki, lay, setup_s, model_s

    dt, ku, ki, lay, setup_s, model_s = timed(0)
    phases = 4 + 3 * k
    config = {"workload": "c4 share: FM k=%d, %d users x %d items x %d conditions, %d ratings (one GPU of BASELINE configs[3])"
                          % (k, data.n_users, data.n_items, data.n_conds, data.n), "phases_per_sweep": phases,
              "form": "default: fixed-order sums, bit-reproducible (fm_cell_kernel)",
              "setup_s": setup_s, "set_model_and_init_s": model_s}
    out = {"metric": "FM ALS rating-sweeps/sec, k=%d" % k, "value": data.n / dt, "unit": "rating-sweeps/s", "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": dt * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64",
           "data": "synthetic", "config": config}
    if not args.full:
        return out
    rdt, rku, rki, rlay, _, _ = timed(capi.FM_FLAG_RELAXED_SUMS)
    # Bytes = what THIS implementation has to move per launch (cmi_fm_layout: 12-byte records streamed once, the coordinates' table entries
    # and sums, one L2 fill of every table slice per XCD) -- not the reference algorithm's errors[] + Q traffic, which it never generates.
    bytes_launch = 0.5 * (lay["bytes_reduce_user"] + lay["bytes_reduce_item"])
    rbytes_launch = 0.5 * (rlay["bytes_reduce_user"] + rlay["bytes_reduce_item"])
    kern, rkern = 0.5 * (ku + ki), 0.5 * (rku + rki)
    sweep_bytes = lay["bytes_per_factor"] * (k + 1)
    # HBM bytes per launch from the committed rocprofv3 PMC passes of tools/bench_fm.py (FETCH_SIZE x 2 + WRITE_SIZE, profiles/r*_c4_pmc.json)
    traffic, tsrc = None, None
    import glob
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_c4_pmc.json")), reverse=True):
        try:
            ks = json.load(open(path))["kernels"]
            vals = [v["hbm_bytes_per_dispatch"] for kk, v in ks.items() if "fm_cell_kernel" in kk and "true>" in kk and "hbm_bytes_per_dispatch" in v]
            if vals:
                traffic, tsrc = float(np.mean(vals)), os.path.relpath(path, ROOT)
                break
        except Exception:
            continue
    ref_bytes = 16 * (3 + 3 * k) + 16 * 3 * k
    out["relaxed_sums"] = {"form": "CMI_FM_FLAG_RELAXED_SUMS: LDS-atomic sums, last bits vary run to run (fm_cell_atomic_kernel)",
                           "value": data.n / rdt, "unit": "rating-sweeps/s", "ms_per_step": rdt * 1e3,
                           "kernel_us": {"user_field": rku * 1e6, "item_field": rki * 1e6},
                           "frac": rbytes_launch / rkern / 1e9 / HBM_PEAK_GBS}
    out["roofline"] = {"bound": "hbm", "achieved": bytes_launch / kern / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                       "frac": bytes_launch / kern / 1e9 / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": tsrc,
                       "traffic_GBps": traffic / kern / 1e9 if traffic else None, "traffic_over_model": traffic / bytes_launch if traffic else None,
                       "kernel": "fm_cell_kernel<0|1> (one factor's user / item phase, the default fixed-order form; fm_cell_atomic_kernel under "
                                 "CMI_FM_FLAG_RELAXED_SUMS: see relaxed_sums)",
                       "kernel_us": {"user_field": ku * 1e6, "item_field": ki * 1e6}, "bytes_per_launch": bytes_launch,
                       "bytes_per_rating_phase": bytes_launch / data.n,
                       "bytes_model": "this implementation's own traffic per launch (cmi_fm_layout): records 12 B x %d, "
                                      "coordinate entries + sums, table-slice fills; the reference ALGORITHM's errors[] + Q traffic would be %d B per "
                                      "rating-sweep (never generated here)" % (data.n, ref_bytes),
                       "whole_sweep_GBps": sweep_bytes / dt / 1e9, "whole_sweep_frac": sweep_bytes / dt / 1e9 / HBM_PEAK_GBS,
                       "limiter": "the memory pattern: 2.3 M stream lines from HBM + 8.3 M gather lines from L2 per launch (3 lanes per line) "
                                  "against ~400 outstanding lines per CU: time ~ sum(lines x latency) / (256 x 400), which also gives the "
                                  "stream-only (59 us) and lone-gather (119 us) microbenchmarks (tools/micro/gather16.hip; DESIGN.md 5); the "
                                  "fixed-order form adds the parking of a batch's products in LDS and its walk (+ ~11 %)",
                       "layout": lay, "avg_phase_us": dt * 1e6 / phases}
    return out


def bench_frappe(args):
    """--workload frappe: BASELINE configs[1]'s data set the way the reference runs it -- `cv -k F -p on`, F recommender instances side by
    side (CARSKit.java:395-412: one Java thread per fold) -- on ONE GPU: F instances of --model (default CAMF_C, k=64) on F streams, each
    training on the tuples outside its fold of the real Frappe file (tests/golden/frappe_compact.csv.gz through the product's DataTransformer
    + DataDAO; rating = 1 + log10(count), the scale the tests train on).  value = aggregate updates/s of the F concurrent folds; with --full,
    cpu_baseline = the C restatement on the same folds, one core and F threads, and config gets one fold timed alone.  These models are ONE
    dependent chain per instance (every rating updates parameters every other rating reads): the bound is the chain's latency, not HBM --
    the roofline object says so."""
    import gzip
    import math
    import tempfile
    from carskit_amd import dao
    depaul = args.workload == "depaul"      # BASELINE configs[0]'s file (5 043 ratings, ':na' conditions: the similarity models can run on it;
    #                                         on Frappe the reference's EmptyContextConditions.get(i) has nothing to return, CAMF_ICS.java:56)
    model = args.model or ("CAMF_ICS" if depaul else "CAMF_C")
    k = args.k if args.k > 0 else (10 if depaul else 64)
    F = max(1, args.folds)
    tmp = tempfile.mkdtemp(prefix="cmi_frappe_")
    if depaul:
        src = os.path.join(ROOT, "tests", "golden", "depaul_ratings_compact.csv")
    else:
        text = gzip.open(os.path.join(ROOT, "tests", "golden", "frappe_compact.csv.gz"), "rb").read().decode("utf-8").split("\n")
        rows = [text[0]]
        for ln in text[1:]:
            if ln:
                f_ = ln.split(",")
                f_[2] = "%.6f" % (1.0 + math.log10(int(f_[2])))
                ln = ",".join(f_)
            rows.append(ln)
        src = os.path.join(tmp, "frappe_log.csv")
        open(src, "w", encoding="utf-8").write("\n".join(rows))
    dao.transform(src, os.path.join(tmp, "train.csv"))
    d = dao.DataDAO(os.path.join(tmp, "train.csv")).rating_data()
    regs = (synth.java_float(1e-4), synth.java_float(1e-4), synth.java_float(1e-4), synth.java_float(1e-3))
    lr = synth.java_float(0.02) if model == "CAMF_C" else synth.java_float(0.02) / 8
    sim = model in ("CAMF_ICS", "CAMF_LCS", "CAMF_MCS")
    num_f = 10
    folds = []
    for f_ in range(F):
        tr = d.subset(np.flatnonzero((np.arange(d.n) % max(F, 5)) != f_)) if F > 1 else d
        tr.meta["num_f"] = num_f
        st = synth.init_state(model, tr, k, seed=synth.DEFAULT_SEED + f_, dtype=np.float32)
        if sim:
            st["P"] = (0.3 * st["P"]).astype(np.float32)
        gm = float(tr.r.sum() / np.count_nonzero(tr.r))
        # (the serial form is what the one-chain models run anyway; the row-local models -- BiasedMF, CAMF_CI / CU / CUCI -- get the schedule
        # cmi_set_ratings picks for the file: the owner epoch on Frappe's heavy-tailed items)
        chain_model = model in ("CAMF_C", "SVD++") or sim
        inst = capi.Instance(model, k, tr.n_users, tr.n_items, tr.n_conds, flags=args.flags | (capi.FLAG_SCHED_SERIAL if chain_model else 0))
        inst.set_hparams(*regs, gm)
        inst.set_device_share(F)
        if sim:
            inst.set_sim_params(num_f, tr.n_dims, d.empty_conds)
        inst.set_ratings(tr.u, tr.j, tr.ctx, tr.r, tr.ctx_ptr, tr.ctx_conds)
        inst.set_states(st)
        folds.append((inst, tr, st, gm))

    def run(steps):
        ths = [threading.Thread(target=lambda i=i: [i.train_epoch(lr) for _ in range(steps)]) for i, _, _, _ in folds]
        t0 = time.perf_counter()
        [t.start() for t in ths]
        [t.join() for t in ths]
        return time.perf_counter() - t0

    run(max(1, args.warmup))
    el = run(args.steps)
    if args.dump_outputs:           # every fold's last loss and model
        outs = {}
        for f_, (i, _, _, _) in enumerate(folds):
            outs["fold%d_loss" % f_] = np.float64(i.last_loss())
            outs.update({"fold%d_%s" % (f_, n): a for n, a in i.get_states(dtype=np.float32).items()})
        dump_outputs(args.dump_outputs, outs)
    one_ms = float(np.mean([i.last_epoch_ms() for i, _, _, _ in folds]))
    total = sum(tr.n for _, tr, _, _ in folds)
    bpu = algorithmic_bytes("CAMF_C", k, 8, 4)
    out = {"metric": "SGD rating-updates/sec, %s k=%d, %d concurrent folds" % (model, k, F), "value": total * args.steps / el, "unit": "rating-updates/s",
           "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": el / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": "f32",
           "data": "real (tests/golden/%s)" % ("depaul_ratings_compact.csv" if depaul else "frappe_compact.csv.gz, rating = 1 + log10(count)"),
           "config": {"workload": "%s: %s k=%d on the %s file (%d users x %d items x %d conditions, %d ratings), %d folds trained "
                                  "concurrently on one GPU, each on the tuples outside its fold (%d per fold)"
                                  % (args.workload, model, k, "DePaulMovie" if depaul else "Frappe", d.n_users, d.n_items, d.n_conds, d.n, F, folds[0][1].n),
                      "concurrent_folds": F, "schedule": folds[0][0].schedule_info()["kind"],
                      "fold_epoch_ms_while_concurrent": one_ms},
           "roofline": {"bound": "hbm", "achieved": total * args.steps * bpu / el / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": total * args.steps * bpu / el / 1e9 / HBM_PEAK_GBS, "traffic": None,
                        "kernel": "one serial wave / conflict-free block chain per instance (camfc_pipe.hip, ext_kernels.hip)",
                        "limiter": "latency of ONE dependent chain per instance (every rating updates parameters every other rating reads: "
                                   "CAMF_C's condBias, the similarity models' shared tables); the whole model is a few MB and cache-resident, "
                                   "HBM is idle -- the fraction is reported for form, the comparison that matters is cpu_baseline"}}
    if args.full:
        # one instance alone (no neighbours): what a fold costs when the GPU has nothing else to do
        t0 = time.perf_counter()
        for _ in range(args.steps):
            folds[0][0].train_epoch(lr)
        alone = (time.perf_counter() - t0) / args.steps
        out["config"].update(one_fold_alone_ms_per_epoch=alone * 1e3, one_fold_alone_updates_per_s=folds[0][1].n / alone)
    if args.full and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(model, k, d, None, 0.0, regs, lr, 0, fold_sets=[(tr, st, gm) for _, tr, st, gm in folds], sim=sim)
        out["vs_cpu_folds"] = out["value"] / out["cpu_baseline"]["five_fold"]["value"]
    for i, _, _, _ in folds:
        i.close()
    return out


def bench_group(args):
    """python bench.py --gpus N (no torchrun): one host process, one cmi_group over N GPUs (user-sharded; the library cuts the ratings,
    runs the shards' epochs concurrently and merges the item-side moves with RCCL reduce-scatter + all-gather).  Weak scaling: every
    GPU gets the workload's tuple count over its own users; items and contexts are shared (ONE context table: synth.merge_user_parts).
    CMI_BENCH_SHARE_GPU=1 puts every shard on device 0 (the in-process exchange): the form tests/test_gpu_bench_group.py runs on a
    one-GPU box -- a code-path check, never a measurement configuration (the line says so in config.parallelism)."""
    model, k, n_users, n_items, n_dims, cpd, n_ratings = WORKLOADS[args.workload]
    if args.k > 0:
        k = args.k
    if args.model:
        model = args.model
    W = args.gpus
    share = bool(os.environ.get("CMI_BENCH_SHARE_GPU"))
    if not share and capi.device_count() < W:
        raise SystemExit("--gpus %d: only %d device(s) visible" % (W, capi.device_count()))
    t0 = time.perf_counter()
    data = synth.merge_user_parts([synth.generate_fast(n_users, n_items, n_dims, cpd, n_ratings, seed=synth.DEFAULT_SEED + 1000 * r)
                                   for r in range(W)])
    log("group of %d: %d tuples (%d users, %d items, %d contexts in one table) generated in %.1fs"
        % (W, data.n, data.n_users, data.n_items, data.n_ctx, time.perf_counter() - t0))
    gm = float(data.r.sum() / np.count_nonzero(data.r))
    regs = (synth.java_float(1e-4), synth.java_float(1e-4), synth.java_float(1e-4), synth.java_float(1e-3))
    lr = synth.java_float(0.02)
    devices = [0] * W if share else list(range(W))
    g = capi.Group(model, k, data.n_users, n_items, data.n_conds, W, devices=devices, flags=args.flags)
    g.set_hparams(*regs, gm)
    t0 = time.perf_counter()
    g.set_ratings(data.u, data.j, data.ctx, data.r, data.ctx_ptr, data.ctx_conds)
    setup_s = time.perf_counter() - t0
    log("group of %d: schedules + upload in %.1fs" % (W, setup_s))
    state = synth.init_state(model, data, k, seed=synth.DEFAULT_SEED + 2, dtype=np.float32)   # user-side containers cover all W x n_users users
    g.set_states(state)
    del state
    losses = [g.train_epoch(lr) for _ in range(args.warmup)]
    comp, exch = [], []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        losses.append(g.train_epoch(lr))                 # returns after the global loss is on the host: every shard's stream is done
        c, x = g.last_times()
        comp.append(c)
        exch.append(x)
    elapsed = time.perf_counter() - t0
    if not np.all(np.isfinite(losses)) or (len(losses) > 1 and losses[-1] > losses[0]):
        raise SystemExit("bench: training diverged (epoch losses %s)" % losses)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, dict(loss=np.float64(losses[-1]), **g.get_states(dtype=np.float32)))
    comp, exch = np.asarray(comp, dtype=np.float64), np.asarray(exch, dtype=np.float64)     # [steps, W] HIP-event ms
    shards, bytes_epoch = [], 0.0
    for s in range(W):
        m = g.member(s)
        si, info, sched = g.shard_info(s), m.schedule_info(), m.schedule_traffic()
        bytes_epoch += sched["sector"]
        si.update({"schedule": info["kind"], "launches_per_epoch": info["levels"], "compute_ms": float(comp[:, s].mean()),
                   "exchange_ms": float(exch[:, s].mean()), "avg_launch_us": float(comp[:, s].mean()) * 1e3 / max(1, info["levels"]),
                   "schedule_bytes_per_epoch": sched["sector"],
                   "GBps": sched["sector"] / (float(comp[:, s].mean()) * 1e-3) / 1e9})
        shards.append(si)
    n_phys = len(set(devices))
    compute_ms = float(comp.max(axis=1).mean())          # the slowest shard's local epoch
    exchange_ms = float(exch.max(axis=1).mean())
    step_ms = elapsed / args.steps * 1e3
    peak = HBM_PEAK_GBS * n_phys
    bpu = algorithmic_bytes(model, k, n_dims, 4)
    rf = {"bound": "hbm", "achieved": bytes_epoch / (compute_ms * 1e-3) / 1e9, "peak": peak, "unit": "GB/s",
          "frac": bytes_epoch / (compute_ms * 1e-3) / 1e9 / peak,
          "bytes_model": "sum over the shards of the bytes their loaded schedule has to move per epoch (cmi_schedule_traffic) / the slowest "
                         "shard's local epoch (HIP events on its stream) vs %d x %.0f GB/s" % (n_phys, HBM_PEAK_GBS),
          "bytes_per_epoch": bytes_epoch, "bytes_per_update": bytes_epoch / data.n, "bytes_per_update_algorithmic": bpu,
          "frac_algorithmic": data.n * bpu / (compute_ms * 1e-3) / 1e9 / peak,
          # the same bytes over the WHOLE step (compute + exchange + host): what the aggregate updates/s is worth against N GPUs' HBM
          "frac_whole_step": bytes_epoch / (step_ms * 1e-3) / 1e9 / peak,
          "traffic": None, "kernel": "sgd_chain_level / sgd_level (per shard: config.shards[].schedule)",
          "avg_launch_us": [sh["avg_launch_us"] for sh in shards]}
    out = {"metric": "SGD rating-updates/sec, %s k=%d" % (model, k), "value": float(data.n) * args.steps / elapsed, "unit": "rating-updates/s",
           "n_gpus": W, "steps": args.steps, "warmup": args.warmup, "ms_per_step": step_ms, "higher_is_better": True,
           "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": "%s: %s k=%d, %d users x %d items per GPU, %d ratings per GPU, one context table of %d combinations"
                                  % (args.workload, model, k, n_users, n_items, n_ratings, data.n_ctx),
                      # the exchange the library really runs: RCCL after its pre-flight (one small exchange through RCCL and through the
                      # in-process path, both bit-identical to the host's sums), or the in-process peer-copy exchange -- by design when
                      # shards share a device, as the FALLBACK when RCCL failed to initialise or to pass the pre-flight on this node
                      "parallelism": "one process, cmi_group over %d shards on %d physical GPU(s) (user-sharded; exchange: %s)%s"
                                     % (W, n_phys, g.exchange_path(),
                                        " -- SHARED DEVICE: a code-path check (CMI_BENCH_SHARE_GPU), not a measurement" if share else ""),
                      "exchange": shards[0]["exchange"],
                      "setup_s": setup_s, "shards": shards},
           "compute_ms": compute_ms, "exchange_ms": exchange_ms, "host_ms": max(0.0, step_ms - compute_ms - exchange_ms),
           "exchange_bytes_per_shard": int(shards[0]["bucket_elems"]) * 4,
           "roofline": rf, "first_loss": losses[0], "final_loss": losses[-1]}
    g.close()
    return out


F32_MFMA_PEAK_TFLOPS = 157.3     # dense fp32 matrix peak (MI355X_MICROARCH.md): v_mfma_f32_32x32x2_f32


def rank_roofline(nq, n_cand, dev, flops, kern_ms):
    """The evaluation's device loop is two kernels.  `roofline` prices the CONTRACTION (rank_gemm_mfma_f32: S1 = [P[u] | 1] x [Q[j] | b_j]^T
    over the distinct query users) against the f32 matrix peak, by HIP events around its launches inside the loop.  The SELECTION
    (rank_topn_split) streams one S1 row and one S2 row per QUERY out of L2 / Infinity Cache (the S1 slab is written and read through HBM
    once): its rate rides along as `selection`."""
    g, t = kern_ms["contraction"] * 1e-3, kern_ms["selection"] * 1e-3
    out = {"bound": "mfma", "peak": F32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "achieved": flops / g / 1e12 if g else None,
           "frac": flops / g / 1e12 / F32_MFMA_PEAK_TFLOPS if g else None, "traffic": None,
           "kernel": "rank_gemm_mfma_f32 (v_mfma_f32_32x32x2_f32)", "flops": flops, "kernel_ms": g * 1e3,
           "timing": "HIP events around the contraction's launches on the instance stream, summed over the batches of one evaluation",
           "selection": {"kernel": "rank_topn_split<float>" if os.environ.get("CMI_RANK_NO_PRUNE") else "rank_topn_split_pruned<float>", "kernel_ms": t * 1e3,
                         "bytes_streamed": 2.0 * nq * n_cand * 4,
                         "GBps_through_L2": 2.0 * nq * n_cand * 4 / t / 1e9 if t else None,
                         "note": "one S1 row (shared by the user's queries: L2) and one S2 row (Infinity Cache) per query; bytes_streamed / GBps_through_L2 "
                                 "count EVERY candidate: the pruned selection skips the 64-candidate tiles whose bound cannot pass (~60 % here)"},
           "contraction_TFLOPs_over_whole_loop": flops / dev / 1e12}
    return out


def bench_rank(args):
    """--workload rank: Recommender.evalRankings (Recommender.java:668-964) for CAMF_CI k=128: every test (user, context) query scores
    ALL candidate items -- the one GEMM-shaped operation of this code base (f32 matrix cores).  A step = one whole evaluation."""
    model, k = "CAMF_CI", 128
    data = synth.generate_fast(50_000, 20_000, 4, 6, 2_000_000, seed=11)
    train, test = synth.split(data, 0.2, seed=3)
    state = synth.init_state(model, train, k, seed=5)
    inst = capi.Instance(model, k, train.n_users, train.n_items, train.n_conds, flags=args.flags)
    inst.set_hparams(1e-4, 1e-4, 1e-4, 1e-3, float(train.r.mean()))
    inst.set_ratings(train.u, train.j, train.ctx, train.r, train.ctx_ptr, train.ctx_conds)
    inst.set_states(state)
    tr, te = (train.u, train.j, train.ctx, train.r), (test.u, test.j, test.ctx, test.r)
    for _ in range(args.warmup):
        inst.eval_rankings(tr, te, bin_thold=2.5, num_recs=10)
    ms, walls = [], []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        res = inst.eval_rankings(tr, te, bin_thold=2.5, num_recs=10)
        walls.append(time.perf_counter() - t0)
        dev_ms, flops = inst.last_rank_ms()
        ms.append(dev_ms)
        kern = inst.last_rank_kernel_ms()
    dev = float(np.mean(ms)) * 1e-3
    wall = float(np.mean(walls))
    nq = res["n_queries"]
    if args.dump_outputs:           # the measures of the last evaluation
        dump_outputs(args.dump_outputs, {m: np.float64(v) for m, v in res.items()})
    if args.full:
        # the two kernels ON THEIR OWN: in the timed evaluations the selection of batch b runs beside the contraction of batch b + 1 (two
        # streams), so their HIP-event times overlap and stretch each other; the roofline prices the contraction alone (one stream)
        overlapped = dict(kern)
        os.environ["CMI_RANK_ONE_STREAM"] = "1"
        try:
            one_dev = []
            for _ in range(3):
                inst.eval_rankings(tr, te, bin_thold=2.5, num_recs=10)
                one_dev.append(inst.last_rank_ms()[0])
                kern = inst.last_rank_kernel_ms()
        finally:
            del os.environ["CMI_RANK_ONE_STREAM"]
    n_cand = int(len(np.unique(train.j)))
    # value = queries / WALL time of the whole cmi_eval_rankings call (plan + uploads + scoring + lists back + measures), timed
    # around the C-ABI call on the host; the roofline object (--full) prices the device scoring loop (HIP events) against the f32 MFMA peak
    out = {"metric": "evalRankings queries/sec, %s k=%d" % (model, k), "value": nq / wall, "unit": "queries/s", "n_gpus": 1,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": wall * 1e3, "higher_is_better": True, "scaling": "weak",
           "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "config": {"workload": "rank: %s k=%d, %d users x %d items, %d queries x %d candidates, top-10" %
                                  (model, k, train.n_users, train.n_items, nq, int(len(np.unique(train.j)))),
                      "device_ms_per_step": dev * 1e3, "device_queries_per_s": nq / dev, "host_wall_over_device": wall / dev,
                      "host_ms_breakdown_last_step": inst.last_rank_host_ms(),
                      "note": "value = queries / host wall clock of the whole call: the plan (candidates, queries, exclusions; host threads), "
                              "uploads, the device scoring loop, and the per-query measures computed batch by batch behind the device"},
           "AUC10": res["AUC10"]}
    if args.full:
        out["roofline"] = rank_roofline(nq, n_cand, dev, flops, kern)
        out["roofline"]["kernel_ms_while_overlapped"] = overlapped
        out["roofline"]["device_ms_one_stream"] = float(np.mean(one_dev[1:]))
        out["roofline"]["timing"] = ("contraction and selection timed on ONE stream (CMI_RANK_ONE_STREAM=1, HIP events around their launches, summed over "
                                     "the batches of an evaluation); the timed evaluations overlap them on two streams (kernel_ms_while_overlapped)")
    if args.full and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(model, k, train, state, float(train.r.mean()), (1e-4, 1e-4, 1e-4, 1e-3), 0.0, 0, rank_queries=(test, 200))
    inst.close()
    return out


def box_state():
    """What the box reports about itself (rocm-smi), kept beside the numbers: the same library measures 41.6 ms per C5 epoch on one
    MI355X box and 50.5 ms on another, so a line says which kind of box it ran on.  Never fails the bench."""
    import re
    import subprocess
    try:
        txt = subprocess.run(["rocm-smi", "--showtemp", "--showclocks", "--showpower", "--showmemuse"], capture_output=True, text=True,
                             timeout=20).stdout
    except Exception as e:
        return {"error": repr(e)}
    out = {}
    for key, pat in (("mclk_MHz", r"GPU\[0\].*mclk clock level: \d+: \((\d+)Mhz\)"), ("sclk_MHz", r"GPU\[0\].*sclk clock level: \d+: \((\d+)Mhz\)"),
                     ("fclk_MHz", r"GPU\[0\].*fclk clock level: \d+: \((\d+)Mhz\)"),
                     ("temp_junction_C", r"GPU\[0\].*Sensor junction\) \(C\): ([0-9.]+)"), ("temp_memory_C", r"GPU\[0\].*Sensor memory\) \(C\): ([0-9.]+)"),
                     ("power_W", r"GPU\[0\].*Package Power \(W\): ([0-9.]+)")):
        m = re.search(pat, txt)
        if m:
            out[key] = float(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="c3", choices=sorted(WORKLOADS) + ["c4", "rank", "frappe", "depaul"],
                    help="c3 (default) / northstar / c5 / small: the SGD hot path; c4: one GPU's share of the FM configuration (ALS sweep); "
                         "rank: evalRankings (top-N scoring on the f32 matrix cores)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run every secondary measurement: CPU baseline, fp64 leg, HBM calibration, two "
                         "models side by side, north_star shape, C5 / C4 / evalRankings objects, box clocks, per-kernel rooflines "
                         "(~1.5 min for the default workload); the --no-* options below leave parts of it out")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-tuples", type=int, default=20_000_000)
    ap.add_argument("--no-f64", action="store_true", help="skip the secondary fp64-state measurement")
    ap.add_argument("--f64-steps", type=int, default=3)
    ap.add_argument("--no-calibration", action="store_true", help="skip the in-run HBM calibration kernels")
    ap.add_argument("--no-northstar", action="store_true",
                    help="skip the `northstar` object (the north_star target shape, 200 M ratings: ~1.5 min of generation + upload)")
    ap.add_argument("--northstar-steps", type=int, default=5)
    ap.add_argument("--no-extras", action="store_true", help="skip the compact c5 / fm_c4 / rank objects of the default N=1 line (~1 min)")
    ap.add_argument("--f64-primary", action="store_true", help="profiling knob: the PRIMARY measurement keeps the model in fp64 (PMC passes of the fp64 kernel)")
    ap.add_argument("--merge", default="mean", choices=("mean", "sum"), help="multi-GPU merge rule of the item-side moves")
    ap.add_argument("--flags", type=int, default=0, help="extra cmi_create flags (e.g. 16 = no hipGraph, 256 = no hub-chain)")
    ap.add_argument("--k", type=int, default=0, help="experiment knob: override the workload's num.factors")
    ap.add_argument("--model", default="", help="experiment knob: override the workload's recommender")
    ap.add_argument("--item-zipf", type=float, default=0.0,
                    help="stress knob (SURVEY 8d): draw items from Zipf(a) instead of uniformly (slow generator; use with --workload small)")
    ap.add_argument("--folds", type=int, default=1,
                    help="independent recommender instances per GPU trained concurrently (the reference's `cv -p on`: "
                         "one thread per fold), each on its own stream; value then aggregates all of them")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned in its last step as DIR/<name>.npy (float32/64, "
                         "at most 64 MB in all: a fixed, seeded row sample of larger outputs), to compare two builds output for output")
    args = ap.parse_args()

    if args.workload in ("c4", "rank", "frappe", "depaul"):
        if args.gpus != 1:
            raise SystemExit("--workload %s is a single-GPU measurement (FM over ranks: carskit_amd.dist.ShardedFMRunner, tests/test_dist_fm_gloo.py)" % args.workload)
        print(json.dumps({"c4": bench_fm, "rank": bench_rank, "frappe": bench_frappe, "depaul": bench_frappe}[args.workload](args)), flush=True)
        return
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            # not under torch.distributed.run: ONE process drives all N GPUs through cmi_group_* -- the form the Java / C++ hosts use
            # (-Dcarskit.shards=N).  Same weak-scaling workload, same exchange function (group_api.cpp exchange_collective) as the
            # one-process-per-GPU form below.
            print(json.dumps(bench_group(args)), flush=True)
            return
        raise SystemExit("WORLD_SIZE=%d does not match --gpus %d" % (world, args.gpus))

    import torch
    dist = None
    if world > 1:
        import torch.distributed as dist
        if os.environ.get("CMI_BENCH_SHARE_GPU"):
            # test hook (tests/test_gpu_bench_ranks.py): two ranks on ONE GPU over gloo, to exercise this N>1 code path on
            # a single-GPU box; never a measurement configuration
            local_rank = 0
            torch.cuda.set_device(0)
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local_rank)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    model, k, n_users, n_items, n_dims, cpd, n_ratings = WORKLOADS[args.workload]
    if args.k > 0:
        k = args.k
    if args.model:
        model = args.model
    t0 = time.perf_counter()
    # every rank owns its own users (seeded by rank); items and contexts are the shared, replicated side
    if args.item_zipf > 0:
        data = synth.generate(n_users, n_items, n_dims, cpd, n_ratings, seed=synth.DEFAULT_SEED + 1000 * rank,
                              item_zipf=args.item_zipf)
    else:
        data = synth.generate_fast(n_users, n_items, n_dims, cpd, n_ratings, seed=synth.DEFAULT_SEED + 1000 * rank)
    log("rank %d: generated %d tuples (%d users, %d items, %d contexts) in %.1fs"
        % (rank, data.n, data.n_users, data.n_items, data.n_ctx, time.perf_counter() - t0))
    regs = (synth.java_float(1e-4), synth.java_float(1e-4), synth.java_float(1e-4), synth.java_float(1e-3))
    lr = synth.java_float(0.02)
    if world > 1:   # SparseMatrix.getGlobalAvg over ALL ranks' tuples
        from carskit_amd import dist as cdist
        gm = cdist.global_mean(dist, data.r, device="cuda")
    else:
        gm = float(data.r.sum() / np.count_nonzero(data.r))
    t0 = time.perf_counter()
    es = 8 if args.f64_primary else 4
    if args.f64_primary:
        args.flags |= capi.FLAG_STATE_F64
        args.no_f64 = True
    state = synth.init_state(model, data, k, seed=synth.DEFAULT_SEED + 2, dtype=np.float64 if es == 8 else np.float32)
    if world > 1:
        # item-side state must start identical on every rank; user-side differs per rank
        # (only the user-side containers this model owns: CAMF_CU / CAMF_CUCI / PMF have no userBias)
        rng_u = np.random.default_rng(synth.DEFAULT_SEED + 7 + rank)
        state["P"] = (0.1 * rng_u.standard_normal(state["P"].shape)).astype(np.float32)
        if "userBias" in state:
            state["userBias"] = (0.1 * rng_u.standard_normal(state["userBias"].shape)).astype(np.float32)
        if "ucBias" in state:
            state["ucBias"] = rng_u.random(state["ucBias"].shape).astype(np.float32)
    log("rank %d: init state in %.1fs" % (rank, time.perf_counter() - t0))

    t0 = time.perf_counter()
    inst = make_instance(model, k, data, n_items, state, regs, gm, local_rank, args.flags)
    setup_s = time.perf_counter() - t0     # cmi_create + cmi_set_ratings (schedule construction + tuple stream upload) + cmi_set_state
    info, sched = inst.schedule_info(), inst.schedule_traffic()
    log("rank %d: schedule + upload in %.1fs: %s" % (rank, setup_s, info))

    trainer = None
    preflight = None
    if world > 1:
        # pre-flight: one epoch + exchange of a small problem through the exchange this job will use and through the
        # torch-issued form, compared across ranks and with each other, BEFORE anything is timed; if the library-issued RCCL exchange is
        # unusable on this node every rank switches to the torch-issued one (CMI_DIST_TORCH=1) and the line says so
        tiny = synth.generate_fast(4000, 600, n_dims, cpd, 100_000, seed=synth.DEFAULT_SEED + 555 + 1000 * rank)
        tiny_state = synth.init_state(model, tiny, k, seed=synth.DEFAULT_SEED + 3, dtype=np.float32)
        tiny_insts = []

        def make_runner(force_torch):
            old = os.environ.pop("CMI_DIST_TORCH", None)
            if force_torch:
                os.environ["CMI_DIST_TORCH"] = "1"
            try:
                ti = make_instance(model, k, tiny, 600, tiny_state, regs, 3.0, local_rank, args.flags)
                tiny_insts.append(ti)
                return cdist.ShardedEpochRunner(ti, dist, device_index=local_rank, merge=args.merge)
            finally:
                os.environ.pop("CMI_DIST_TORCH", None)
                if old is not None:
                    os.environ["CMI_DIST_TORCH"] = old

        t_pf = time.perf_counter()
        preflight = cdist.preflight_exchange(make_runner, lambda run: {n: run.engine.inst.get_state(n) for n in cdist.ITEM_SIDE[model]}, dist, lr=lr)
        preflight["seconds"] = time.perf_counter() - t_pf
        for ti in tiny_insts:
            ti.close()
        if not preflight["ok"]:
            log("rank %d: exchange pre-flight FAILED (%s): every rank uses the torch-issued exchange" % (rank, preflight["note"]))
            os.environ["CMI_DIST_TORCH"] = "1"
        trainer = cdist.ShardedEpochRunner(inst, dist, device_index=local_rank, merge=args.merge)
    extra = []
    if args.folds > 1:
        if world > 1:
            raise SystemExit("--folds is a single-GPU mode")
        for _ in range(args.folds - 1):        # further folds: same tuples, independent models and streams
            extra.append(make_instance(model, k, data, n_items, state, regs, gm, local_rank, args.flags))

    def step():
        if trainer is not None:
            return trainer.epoch(lr)
        if extra:
            ths = [threading.Thread(target=o.train_epoch, args=(lr,)) for o in extra]
            [t.start() for t in ths]
            loss = inst.train_epoch(lr)
            [t.join() for t in ths]
            return loss
        return inst.train_epoch(lr)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        inst.synchronize()

    losses = []
    for _ in range(args.warmup):
        losses.append(step())
    barrier()
    # the first training call may have chosen between the table and the arena form of the spoke rows for THIS box (spoke tables of
    # 256 MiB .. 2 GiB: cmi_api.cpp arena_probe): price the roofline at the form that runs
    if args.warmup > 0:
        info, sched = inst.schedule_info(), inst.schedule_traffic()
    t0 = time.perf_counter()
    gpu_ms, exch_ms = [], []
    lib_comm = trainer is not None and getattr(trainer.engine, "lib_comm", False)
    for _ in range(args.steps):
        losses.append(step())
        gpu_ms.append(inst.last_epoch_ms())
        if lib_comm:
            exch_ms.append(inst.comm_last_exchange_ms())   # HIP events around pack .. loss all-reduce on the instance's stream
    barrier()
    elapsed = time.perf_counter() - t0
    # a diverging run is not a measurement: the loss must be finite and must not have grown over the run (one rate, no bold driver)
    if not np.all(np.isfinite(losses)) or (len(losses) > 1 and losses[-1] > losses[0]):
        raise SystemExit("bench: training diverged (epoch losses %s) -- throughput of a diverging run is not reported" % losses)
    if args.dump_outputs:
        # the last step's loss and the model(s) it left behind; with several ranks each writes its own shard under rank<r>_
        sdt = np.float64 if es == 8 else np.float32
        outs = {"loss": np.float64(losses[-1])}
        for f, o in enumerate([inst] + extra):
            outs.update({("fold%d_" % f if extra else "") + n: a for n, a in o.get_states(dtype=sdt).items()})
        if world > 1:
            outs = {"rank%d_%s" % (rank, n): a for n, a in outs.items()}
        dump_outputs(args.dump_outputs, outs, DUMP_BUDGET // world)
        del outs
    if dist is not None:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
        tot = torch.tensor([float(data.n), float(sched["sector"])], dtype=torch.float64, device="cuda")
        dist.all_reduce(tot)
        total_tuples, total_sched_bytes = float(tot[0].item()), float(tot[1].item())
        # the slowest rank's local epoch / exchange (HIP events on each rank's own stream), and every rank's launch time
        tms = torch.tensor([float(np.mean(gpu_ms)), float(np.mean(exch_ms)) if exch_ms else -1.0], dtype=torch.float64, device="cuda")
        allms = [torch.zeros_like(tms) for _ in range(world)]
        dist.all_gather(allms, tms)
        rank_compute_ms = [float(t[0].item()) for t in allms]
        rank_exchange_ms = [float(t[1].item()) for t in allms]
    else:
        total_tuples = float(data.n) * args.folds

    if rank == 0:
        kern_ms = float(np.mean(gpu_ms))          # HIP events on the instance stream around one epoch's launches
        # with concurrent folds the streams overlap, so the per-stream event time no longer isolates one kernel:
        # use the wall time of the step for the aggregate
        if args.folds > 1:
            kern_ms = elapsed / args.steps * 1e3 / args.folds
        out = {
            "metric": "SGD rating-updates/sec, %s k=%d" % (model, k),
            "value": total_tuples * args.steps / elapsed,
            "unit": "rating-updates/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64" if es == 8 else "f32", "data": "synthetic",
            "config": {"workload": "%s: %s k=%d, %d users x %d items x %d conditions (%d dims), %d ratings per GPU, "
                                   "lr 0.02f reg 1e-4f regC 1e-3f, order-exact %s schedule"
                                   % (args.workload, model, k, data.n_users, n_items, data.n_conds, n_dims, data.n,
                                      "hub-chain level" if info["kind"].startswith("chain") else
                                      "owner (dataflow)" if info["kind"].startswith("owner") else "dependency-level"),
                       "levels_per_epoch": info["levels"], "first_loss": losses[0], "final_loss": losses[-1],
                       "concurrent_folds": args.folds,
                       "parallelism": "1 GPU" if world == 1 else
                       "user-sharded x%d + RCCL reduce-scatter/all-gather of item-side moves (%s merge); exchange issued by: %s"
                       % (world, args.merge, getattr(trainer.engine, "exchange_path", "torch.distributed"))
                       + ("" if preflight is None else
                          ("; pre-flight FAILED (%s): FALLBACK to the torch-issued exchange" % preflight["note"] if not preflight["ok"] else
                           "; pre-flight (%.1f s): identical on every rank and equal to the torch-issued exchange" % preflight["seconds"]
                           if preflight["verified"] else
                           "; pre-flight (%.1f s): identical on every rank; NOT verified against the torch-issued exchange (%s)"
                           % (preflight["seconds"], preflight["note"])))},
            "roofline": roofline(model, k, n_dims, data.n, info, sched, kern_ms, es, args.workload),
        }
        out["config"]["setup_s"] = setup_s
        if world > 1:
            # N ranks: `roofline` above is rank 0's kernel against ONE GPU's peak; `roofline_aggregate` is the job -- all ranks' schedule
            # bytes over the slowest rank's local epoch against N x 8 TB/s -- and the step splits into compute / exchange / host
            step_ms = elapsed / args.steps * 1e3
            cms, xms = max(rank_compute_ms), max(rank_exchange_ms)
            out["compute_ms"], out["exchange_ms"] = cms, (xms if xms >= 0 else None)
            out["host_ms"] = max(0.0, step_ms - cms - max(xms, 0.0))
            out["rank_compute_ms"], out["rank_exchange_ms"] = rank_compute_ms, (rank_exchange_ms if xms >= 0 else None)
            out["rank_avg_launch_us"] = [c * 1e3 / max(1, info["levels"]) for c in rank_compute_ms]
            out["roofline_aggregate"] = {"bound": "hbm", "peak": HBM_PEAK_GBS * world, "unit": "GB/s",
                                         "achieved": total_sched_bytes / (cms * 1e-3) / 1e9,
                                         "frac": total_sched_bytes / (cms * 1e-3) / 1e9 / (HBM_PEAK_GBS * world),
                                         "frac_whole_step": total_sched_bytes / (step_ms * 1e-3) / 1e9 / (HBM_PEAK_GBS * world),
                                         "bytes_per_epoch_all_ranks": total_sched_bytes}
        for o in extra:
            o.close()
        # --full: what the headline figure does not need, each part in runs of its own after the timed steps and the dump
        full = world == 1 and args.full
        if full and not args.no_calibration:
            inst.synchronize()
            with_measured(out["roofline"], local_rank)
        if full and args.folds == 1 and args.workload == "c3" and not args.no_extras and not args.item_zipf and trainer is None:
            # secondary line: TWO independent models of the same workload side by side on this GPU (two instances, two streams, two host
            # threads: the reference's `cv -p on`, CARSKit.java:395-412).  The second model fills the first one's level boundaries
            # (285 dependent launches per epoch, each with its pipeline ramp and drain): what a lone model's order-exact schedule leaves idle
            try:
                other = make_instance(model, k, data, n_items, state, regs, gm, local_rank, args.flags)

                def pair():
                    th = threading.Thread(target=other.train_epoch, args=(lr,))
                    th.start()
                    inst.train_epoch(lr)
                    th.join()
                pair()
                inst.synchronize()
                other.synchronize()
                t2 = time.perf_counter()
                for _ in range(3):
                    pair()
                inst.synchronize()
                other.synchronize()
                el2 = time.perf_counter() - t2
                rf2 = roofline(model, k, n_dims, data.n, info, sched, el2 / 3 * 1e3 / 2, 4, args.workload)
                out["two_folds"] = {"value": 2 * data.n * 3 / el2, "unit": "rating-updates/s", "steps": 3, "ms_per_step": el2 / 3 * 1e3,
                                    "note": "aggregate of two independent models trained side by side (ms_per_step = one epoch of BOTH)",
                                    "roofline": {"frac": rf2["frac"], "achieved": rf2["achieved"], "peak": rf2["peak"], "unit": rf2["unit"]}}
                other.close()
            except Exception as e:
                out["two_folds"] = {"value": None, "error": repr(e)}
        if full and not args.no_f64 and args.folds == 1:
            # secondary line: the same workload with the model kept in fp64 on the GPU (the reference's precision)
            try:
                inst.close()
                st64 = {n: a.astype(np.float64) for n, a in state.items()}
                i64 = make_instance(model, k, data, n_items, st64, regs, gm, local_rank, args.flags | capi.FLAG_STATE_F64)
                info64, sched64 = i64.schedule_info(), i64.schedule_traffic()
                del st64
                l64, el64, ms64 = timed_epochs(i64, lr, args.f64_steps, 1)
                out["f64"] = {"dtype": "f64", "value": data.n * args.f64_steps / el64, "unit": "rating-updates/s",
                              "steps": args.f64_steps, "ms_per_step": el64 / args.f64_steps * 1e3, "final_loss": l64[-1],
                              "roofline": roofline(model, k, n_dims, data.n, info64, sched64, ms64, 8, args.workload)}
                i64.close()
                with_measured(out["f64"]["roofline"], local_rank, not args.no_calibration)
            except Exception as e:
                out["f64"] = {"value": None, "error": repr(e)}
        if full and not args.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(model, k, data, state, gm, regs, lr, args.cpu_tuples)
            except Exception as e:  # the oracle is only the reported baseline, never the product path
                out["cpu_baseline"] = {"value": None, "error": repr(e)}
        if full and args.folds == 1 and args.workload == "c3" and not args.no_northstar and not args.item_zipf:
            # the shape the north_star target sentence is quoted on, driver-timed in the same run
            try:
                inst.close()
                del data, state
                out["northstar"] = secondary_workload("northstar", args.northstar_steps, args.warmup, local_rank, args.flags, regs, lr,
                                                      not args.no_calibration)
            except SystemExit:
                raise
            except Exception as e:
                out["northstar"] = {"value": None, "error": repr(e)}
            # ... and the other measured paths, so that the driver's own run times them too (VERDICT r2 "missing" item 6): one GPU's share of
            # C5 (CAMF_CU k=256), of C4 (FM ALS sweep) and the top-N evaluation -- compact objects, each with its own roofline
            if not args.no_extras:
                import copy
                small = copy.copy(args)
                small.steps, small.warmup, small.no_cpu_baseline, small.dump_outputs = 3, 1, True, None
                rk = copy.copy(small)
                rk.steps, rk.warmup = 8, 2      # an evaluation is 15 ms of which a third is host work: more of them, so that one disturbed call weighs less
                for key, fn in (("c5", lambda: secondary_workload("c5", 3, 1, local_rank, args.flags, regs, lr, not args.no_calibration)),
                                ("fm_c4", lambda: bench_fm(small)), ("rank", lambda: bench_rank(rk))):
                    try:
                        o = fn()
                        out[key] = {kk: o[kk] for kk in ("metric", "workload", "value", "unit", "steps", "ms_per_step", "setup_s", "dtype", "roofline", "config", "relaxed_sums")
                                    if kk in o}
                    except SystemExit:
                        raise
                    except Exception as e:
                        out[key] = {"value": None, "error": repr(e)}
        if full:
            out["box"] = box_state()     # read right after the timed work, clocks still up
            # the driver's record keeps `config`, `roofline` and `cpu_baseline` and drops every other key of the line: the secondary
            # workloads timed in this same run travel as five numbers each inside config; the full objects stay at
            # the top level for whoever reads the line itself
            sec = {}
            for key in ("northstar", "c5", "f64", "two_folds", "fm_c4", "rank"):
                o = out.get(key)
                if not isinstance(o, dict) or o.get("value") is None:
                    continue
                rf = o.get("roofline") or {}
                sec[key] = {"value": o["value"], "unit": o.get("unit"), "ms_per_step": o.get("ms_per_step"), "frac": rf.get("frac"),
                            "traffic_over_model": rf.get("traffic_over_model")}
                if key == "fm_c4" and isinstance(o.get("relaxed_sums"), dict):
                    sec["fm_c4_relaxed_sums"] = {"value": o["relaxed_sums"]["value"], "unit": o["relaxed_sums"]["unit"],
                                                 "ms_per_step": o["relaxed_sums"]["ms_per_step"], "frac": o["relaxed_sums"].get("frac"),
                                                 "traffic_over_model": None}
            if sec:
                out["config"]["secondary"] = sec
        if world == 1:
            out["roofline"]["note"] = ("frac = schedule-model bytes (what this schedule has to move: hub rows once per unit, spoke rows once per tuple) "
                                       "/ HIP-event kernel time / 8 TB/s; SURVEY 8(d)'s zero-reuse bytes_per_update_algorithmic exceed what the "
                                       "schedule moves (hub rows stay on chip for ~4.5 tuples), so frac_algorithmic may exceed 1 without any "
                                       "update being skipped (tests/test_gpu_fullsize.py holds all updates of the epoch to the oracle)")
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
