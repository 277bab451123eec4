/*
 * carskit_mi355x.h -- C ABI of libcarskit_mi355x.so: the MI355X (gfx950) replacement for the
 * per-rating SGD inner loop of buildModel() in CARSKit's BiasedMF / CAMF_C / CAMF_CI / CAMF_CU /
 * CAMF_CUCI recommenders, plus the numeric part of evalRatings().
 *
 * The reference (irecsys/CARSKit v0.4.0) is Java and has no FFI of its own; this is the surface a
 * JNI shim (see INTEGRATION.md and java/) binds.  Every entry point names the reference code it
 * stands in for (paths relative to the reference root).  Plain pointers and sizes only; the
 * caller owns every host buffer; the library owns the device copies.
 *
 * Threading: a handle is an independent recommender instance bound to one GPU; different handles
 * may be used from different threads concurrently (the reference runs one Java thread per CV
 * fold, src/carskit/main/CARSKit.java:395-412).  One handle must not be used from two threads at
 * once.  No process-global state.
 *
 * Errors: every function returns CMI_OK (0) or a negative CMI_E_* code; cmi_last_error() gives
 * the message (the reference throws checked Exceptions, src/carskit/generic/Recommender.java:319;
 * the JNI shim turns a non-zero status into a RuntimeException).  There is NO CPU fallback: without
 * a HIP device every compute entry point fails with CMI_E_NO_DEVICE.
 */
#ifndef CARSKIT_MI355X_H
#define CARSKIT_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMI_ABI_VERSION 5 /* 5: round 6 -- CMI_E_BUSY; cmi_group_exchange_path (RCCL pre-flight + fallback); FM: the fixed-order (bit-reproducible) sweep is the DEFAULT, CMI_FM_FLAG_RELAXED_SUMS opts into the
                             LDS-atomic form (CMI_FM_FLAG_DETERMINISTIC is still accepted and now changes nothing)
                             4: round 5 -- ADDED cmi_group_last_times, cmi_comm_last_exchange_ms (exchange vs compute time of an epoch),
                             cmi_chain_schedule_device; CMI_E_HOST; CMI_FM_FLAG_DETERMINISTIC; cmi_fm_layout's [5..6] are batches
                             3: round 4 -- cmi_comm_*, cmi_fm_comm_*, group resident evaluation, FM layout / timing, ranking host
                             clock; REMOVED: CMI_FLAG_SCHED_FLOW, CMI_FLAG_TWO_LANE, cmi_flow_schedule, cmi_split_schedule */

/* status codes */
#define CMI_OK 0
#define CMI_E_INVALID (-1)    /* bad argument / bad call order */
#define CMI_E_NO_DEVICE (-2)  /* no HIP device (no CPU fallback exists) */
#define CMI_E_HIP (-3)        /* a HIP runtime call failed */
#define CMI_E_NUMERIC (-4)    /* loss became NaN/Inf (IterativeRecommender.java:181-184) */
#define CMI_E_UNSUPPORTED (-5)
#define CMI_E_HOST (-6)       /* a C++ exception (std::bad_alloc ...) reached the boundary: caught there, never thrown at the host;
                                 the JNI shim turns it into a RuntimeException like every other status (Recommender.java:1162-1171) */
#define CMI_E_BUSY (-7)       /* an owner (persistent) epoch was NOT launched: another process held the device's owner-epoch lock for the
                                 whole bounded wait, or the lock file cannot be opened (CMI_OWNER_NO_LOCK=1 waives it); model untouched */

/* recommender kinds = the `recommender=` names the reference's factory switch maps to the classes
 * this library accelerates (src/carskit/main/CARSKit.java:461,700-707) */
#define CMI_MODEL_BIASEDMF 0  /* src/carskit/alg/baseline/cf/BiasedMF.java */
#define CMI_MODEL_CAMF_C 1    /* src/carskit/alg/cars/adaptation/dependent/dev/CAMF_C.java */
#define CMI_MODEL_CAMF_CI 2   /* .../dev/CAMF_CI.java */
#define CMI_MODEL_CAMF_CU 3   /* .../dev/CAMF_CU.java */
#define CMI_MODEL_CAMF_CUCI 4 /* .../dev/CAMF_CUCI.java */
#define CMI_MODEL_PMF 5       /* src/carskit/alg/baseline/cf/PMF.java:47-82: BiasedMF without biases and without
                                 globalMean (predict = rowMult, IterativeRecommender.java:126-128); 2-D train matrix */
/* the remaining SGD recommenders of the same family (CARSKit.java:469,708-712).  Every rating updates parameters every other
 * rating reads (Y rows of all the user's items; the condition-similarity scalars / vectors / positions), so their exact semantics
 * are one dependent chain: CMI_FLAG_SCHED_SERIAL is required, as for CAMF_C.  cmi_set_sim_params must be called before
 * cmi_set_ratings for the three CAMF_*CS models. */
#define CMI_MODEL_SVDPP 6     /* src/carskit/alg/baseline/cf/SVDPlusPlus.java:46-146 (2-D train matrix, like BiasedMF) */
#define CMI_MODEL_CAMF_ICS 7  /* src/carskit/alg/cars/adaptation/dependent/sim/CAMF_ICS.java:33-133 */
#define CMI_MODEL_CAMF_LCS 8  /* .../sim/CAMF_LCS.java:34-147 */
#define CMI_MODEL_CAMF_MCS 9  /* .../sim/CAMF_MCS.java:38-166 */

/* state containers = the model fields a subclass must leave consistent
 * (IterativeRecommender.java:56-64, CAMF.java:40-42) */
#define CMI_STATE_P 0         /* DenseMatrix P        numUsers x k */
#define CMI_STATE_Q 1         /* DenseMatrix Q        numItems x k */
#define CMI_STATE_USER_BIAS 2 /* DenseVector userBias numUsers */
#define CMI_STATE_ITEM_BIAS 3 /* DenseVector itemBias numItems */
#define CMI_STATE_COND_BIAS 4 /* DenseVector condBias numConditions         (CAMF_C) */
#define CMI_STATE_UC_BIAS 5   /* DenseMatrix ucBias   numUsers x numConditions (CAMF_CU, CAMF_CUCI) */
#define CMI_STATE_IC_BIAS 6   /* DenseMatrix icBias   numItems x numConditions (CAMF_CI, CAMF_CUCI) */
#define CMI_STATE_Y 7         /* DenseMatrix Y            numItems x k                (SVD++, SVDPlusPlus.java:36) */
#define CMI_STATE_CC_MATRIX 8 /* SymmMatrix ccMatrix_ICS  numConditions x numConditions, exchanged as the full symmetric matrix (CAMF.java:45) */
#define CMI_STATE_CF_MATRIX 9 /* DenseMatrix cfMatrix_LCS numConditions x numF       (CAMF.java:46; numF from cmi_set_sim_params) */
#define CMI_STATE_C_VECTOR 10 /* DenseVector cVector_MCS  numConditions               (CAMF.java:47) */
#define CMI_STATE_COUNT 11

/* host buffer element types for cmi_set_state / cmi_get_state */
#define CMI_DTYPE_F32 0
#define CMI_DTYPE_F64 1

/* cmi_create flags.  CAMF_C updates the condBias vector shared by every tuple, so its tuples do not
 * commute and it requires CMI_FLAG_SCHED_SERIAL (cmi_create returns CMI_E_UNSUPPORTED otherwise). */
#define CMI_FLAG_STATE_F64 0x1u  /* keep the model in fp64 on the GPU (reference precision); default fp32 */
#define CMI_FLAG_SCHED_SERIAL 0x2u /* one wavefront walks the tuples in the reference's CRS order (exact for
                                      every model incl. CAMF_C; slow).  Default: dependency-level schedule --
                                      tuples that share no user and no item commute exactly, so the result equals
                                      the sequential order at equal precision while whole levels run in parallel */
#define CMI_FLAG_STRICT 0x4u     /* generic kernel + strictly left-to-right dot product (DenseMatrix.rowMult
                                      order) and, under SCHED_SERIAL, the reference's running-sum order for `loss`:
                                      with STATE_F64 the model (and under SERIAL the loss) is bit-identical to the
                                      Java arithmetic */
/* 0x20u, 0x40u: CMI_FLAG_SCHED_FLOW / CMI_FLAG_TWO_LANE of ABI 2 (round-1 experiments, measured slower than the level launches)
 * were removed in ABI 3; the bits are reserved */
#define CMI_FLAG_SCHED_CHAIN 0x80u /* force the hub-chain level schedule (the default whenever its levels are wide enough):
                                      consecutive tuples of one item (or user) whose other row is already final run back to
                                      back in one 16-lane group with the shared row, its bias and its context-bias row kept on
                                      chip; same result as the plain level schedule, bit for bit in fp32.
                                      CMI_E_UNSUPPORTED at cmi_set_ratings if the model/k has no chain kernel */
#define CMI_FLAG_NO_CHAIN 0x100u /* never use the hub-chain schedule (A/B runs against the plain level launches) */
#define CMI_FLAG_SCHED_OWNER 0x200u /* heavy-tailed degrees: ONE persistent launch per epoch in which every row of the heavy side
                                     * (items, or users) is owned by one wavefront that walks the row's tuples in CRS order with the
                                     * row in registers; the other side's rows travel between owners as tagged records
                                     * (owner_kernels.hip).  Order-exact like the level schedules; k <= 256 (fp64: 128), <= 384 conditions */
#define CMI_FLAG_NO_OWNER 0x400u /* never pick the owner schedule automatically (it is picked for >= 2^16 tuples whose dependency levels
                                  * are narrow -- heavy-tailed degrees -- when its estimated epoch is at least twice shorter) */
#define CMI_FLAG_SPOKE_ARENA 0x800u /* hub-chain schedule: keep the spoke rows in an arena of one slot per tuple, in schedule order -- the row
                                      of the tuple at stream position p is READ from slot p (a level's spoke reads become one sequential
                                      stream) and WRITTEN to the slot of the same row's next tuple.  Same arithmetic, same bits; costs
                                      tuples x k x 4 (8) bytes of HBM.  Picked automatically when the spoke table is >= 2 GiB (random 512-B
                                      rows over such a table run at 0.5 of the HBM peak, the arena form at 0.7) and the arena fits in 60 % of
                                      the free device memory; CMI_FLAG_NO_ARENA opts out */
#define CMI_FLAG_NO_ARENA 0x1000u
#define CMI_FLAG_NO_GRAPH 0x10u  /* launch the per-level kernels eagerly instead of replaying a hipGraph */

typedef struct cmi_instance *cmi_handle;

/* library / device probes (no reference counterpart) */
int cmi_abi_version(void);
int cmi_device_count(void); /* 0 when no HIP device is visible; never fails */
/* measurement: what this GPU sustains right now, GB/s (read + write bytes) over a scratch buffer of `bytes` (>= 1 MiB; use >= 2 GiB
 * to be past the 256 MB Infinity Cache): out[0] = streaming float4 copy, out[1] = random 512-byte-row read-modify-write (the SGD
 * kernels' row traffic pattern).  bench.py reports both beside the spec peak. */
int cmi_measure_hbm(int device, int64_t bytes, double out[2]);

/* new Recommender(trainMatrix, testMatrix, fold) + initModel() container allocation
 * (Recommender.java:180-275, IterativeRecommender.java:232-247, CAMF_CI.java:51-63 ...).
 * State is zero until cmi_set_state: the library never draws random numbers (the reference's
 * init stream is unseedable), the host injects the arrays. */
int cmi_create(int model, int k, int n_users, int n_items, int n_conds, int device, unsigned flags,
               cmi_handle *out);
int cmi_destroy(cmi_handle h);
/* message of the last failure on this handle; h == NULL: the last failure on this thread of cmi_create or of a handle-less cmi_*
 * function */
const char *cmi_last_error(cmi_handle h);

/* The training matrix: what `for (MatrixEntry me : trainMatrix)` yields, flattened
 * (CAMF_CI.java:80-86; librec SparseMatrix CSR arrays + DataDAO.getUserIdFromUI/getItemIdFromUI,
 * src/carskit/data/processor/DataDAO.java:1038-1046).  n tuples in CRS order: u[t], j[t] inner
 * user/item ids, ctx[t] context-combination id, r[t] rating.  ctx_ptr/ctx_conds (n_ctx+1 / nnz) is
 * ContextRecommender.getConditions (src/carskit/generic/ContextRecommender.java:53-61) as CSR.
 * BiasedMF: the 2-D `train` matrix (BiasedMF.java:62-66); ctx, ctx_ptr, ctx_conds may be NULL.
 * Builds the execution schedule (host integer work) and uploads. */
int cmi_set_ratings(cmi_handle h, int64_t n, const int32_t *u, const int32_t *j, const int32_t *ctx,
                    const double *r, int32_t n_ctx, const int32_t *ctx_ptr, const int32_t *ctx_conds);

/* copy-in at buildModel() entry / copy-back at exit of one model container (row-major, count
 * elements = rows*cols).  Converts between the host dtype and the device state dtype. */
int cmi_set_state(cmi_handle h, int which, const void *src, int64_t count, int dtype);
int cmi_get_state(cmi_handle h, int which, void *dst, int64_t count, int dtype);

/* CAMF_ICS / CAMF_LCS / CAMF_MCS: EmptyContextConditions (ContextRecommender.java:43 = the ":na" conditions in header order,
 * DataDAO.java:213-214; the i-th condition of a context is compared with empty_conds[i]), numF = `-f` of the CAMF_LCS option line
 * (CAMF_LCS.java:37; allocates cfMatrix_LCS), and rateDao.numContextDims() (CAMF_MCS.java:47: upbound = 1/sqrt(dims)).  Ignored
 * by the other models. */
int cmi_set_sim_params(cmi_handle h, int num_f, int n_ctx_dims, const int32_t *empty_conds, int n_empty);

/* regU/regI/regB/regC (IterativeRecommender.java:40,94-98: Java floats promoted to double) and
 * globalMean (Recommender.java:265) */
int cmi_set_hparams(cmi_handle h, double regU, double regI, double regB, double regC, double global_mean);

/* `cv -p on` (CARSKit.java:395-412: one thread per fold, every fold a recommender of its own): `instances` = how many instances the
 * host trains CONCURRENTLY on this handle's device.  A hint, not semantics: the persistent kernels (the owner epoch, one launch whose
 * wavefronts must all be resident) size their grids to 1 / instances of the device, so the instances' launches run side by side instead
 * of one after another; results are what they are without the hint (the schedules are order-exact).  Call before cmi_set_ratings.
 * Default 1.  instances < 1 -> CMI_E_INVALID. */
int cmi_set_device_share(cmi_handle h, int instances);

/* One pass of the `for (MatrixEntry me : trainMatrix) {...}` body + `loss *= 0.5`
 * (e.g. CAMF_CI.java:79-123) with learning rate lrate; *loss_out = the epoch's loss.  The host keeps
 * calling isConverged() itself (the Java drop-in does exactly this). */
int cmi_train_epoch(cmi_handle h, double lrate, double *loss_out);

/* Whole buildModel(): up to num_iters epochs with IterativeRecommender.isConverged/updateLRate
 * (IterativeRecommender.java:145-229) evaluated between epochs.  early_stop: 0 none, 1 loss.
 * losses/lrates (num_iters each, may be NULL) receive the per-epoch loss and the rate used;
 * *iters_run the number of epochs executed; *final_lrate (may be NULL) the lRate field afterwards.
 * NaN/Inf loss -> CMI_E_NUMERIC (the reference calls System.exit(-1)). */
int cmi_train(cmi_handle h, int num_iters, double init_lrate, double max_lrate, int bold_driver, double decay,
              int early_stop, double *losses, double *lrates, int *iters_run, double *final_lrate);

/* saveModel() / loadModel() (IterativeRecommender.java:249-292), as ONE documented, versioned, checksummed file holding every
 * container of the model (the reference serialises P, Q, userBias, itemBias with Java object streams and forgets condBias /
 * ucBias / icBias), the hyper-parameters of cmi_set_hparams, and the resume state of the epoch loop (the learning rate the next
 * epoch would use, the last epoch's loss, epochs done): training N epochs, saving, loading into a fresh handle and training M more
 * equals training N + M epochs.  Layout: carskit_amd/csrc/model_io.cpp.  cmi_load_model checks that the file matches the handle
 * (model, k, sizes) and its checksum before it changes anything; lrate / last_loss / epochs_done may be NULL.  Host I/O only (the
 * state moves through cmi_get_state / cmi_set_state).  NOT the reference's Java serialization format (no JVM to verify one). */
int cmi_save_model(cmi_handle h, const char *path, double lrate, double last_loss, int epochs_done);
int cmi_load_model(cmi_handle h, const char *path, double *lrate, double *last_loss, int *epochs_done);

/* cmi_train continued: epochs first_iter .. first_iter + num_iters - 1 of the same loop, prev_loss = the loss of epoch
 * first_iter - 1 (what isConverged()/updateLRate() compare with).  cmi_train == cmi_train_from(first_iter = 1, prev_loss = 0).
 * With cmi_save_model / cmi_load_model: N epochs, save, load, cmi_train_from(N + 1, ...) equals N + M epochs in one go. */
int cmi_train_from(cmi_handle h, int first_iter, double prev_loss, int num_iters, double init_lrate, double max_lrate,
                   int bold_driver, double decay, int early_stop, double *losses, double *lrates, int *iters_run,
                   double *final_lrate);

/* predict(u, j, c, bound) for n tuples (Recommender.java:306-317 + the model's predict());
 * bound != 0 clamps to [lo, hi].  ctx may be NULL for BiasedMF. */
int cmi_predict_batch(cmi_handle h, int64_t n, const int32_t *u, const int32_t *j, const int32_t *ctx, int bound,
                      double lo, double hi, double *out);

/* numeric part of Recommender.evalRatings (Recommender.java:504-594) over n test tuples whose ctx
 * ids index the SAME ctx_ptr/ctx_conds table given to cmi_set_ratings.
 * out[0]=MAE out[1]=RMSE out[2]=NMAE out[3]=rMAE out[4]=rRMSE; *count = tuples with non-NaN prediction */
int cmi_eval_ratings(cmi_handle h, int64_t n, const int32_t *u, const int32_t *j, const int32_t *ctx,
                     const double *r, double min_rate, double max_rate, double *out, int64_t *count);

/* ---- plumbing for the host layer (multi-GPU exchange, measurement); no reference counterpart ---- */

/* `--early-stop MAE|RMSE` evaluates the test set after every epoch (IterativeRecommender.java:156-161): upload the test tuples
 * once, then evaluate from device memory.  Same numbers as cmi_eval_ratings on the same tuples. */
int cmi_set_eval_ratings(cmi_handle h, int64_t n, const int32_t *u, const int32_t *j, const int32_t *ctx, const double *r);
int cmi_eval_resident(cmi_handle h, double min_rate, double max_rate, double out[5], int64_t *count);

/* ---- top-N ranking evaluation: Recommender.evalRankings (src/carskit/generic/Recommender.java:668-964) ----------
 * The reference scores every candidate item for every test (user, context) pair with one predict() call each
 * (O(queries x items x k)); here that scoring is one dense contraction per query batch plus a fused top-N selection
 * on the GPU, and only the per-query metric formulas (happy.coding.math.Measures via src/carskit/eval/Measures.java)
 * run on the host.
 *   train tuples  -> candidate items = items seen in training, in java.util.HashSet<Integer> iteration order
 *                    (DataDAO.getItemList, DataDAO.java:1210-1218); minus the num_ignore most-rated ones
 *                    (Recommender.java:720-735); and the per-(user, context) already-rated items that are skipped
 *                    (Recommender.java:793-816).  tr may be NULL (all entries non-zero).
 *   test tuples   -> queries: (user, context) pairs with at least one item rated > bin_thold that is a candidate
 *                    (DataDAO.getUserCtxList(sm, threshold), DataDAO.java:1114-1140; Recommender.java:776-790).
 *   score         -> ranking(u,j,c) = predict(u,j,c) unbounded (Recommender.java:1016-1018); kept if not NaN and
 *                    > bin_thold; sorted descending, ties in candidate order (stable Collections.sort); cut at num_recs.
 *   num_recs      -> `-topN`; must be >= 1 (the reference throws for a negative cut-off, Measures.java:13-16).
 *   strategy      -> CMI_RANK_UCU: mean over contexts per user, then over users; CMI_RANK_UC: mean over all pairs
 *                    (`evaluation.setup --rand-seed ... -strategy`, Recommender.java:856-926).  Stats.mean skips NaN.
 * out[21] = Pre5 Pre10 PreN Rec5 Rec10 RecN AUC5 AUC10 AUCN MAP5 MAP10 MAPN NDCG5 NDCG10 NDCGN MRR5 MRR10 MRRN D5 D10 DN
 * (D* = 0: diversity is off unless `-diverse`, which needs the item-similarity cache and is not built).
 * Optional per-query outputs (NULL to skip), sized for n_test queries: q_user/q_ctx/q_count[n] and
 * top_items/top_scores[n * num_recs] (inner item ids, -1 / NaN padded) -- the `-isResultsOut` list of the reference.
 * Context ids index the ctx table given to cmi_set_ratings (2-D models ignore the table). */
#define CMI_RANK_MEASURES 21
#define CMI_RANK_UCU 0
#define CMI_RANK_UC 1
int cmi_eval_rankings(cmi_handle h, int64_t n_train, const int32_t *tu, const int32_t *tj, const int32_t *tctx,
                      const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx,
                      const double *sr, double bin_thold, int num_recs, int num_ignore, int strategy,
                      double out[CMI_RANK_MEASURES], int64_t *n_queries, int32_t *q_user, int32_t *q_ctx,
                      int32_t *q_count, int32_t *top_items, double *top_scores);
/* measurement: GPU time (HIP events on cmi_stream()) of the most recent cmi_eval_rankings scoring loop (operand
 * gather + contraction + mask + top-N over all query batches) and the flops of its contraction
 * (2 x queries x candidates x padded operand length) */
int cmi_last_rank_ms(cmi_handle h, float *ms, double *flops);
/* host wall clock of the last cmi_eval_rankings call, milliseconds: out[0] plan (candidates, queries, exclusions), [1] setup (buffers,
 * uploads, item operands), [2] the scoring loop including the per-batch measures computed behind it, [3] tail (last batch's measures +
 * the averages), [4] the whole call */
int cmi_last_rank_host_ms(cmi_handle h, double out[5]);
/* GPU time of the last evaluation's two kernels, by HIP events around their launches inside the scoring loop, milliseconds summed over
 * the batches: out[0] the contraction (rank_gemm_mfma_f32), out[1] the selection (rank_topn_split); both 0 when the evaluation did not
 * run the split form (fp64 state, SVD++ / CAMF_ICS / LCS / MCS) */
int cmi_last_rank_kernel_ms(cmi_handle h, double out[2]);
/* host-only (no GPU): the bookkeeping cmi_eval_rankings does before scoring -- candidate items in HashSet<Integer> order minus the
 * `num_ignore` most rated (Recommender.java:704-735), the (user, context) queries with their correct items (:776-790), and per
 * query the candidate POSITIONS of the items already rated in that context (:793-816).  Call once with null arrays for
 * sizes = {n_cand, n_queries, n_truth, n_excl}, then with arrays (truth_ptr / excl_ptr hold n_queries + 1 offsets). */
int cmi_rank_plan(int32_t n_users, int32_t n_items, int64_t n_train, const int32_t *tu, const int32_t *tj, const int32_t *tctx,
                  const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx, const double *sr,
                  double bin_thold, int num_ignore, int64_t sizes[4], int32_t *cand, int32_t *q_user, int32_t *q_ctx,
                  int64_t *truth_ptr, int32_t *truth_items, int64_t *excl_ptr, int32_t *excl_idx);
/* host-only: the 18 measures of ONE ranked list exactly as cmi_eval_rankings computes them per query (out[measure*3 + cut-off],
 * measures Pre Rec AUC MAP NDCG MRR, cut-offs {5, 10, num_recs}); ranked = the list already cut at num_recs, truth = the query's
 * correct items in ascending order, num_dropped = candidates not listed (Recommender.java:850-858) */
int cmi_rank_list_measures(const int32_t *ranked, int len, const int32_t *truth_sorted, int n_truth, int num_dropped,
                           int num_recs, double out[18]);
/* iteration order of a java.util.HashSet<Integer> after add()ing values[0..n) (the candidate-item order above) */
int cmi_java_int_hashset_order(int64_t n, const int32_t *values, int32_t *out, int64_t *n_out);

/* device pointer of a state container (element type per CMI_FLAG_STATE_F64), so the host can run its
 * epoch-boundary exchange (RCCL all-reduce of item-side deltas) in place.  The table behind the pointer is current
 * when the call returns and host writes through it are honoured by the next epoch (a container whose live rows sit
 * in the spoke arena is re-read from the table); call it again after every training call before touching the memory. */
int cmi_state_device_ptr(cmi_handle h, int which, void **ptr, int64_t *count, int *dtype);
/* the HIP stream (hipStream_t) all of this handle's work is enqueued on */
int cmi_stream(cmi_handle h, void **stream);
/* Epoch-boundary exchange of the REPLICATED item-side containers when ratings are sharded by user over several GPUs
 * (carskit_amd/dist.py; the reference loop is sequential, CAMF_CI.java:79-123, so this has no counterpart there).  One flat
 * device buffer, the "bucket" (element type = state dtype), holds container after container (Q, then itemBias / icBias as the
 * model owns them; every segment padded to 4 elements, the total to a multiple of pad_to so that it splits evenly over the
 * ranks of a reduce-scatter) this rank's movement of the item-side state since the last snapshot:
 *   cmi_exchange_setup  allocates bucket + snapshot, snapshot = current state; returns the bucket's device address / length
 *   cmi_exchange_pack   bucket = state - snapshot                       -> the host sums the bucket over ranks (RCCL)
 *   cmi_exchange_apply  state = snapshot + scale * bucket; snapshot = state        (scale = 1/W: mean of the ranks' moves)
 * All enqueued on cmi_stream().  CAMF_C (shared condBias, serial-only) is not sharded: CMI_E_UNSUPPORTED. */
int cmi_exchange_setup(cmi_handle h, int64_t pad_to, void **bucket, int64_t *count);
int cmi_exchange_pack(cmi_handle h);
int cmi_exchange_apply(cmi_handle h, double scale);
/* device address of the double the most recent epoch's loss is left in (so the host can sum it over ranks on the device) */
int cmi_loss_device_ptr(cmi_handle h, void **ptr);
int cmi_synchronize(cmi_handle h);
/* enqueue one epoch without reading the loss back (pair with cmi_synchronize / cmi_last_loss) */
int cmi_train_epoch_async(cmi_handle h, double lrate);
int cmi_last_loss(cmi_handle h, double *loss_out);
/* schedule facts: info[0]=level launches per epoch (a long run of narrow final levels counts as ONE launch: a single
 * workgroup walks them),  info[1]=largest level, info[2]=tuples,
 * info[3]=max conditions per tuple (D), info[4]=state bytes on device, info[5]=tuple-stream bytes on device,
 * info[6]=schedule kind actually running (0 level launches, 1 serial, 2 and 3 reserved (schedules removed in ABI 3),
 * 4 hub-chain levels along items, 5 hub-chain levels along users; then info[1]=most units in a level, info[7]=units;
 * 6 owner epoch with items owned, 7 with users owned; then info[0]=1, info[1]=tuples of the busiest owner, info[7]=owners in the
 * low 32 bits and, in the high 32 bits, how many of them run as teams of three wavefronts),
 * info[7] for kind 1: CAMF_C's number of conflict-free CRS blocks its epoch is cut into (0: the serial wave); its former meaning
 * "workgroups of the dataflow launch" is reserved (removed in ABI 3) */
int cmi_schedule_info(cmi_handle h, int64_t info[8]);
/* host-only: the bookkeeping of the spoke arena (CMI_FLAG_SPOKE_ARENA).  spoke[p] = spoke row id of the tuple at stream position p;
 * next[p] = position of the next tuple of the same row, the last one wrapping to the first; first[row] = position of the row's first
 * tuple or -1 */
int cmi_arena_positions(int64_t n, const int32_t *spoke, int32_t n_spokes, int32_t *next, int32_t *first);
/* "" or one sentence saying why cmi_set_ratings could not pick the schedule the data calls for (heavy-tailed degrees outside the owner
 * epoch's limits: the order-exact level walk runs, correct but roughly 10x slower) -- visible to the host instead of silent */
const char *cmi_schedule_note(cmi_handle h);
/* HBM bytes one epoch of the loaded schedule has to move, derived from the schedule (no reference counterpart: measurement).
 * out[0]: every scattered scalar billed at its 64-byte sector, read and written (hub-chain schedules: hub row, hub bias and hub
 * context-bias row once per UNIT; spoke row, tuple stream, spoke bias and spoke context-bias cells per tuple); out[1]: the same with
 * scalars at their own size; out[2]: SURVEY 8(d)'s no-reuse algorithmic bytes; out[3]: bit 0 = on-chip hub reuse is modelled, bit 1 = the spoke arena is in use */
int cmi_schedule_traffic(cmi_handle h, int64_t out[4]);
/* GPU time of the most recent epoch's kernels measured with HIP events on cmi_stream() */
int cmi_last_epoch_ms(cmi_handle h, float *ms);

/* ---- one recommender over several GPUs from ONE host process (carskit_amd/csrc/group_api.cpp) -------------------------------
 * The reference trains one fold on one thread (CARSKit.java:395-412 is its only parallelism: a thread per fold) -- there is no
 * counterpart to translate.  SURVEY 8b's `device_mask` entry, as a handle of its own: ratings are sharded BY USER over n_shards
 * instances (contiguous user ranges holding about n / n_shards tuples each; user-side containers P, userBias, ucBias live on
 * exactly one shard), the item-side containers (Q, itemBias, icBias) are replicated and merged after every epoch:
 *     item_side = snapshot + (sum over shards of (item_side_shard - snapshot)) / n_shards        (the MEAN of the shards' moves)
 * through ncclReduceScatter + ncclAllGather over xGMI on the shards' own streams (librccl, one communicator per shard, grouped
 * calls), and the fp64 epoch losses are all-reduced, so cmi_group_train_epoch returns the GLOBAL loss and the unchanged host-side
 * isConverged()/updateLRate() keeps steering.  Shards that share a device use an in-process exchange
 * (sum in shard order on shard 0's stream) instead -- same arithmetic.  n_shards = 1 is exactly the single-instance path.
 * With n_shards > 1 this is NOT the reference's sequential semantics (n_shards local SGD streams merged per epoch): accuracy is
 * reported as a band against the 1-GPU result.  CAMF_C / SVD++ / CAMF_*CS are serial chains: 1 shard only.
 * Call order: create, set_hparams, set_ratings (creates the instances: their user counts depend on the cut), set_state, train.
 * devices: n_shards device indices (may repeat), or NULL = round robin over the visible devices. */
typedef struct cmi_group *cmi_group_handle;
int cmi_group_create(int model, int k, int n_users, int n_items, int n_conds, int n_shards, const int *devices, unsigned flags,
                     cmi_group_handle *out);
int cmi_group_destroy(cmi_group_handle g);
const char *cmi_group_last_error(cmi_group_handle g);
int cmi_group_size(cmi_group_handle g);
int cmi_group_set_hparams(cmi_group_handle g, double regU, double regI, double regB, double regC, double global_mean);
/* the WHOLE training matrix, as for cmi_set_ratings; the library cuts it by user */
int cmi_group_set_ratings(cmi_group_handle g, int64_t n, const int32_t *u, const int32_t *j, const int32_t *ctx, const double *r,
                          int32_t n_ctx, const int32_t *ctx_ptr, const int32_t *ctx_conds);
/* whole containers in the reference's shapes (count = rows * cols over ALL users / items): user-side ones are scattered to /
 * gathered from the owning shards, item-side ones are replicated / read from shard 0 */
int cmi_group_set_state(cmi_group_handle g, int which, const void *src, int64_t count, int dtype);
int cmi_group_get_state(cmi_group_handle g, int which, void *dst, int64_t count, int dtype);
int cmi_group_train_epoch(cmi_group_handle g, double lrate, double *loss_out);
/* local learning rate of every shard = lrate x scale when the group has more than one shard (default 1).  The mean merge divides an
 * item row's move by the shard count, so at equal rate a sharded run needs more epochs for the same training RMSE (1.2x / 1.4x / 1.6x
 * at 2 / 4 / 8 shards); scale = sqrt(n_shards) recovers it to <= 1.2x -- what the Java / C++ hosts set */
int cmi_group_set_lr_scale(cmi_group_handle g, double scale);
int cmi_group_train(cmi_group_handle g, int num_iters, double init_lrate, double max_lrate, int bold_driver, double decay, int early_stop,
                    double *losses, double *lrates, int *iters_run, double *final_lrate);
int cmi_group_train_from(cmi_group_handle g, int first_iter, double prev_loss, int num_iters, double init_lrate, double max_lrate,
                         int bold_driver, double decay, int early_stop, double *losses, double *lrates, int *iters_run, double *final_lrate);
/* test tuples are routed to the shard that owns their user; the error sums are merged exactly */
int cmi_group_eval_ratings(cmi_group_handle g, int64_t n, const int32_t *u, const int32_t *j, const int32_t *ctx, const double *r,
                           double min_rate, double max_rate, double *out, int64_t *count);
int cmi_group_predict_batch(cmi_group_handle g, int64_t n, const int32_t *u, const int32_t *j, const int32_t *ctx, int bound, double lo,
                            double hi, double *out);
/* info[0..1] = [first, last) user of the shard, info[2] = its tuples, info[3] = its device, info[4] = exchange in use (0 none: one
 * shard, 1 RCCL, 2 in-process), info[5] = elements of the exchanged bucket */
int cmi_group_shard_info(cmi_group_handle g, int shard, int64_t info[6]);
/* measurement (no reference counterpart; the reference's fold threads are timed by Recommender.execute()'s wall clock,
 * Recommender.java:284-297): HIP-event times of the most recent cmi_group_train_epoch, one float per shard -- compute_ms = the local
 * epoch's launches, exchange_ms = pack .. apply on the shard's stream (the collectives or the in-process sums, including the wait for
 * the slowest shard; 0 for a group of one) */
int cmi_group_last_times(cmi_group_handle g, float *compute_ms, float *exchange_ms);
/* Which exchange the group runs and why, as text (valid after cmi_group_set_ratings): RCCL -- after a pre-flight that ran one small
 * exchange of integer values through RCCL and through the in-process path and found both bit-identical to the host's sums -- or the
 * in-process exchange (peer copies): because shards share a device, or as the FALLBACK when ncclCommInitAll or the pre-flight failed
 * on this node (the reason is in the text and on stderr; training works either way).  No reference counterpart (CARSKit.java:395-412
 * has threads, not devices). */
const char *cmi_group_exchange_path(cmi_group_handle g);
/* the shard's instance (owned by the group), e.g. for cmi_schedule_info / cmi_last_epoch_ms */
int cmi_group_member(cmi_group_handle g, int shard, cmi_handle *out);
/* `--early-stop MAE|RMSE` for a sharded recommender (IterativeRecommender.java:149-161: isConverged() scores the test set after every
 * epoch): the test tuples are routed ONCE to the shard that owns their user and stay on its device (cmi_set_eval_ratings per shard);
 * cmi_group_eval_resident adds the shards' sums in shard order -> out = {MAE, RMSE, NMAE, rMAE, rRMSE} as cmi_eval_resident */
int cmi_group_set_eval_ratings(cmi_group_handle g, int64_t n, const int32_t *u, const int32_t *j, const int32_t *ctx, const double *r);
int cmi_group_eval_resident(cmi_group_handle g, double min_rate, double max_rate, double out[5], int64_t *count);

/* ---- the same exchange for a one-process-per-GPU job (carskit_amd/dist.py, bench.py --gpus N under torch.distributed.run) ------------
 * ONE implementation serves both hosts: cmi_group_* (one process, ncclCommInitAll) and cmi_comm_* (ncclCommInitRank) issue the same
 * three collectives from the same function (group_api.cpp, exchange_collective).  The host ranks share CMI_COMM_ID_BYTES bytes once
 * (rank 0 calls cmi_comm_unique_id, the host's own rendezvous hands the bytes to the other ranks), every rank calls cmi_comm_init
 * on its handle (after cmi_set_ratings / cmi_set_state: it snapshots the item-side containers), then per epoch
 *   cmi_comm_train_epoch(h, lrate, scale, &loss) = local epoch -> pack -> reduce-scatter + all-gather -> apply(scale) -> loss all-reduce
 * with scale = 1/world (the mean of the ranks' moves); `loss` is the GLOBAL loss, the epoch's one host
 * synchronisation.  cmi_comm_exchange alone is the exchange without the epoch (everything enqueued on cmi_stream()). */
#define CMI_COMM_ID_BYTES 128
int cmi_comm_unique_id(void *id /* CMI_COMM_ID_BYTES */);
int cmi_comm_init(cmi_handle h, const void *id, int rank, int world);
int cmi_comm_exchange(cmi_handle h, double scale);
int cmi_comm_train_epoch(cmi_handle h, double lrate, double scale, double *global_loss);
/* HIP-event time of the most recent cmi_comm_exchange on the handle's stream (pack .. loss all-reduce, including the wait for the
 * slowest rank); cmi_last_epoch_ms is the local epoch beside it */
int cmi_comm_last_exchange_ms(cmi_handle h, float *ms);

/* ---- FM: src/carskit/alg/cars/adaptation/dependent/FM.java (ALS / coordinate-descent sweep, not SGD) ---------
 * Separate handle type: the state is (w0, w[p], V[p x k]) with p = numUsers+numItems+numConditions
 * (FM.java:57-74) plus the per-rating errors[] and Q[][] of buildModel() (FM.java:117-146).  fp64 on the
 * device (the reference's precision).  The reference's quirks are kept: the context feature of a rating is
 * index numUsers+numItems+c with c the CONTEXT-COMBINATION id and value 1/numContextDims, present only if
 * c < numConditions (FM.java:81-86); denominators add the regulariser once per rating (FM.java:181,201); the
 * error/Q update of a factor uses x_il (FM.java:209-210).  errors[] and Q[][] are not stored: an error is
 * err0 + the running delta sums of its three coordinates (fm_kernels.hip), and a coordinate's sums are added per
 * slice of its support (not the Java's sequential order): model within ~1e-8 relative of the reference
 * arithmetic, RMSE within 1e-9.  `loss` (FM.java:218) is never
 * read by the reference and is not computed. */
typedef struct cmi_fm_instance *cmi_fm_handle;

/* new FM(train, test, fold) + initModel() allocation (FM.java:49-74).  Default (flags 0): every coordinate's sums are added in an order
 * the data layout alone decides (LDS parking + a fixed walk) -- two runs on identical inputs give bit-identical models, as two runs of
 * the reference's sweep do (FM.java:148-218), and the split phases (reduce / apply) equal the fused sweep bit for bit.
 * CMI_FM_FLAG_RELAXED_SUMS (or env CMI_FM_RELAXED_SUMS=1): the records' products are added with LDS atomics as they are evaluated --
 * ~11 % less time per sweep, same sums to the last few bits, but the order of the fp64 additions (so the last bits of the model, ~1e-12
 * relative) varies from run to run.  Both forms are within the 1e-8 the FM path promises against the reference arithmetic.
 * CMI_FM_FLAG_DETERMINISTIC: the round-5 name of what is now the default; accepted, no effect. */
#define CMI_FM_FLAG_DETERMINISTIC 0x1u
#define CMI_FM_FLAG_RELAXED_SUMS 0x2u
int cmi_fm_create(int k, int n_users, int n_items, int n_conds, int n_ctx_dims, int device, unsigned flags,
                  cmi_fm_handle *out);
int cmi_fm_destroy(cmi_fm_handle h);
const char *cmi_fm_last_error(cmi_fm_handle h);
/* -lw / -lf of the `FM=` line (FM.java:53-54; Java floats promoted) and `size` = trainMatrix.size() over ALL
 * ranks (FM.java:64; <= 0 means the local tuple count) */
int cmi_fm_set_hparams(cmi_fm_handle h, double regLw, double regLf, int64_t global_size);
/* training tuples as `trainMatrix.iterator()` yields them (FM.java:118-127); ctx = context-combination id */
int cmi_fm_set_ratings(cmi_fm_handle h, int64_t n, const int32_t *u, const int32_t *j, const int32_t *ctx,
                       const double *r);
/* w0, w (p), V (p x k row-major): injected initial model / trained model (FM.java:65-70) */
int cmi_fm_set_model(cmi_fm_handle h, double w0, const double *w, const double *V);
int cmi_fm_get_model(cmi_fm_handle h, double *w0, double *w, double *V);
/* the pre-pass of buildModel(): errors[] and Q[][] from the current model (FM.java:117-146) */
int cmi_fm_init(cmi_fm_handle h);
/* one iteration of the `for (iter ...)` loop (FM.java:148-218) on one GPU */
int cmi_fm_sweep(cmi_fm_handle h);
/* whole buildModel(): cmi_fm_init + num_iters sweeps (the reference has no early stop for FM) */
int cmi_fm_train(cmi_fm_handle h, int num_iters);
/* FM.predict (FM.java:93-113) (+ bounding, Recommender.java:306-317).  The reference multiplies EVERY entry of w and V by the
 * feature vector, its zeros included (FM.java:97-98, 103-105): while w or V holds an entry that is an infinity or a NaN, every
 * prediction whose tuple does not hold that entry's coordinate is NaN (an entry of V: every prediction) -- here and in
 * cmi_fm_eval_rankings.  (How such entries spread through cmi_fm_init and the sweeps is not modelled.) */
int cmi_fm_predict_batch(cmi_fm_handle h, int64_t n, const int32_t *u, const int32_t *j, const int32_t *ctx,
                         int bound, double lo, double hi, double *out);
int cmi_fm_synchronize(cmi_fm_handle h);
/* the HIP stream (hipStream_t) all of this handle's work is enqueued on (a multi-GPU host orders its collectives on it) */
int cmi_fm_stream(cmi_fm_handle h, void **stream);
/* Recommender.evalRankings (Recommender.java:668-964) with FM.predict (FM.java:93-113) as the scorer: arguments, outputs
 * and semantics exactly as cmi_eval_rankings above */
int cmi_fm_eval_rankings(cmi_fm_handle h, int64_t n_train, const int32_t *tu, const int32_t *tj, const int32_t *tctx,
                         const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx,
                         const double *sr, double bin_thold, int num_recs, int num_ignore, int strategy, double out[21],
                         int64_t *n_queries, int32_t *q_user, int32_t *q_ctx, int32_t *q_count, int32_t *top_items,
                         double *top_scores);
/* multi-GPU plumbing (no reference counterpart): a sweep is cmi_fm_num_phases() phases (0: w0; 1-3: w of the
 * user / item / context-feature field; 4+3f+field: column f of V).  phase_reduce leaves the local partial sums
 * [num(count/2) | den(count/2)] in a device buffer the host may all-reduce (ratings sharded across ranks),
 * phase_apply consumes it.  reduce+apply over all phases == cmi_fm_sweep. */
int cmi_fm_num_phases(cmi_fm_handle h);
int cmi_fm_phase_reduce(cmi_fm_handle h, int phase);
int cmi_fm_phase_buffer(cmi_fm_handle h, int phase, void **dev_ptr, int64_t *count);
int cmi_fm_phase_apply(cmi_fm_handle h, int phase);
/* reduce + apply of one phase fused (no exchange point), for phases whose coordinates are local to the rank */
int cmi_fm_phase_run(cmi_fm_handle h, int phase);
/* measurement (no reference counterpart): the layout cmi_fm_set_ratings built -- out[0..1] slices of the user / item order,
 * [2..4] records of the three orders, [5..6] chunks, [7] HBM bytes one factor has to move, [8..9] of that the reduce launch of
 * the user / item field, [10] slice entries, [11] p -- and the HIP-event duration of one phase's reduce kernel (it writes only
 * scratch, the model is untouched) */
/* ratings sharded by user over one process per GPU: the sweep with its per-phase exchange (all-reduce of [num | den] for the w0 /
 * item / context phases; user phases are rank-local) issued by the library on the instance's stream.  `id`: CMI_COMM_ID_BYTES bytes of
 * cmi_comm_unique_id() from rank 0; cmi_fm_set_hparams' global_size = the ratings of ALL ranks. */
int cmi_fm_comm_init(cmi_fm_handle h, const void *id, int rank, int world);
int cmi_fm_comm_sweep(cmi_fm_handle h);
int cmi_fm_layout(cmi_fm_handle h, int64_t out[12]);
int cmi_fm_time_reduce(cmi_fm_handle h, int phase, int reps, double *avg_ms);

/* ---- data side of the path (host-only, no GPU): DataDAO id-mapper and the compact->binary rewrite -------------
 * Integer / string work that must be BIT-EXACT with the reference (north_star: "integer id mapping bit-exact"). */
typedef struct cmi_dao *cmi_dao_handle;

/* DataDAO.readData (src/carskit/data/processor/DataDAO.java:166-354) for a binary-format rating file:
 * header tokens >= 3 are conditions (`dim:cond`), data lines `user,item,rating,0/1...`; inner ids are assigned
 * in first-seen order (users, items, "u,i" pairs, context keys = active condition indices joined by ','),
 * duplicates of a (pair, context) cell: last line wins; rating scale = sorted distinct values. */
int cmi_dao_read(const char *path, cmi_dao_handle *out);
/* `test-set` evaluation: the test DAO is built over the TRAINING DAO's id maps and extends them with unseen
 * users/items/contexts (src/carskit/main/CARSKit.java:335-340, DataDAO.java:119-143).  The result's counts and raw-id
 * tables are those of the union (what rateDao.numUsers() etc. return afterwards); its matrix is the test matrix. */
int cmi_dao_read_shared(const char *path, cmi_dao_handle train, cmi_dao_handle *out);
int cmi_dao_destroy(cmi_dao_handle h);
/* h == NULL: the last failure on this thread of cmi_dao_read(_shared) or of a handle-less data function (cmi_java_hashmap_order,
 * cmi_transform*, cmi_validate_data_format) */
const char *cmi_dao_last_error(cmi_dao_handle h);
/* out: numUsers, numItems, numUserItems, numContexts, numConditions, numContextDims, numRatings (lines), matrix entries */
int cmi_dao_counts(cmi_dao_handle h, int64_t out[8]);
/* the (user-item x context) rating matrix in MatrixIterator (CRS) order */
int cmi_dao_matrix(cmi_dao_handle h, int32_t *ui, int32_t *ctx, double *r);
/* getUserIdFromUI / getItemIdFromUI (DataDAO.java:1038-1046) as arrays over pair ids */
int cmi_dao_ui_maps(cmi_dao_handle h, int32_t *ui_user, int32_t *ui_item);
/* getContextConditionsList as CSR (ctx_ptr has numContexts+1 entries; cmi_dao_ctx_nnz gives len(ctx_conds)) */
int64_t cmi_dao_ctx_nnz(cmi_dao_handle h);
int cmi_dao_ctx_table(cmi_dao_handle h, int32_t *ctx_ptr, int32_t *ctx_conds);
/* condDimensionMap (numConditions entries) and EmptyContextConditions (conditions whose token ends with ":na") */
int cmi_dao_cond_info(cmi_dao_handle h, int32_t *cond_dim, int32_t *empty_conds, int32_t *n_empty);
int cmi_dao_rating_scale(cmi_dao_handle h, double *out, int32_t cap, int32_t *n);
/* raw key of an inner id; kind: 0 user, 1 item, 2 condition, 3 context key, 4 dimension, 5 "u,i" pair key */
const char *cmi_dao_raw_id(cmi_dao_handle h, int kind, int32_t idx);

/* Iteration order of a default java.util.HashMap<String,?> (JDK 8+) after inserting n DISTINCT keys in the given
 * order: positions[i] = index of the i-th key `for (k : map.keySet())` visits.  *treeified = 1 if a put made a bin of
 * 9 nodes in a table of 64 slots or more at the time of the put (order then not guaranteed).  Used by the transformer below. */
int cmi_java_hashmap_order(int64_t n, const char *const *keys, int64_t *positions, int *treeified);
/* DataTransformer.TransformationFromCompactToBinary + PublishNewRatingFiles + getHeader
 * (src/carskit/data/processor/DataTransformer.java:231-259,266-329,155-163): rewrites a compact-format file
 * (user,item,rating,dim1,dim2,...) as the binary-format train.csv, rows in the reference's HashMap order. */
int cmi_transform_compact_to_binary(const char *in_path, const char *out_path, int *treeified);
/* CARSKit.validateDataFormat (src/carskit/main/CARSKit.java:179-215): 1 binary, 2 loose, 3 compact; 0 where the reference throws
 * (no data line, a one-column header, a data line shorter than the header, a value Integer.valueOf refuses under a dim:cond column) */
int cmi_validate_data_format(const char *path);
/* DataTransformer.run() (DataTransformer.java:331-396) for binary / loose / compact input.  test_in == NULL: only the
 * training file (binary is copied).  With a test file, both are rewritten against the merged, SORTED condition set
 * of getConditions() (DataTransformer.java:57-92). */
int cmi_transform(const char *train_in, const char *train_out, const char *test_in, const char *test_out, int *treeified);

/* ---- host-only integer preprocessing (runs without a GPU) ------------------------------------- */

/* The dependency-level schedule the default mode executes (carskit_amd/csrc/level_schedule.cpp):
 * level(t) = 1 + max(level of the previous tuple with the same user, ... same item).  It replaces the
 * reference's implicit "one tuple after another" order (librec MatrixIterator, CAMF_CI.java:80) by the
 * weakest order that yields the identical result.  perm[n]: schedule position -> CRS tuple index;
 * level_off[0..*n_levels]: offsets of the levels in perm (level_cap = capacity of level_off, must be
 * >= *n_levels + 1; pass level_off = NULL to only count).  order: 0 keep CRS order inside a level,
 * 1 sort by item id, 2 sort by user id (tuples of one level commute, so this is free). */
int cmi_level_schedule(int64_t n, const int32_t *u, const int32_t *j, int32_t n_users, int32_t n_items, int order,
                       int32_t *perm, int64_t *level_off, int64_t level_cap, int64_t *n_levels);

/* The hub-chain form of the level schedule (level_schedule.cpp, build_chain_schedule; the default execution order).  hub: 1 chain
 * along items, 0 along users, -1 pick the one with fewer units, -2 / -3 users / items unless that costs more than 1.3x the units of the
 * other side (what cmi_set_ratings uses for CAMF_CU / CAMF_CI: the side with the context-bias rows) (*hub_used reports the choice).  perm[n]: stream position -> CRS tuple;
 * unit_off[*n_units+1]: offsets of the units in perm; level_off[*n_levels+1]: offsets of the levels in unit_off (unit indices).
 * Pass perm = NULL to only count (*n_units, *n_levels). */
int cmi_chain_schedule(int64_t n, const int32_t *u, const int32_t *j, int32_t n_users, int32_t n_items, int hub, int max_chain,
                       int32_t *perm, int32_t *unit_off, int64_t unit_cap, int64_t *level_off, int64_t level_cap,
                       int64_t *n_units, int64_t *n_levels, int *hub_used);
/* the same schedule built on `device` (sched_device.hip: a lane per hub row walks the row's CRS chain, the spoke rows hand over through
 * atomic words; sorts and scans around it) -- what cmi_set_ratings uses from 2 M tuples on; element for element the host's result, the
 * order of librec's MatrixIterator restated, not changed.  CMI_E_UNSUPPORTED: not built (the caller uses cmi_chain_schedule). */
int cmi_chain_schedule_device(int device, int64_t n, const int32_t *u, const int32_t *j, int32_t n_users, int32_t n_items, int hub, int max_chain,
                              int32_t *perm, int32_t *unit_off, int64_t unit_cap, int64_t *level_off, int64_t level_cap,
                              int64_t *n_units, int64_t *n_levels, int *hub_used);

/* host-only views of two schedule post-passes (tests).  cmi_narrow_runs: run_len[l] > 0 = a run of that many consecutive
 * levels with <= max_tuples tuples each starts at level l and is walked by ONE launch (the library uses 256 / 16), -1 = inside
 * a run, 0 = own launch; *n_launches = launches per epoch.  cmi_conflict_free_blocks: CAMF_C's CRS blocks -- maximal runs of
 * consecutive tuples sharing no user and no item, cut at max_block (the library uses 64); off may be NULL to query *n_blocks. */
int cmi_narrow_runs(int64_t n_levels, const int64_t *level_off, int64_t max_tuples, int64_t min_levels, int32_t *run_len,
                    int64_t *n_launches);
int cmi_conflict_free_blocks(int64_t n, const int32_t *u, const int32_t *j, int32_t n_users, int32_t n_items, int32_t max_block,
                             int32_t *off, int64_t off_cap, int64_t *n_blocks);
/* host-only: the most rated items of a user whose Y rows the default SVD++ epoch (svdpp_team.hip) keeps in LDS at k factors, fp64
 * state or fp32, from the kernel's LDS use (0: k outside 1 .. 1024) -- a user with more is walked by one wave through memory;
 * *lds_bytes (may be NULL): the dynamic LDS of that launch */
int cmi_svdpp_team_rows(int k, int f64, int64_t *lds_bytes);

/* The owner form behind CMI_FLAG_SCHED_OWNER (level_schedule.cpp, build_owner_schedule): like the level schedules it replaces the
 * reference's implicit "one tuple after another" order (librec MatrixIterator in `for (MatrixEntry me : trainMatrix)`,
 * CAMF_CI.java:80) by an explicit order-exact one -- every row of the heavy side is walked by one owner in CRS order, the other side's
 * rows wait for their update count.  hub: 1 items are owned, 0 users, -1 the side
 * with the larger maximum degree (*hub_used reports it).  perm[n]: list position -> CRS tuple (an owner's tuples contiguous, in CRS
 * order); own_off[n_owners+1]; want[n]: updates of the tuple's spoke row that precede it; flags[n]: bit 0 hub row taken over in
 * registers from the previous list entry, bit 1 hub row re-read late (written < depth+1 entries back), bit 2 hub row stored, bit 3
 * spoke row taken over in registers, bit 4 spoke record stored. */
int cmi_owner_schedule(int64_t n, const int32_t *u, const int32_t *j, int32_t n_users, int32_t n_items, int hub, int n_owners, int depth,
                       int32_t *perm, int64_t *own_off, uint32_t *want, uint32_t *flags, int *hub_used);

/* ---- ItemKNN / UserKNN (src/carskit/alg/baseline/cf/{ItemKNN,UserKNN}.java; knn_api.cpp, knn_kernels.hip) -------------------
 * Rating prediction and top-N scores of the two memory-based baselines over the 2-D train matrix (DataDAO.toTraditionalSparseMatrix: a (user, item)
 * cell holds the mean of its ratings over contexts).  cmi_knn_build computes Recommender.buildCorrs on the device -- every pair
 * (a < b) of non-empty rows (UserKNN) or columns (ItemKNN), the reference's correlation() with its sums run sequentially in fp64 in
 * ascending order of the contracted index -- into a dense n x n fp64 matrix; NaN marks an unset entry (the diagonal, pairs with an
 * empty side, NaN similarities).  cmi_knn_predict_batch is the model's predict(u, j): candidates with sim > 0 and a rating, the knn cut
 * by (similarity descending, java.util.HashMap position), the weighted sum in the final HashMap iteration order; bit-exact to the
 * reference.  A tuple whose HashMap would treeify a bin (9 keys in one bucket of a table of 64 slots or more; its iteration order is
 * not modelled) fails the call with CMI_E_UNSUPPORTED.  No CPU fallback: without a device cmi_knn_create returns CMI_E_NO_DEVICE. */
#define CMI_KNN_USER 0
#define CMI_KNN_ITEM 1
#define CMI_SIM_PCC 0
#define CMI_SIM_COS 1
#define CMI_SIM_COS_BINARY 2
#define CMI_SIM_MSD 3
#define CMI_SIM_CPC 4
#define CMI_SIM_EXJACCARD 5
typedef struct cmi_knn_instance *cmi_knn_handle;
/* the measure of a `similarity` value: case-insensitive, and any unknown name is CMI_SIM_PCC (Recommender.correlation's default:) */
int cmi_knn_measure(const char *name);
int cmi_knn_create(int kind, int n_users, int n_items, int device, unsigned flags, cmi_knn_handle *out);
int cmi_knn_destroy(cmi_knn_handle h);
const char *cmi_knn_last_error(cmi_knn_handle h);
/* the 2-D train matrix as n cells; a duplicate (u, i) or an id out of range -> CMI_E_INVALID */
int cmi_knn_set_ratings(cmi_knn_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r);
/* shrinkage: num.shrinkage (applied when > 0); min_rate / max_rate give cpc's median.  The n x n matrix must fit in free device
 * memory, else CMI_E_INVALID with the bytes needed (nothing is built) */
int cmi_knn_build(cmi_knn_handle h, int measure, int shrinkage, double min_rate, double max_rate);
/* rows [row0, row0 + nrows) of the similarity matrix, dense, NaN where unset */
int cmi_knn_get_similarity(cmi_knn_handle h, int32_t row0, int32_t nrows, double *dst);
/* predict(u, j) of n tuples; knn <= 0: every candidate; bound: clamp to [lo, hi] as Recommender.predict(u, j, c, true).  A tuple's
 * candidate list (ItemKNN: the user's items, UserKNN: the item's users) may hold at most CMI_KNN_MAX_CANDIDATES entries: the wave that
 * predicts it ranks the candidates by counting, O(m^2 / 64) steps per lane (2 000 tuples at the limit: 21 ms, tools/bench_knn.py);
 * a longer list -> CMI_E_UNSUPPORTED, naming the tuple, before anything runs */
#define CMI_KNN_MAX_CANDIDATES 16384
int cmi_knn_predict_batch(cmi_knn_handle h, int64_t n, const int32_t *u, const int32_t *j, int knn, double global_mean, int bound,
                          double lo, double hi, double *out);
int cmi_knn_last_build_ms(cmi_knn_handle h, float *ms);
/* Top-N (item.ranking=on).  Recommender.ranking(u, j, c) = predict(u, j, c, false) (Recommender.java:1016-1018): unbounded and
 * context-free.  With isRankingPred set, ItemKNN.predict (ItemKNN.java:92-95) and UserKNN.predict (UserKNN.java:94-97) keep a neighbour
 * on `rate > 0` alone, so negative similarities enter the map, the knn cut and the weighted sum.  The neighbours are the indices of
 * corrs.row(target), and librec's SymmMatrix.row() leaves out the entries equal to zero (+0.0 and -0.0), so over the device matrix
 * (NaN = unset) a neighbour is kept iff sim == sim && sim != 0.0 && rate > 0.  Everything after the filter is
 * cmi_knn_predict_batch's: one device function with the keep rule as its parameter.
 * cmi_knn_ranking_batch: ranking(u, j) of n tuples; the candidate limit as in cmi_knn_predict_batch; a tuple that would treeify a bin
 * -> CMI_E_UNSUPPORTED, the message naming one such (user, item) */
int cmi_knn_ranking_batch(cmi_knn_handle h, int64_t n, const int32_t *u, const int32_t *j, int knn, double global_mean, double *out);
/* Recommender.evalRankings (Recommender.java:668-964) with that ranking(u, j) as the scorer, knn and global_mean as above: arguments,
 * outputs and semantics exactly as cmi_slim_eval_rankings below.  The scores of a user are computed once and serve all of the user's
 * contexts.  Before cmi_knn_build -> CMI_E_INVALID.  An owner list of the evaluation (ItemKNN: a query user's items, UserKNN: a
 * candidate item's users) longer than CMI_KNN_MAX_CANDIDATES -> CMI_E_UNSUPPORTED before anything runs; a (user, item) that would
 * treeify a bin -> CMI_E_UNSUPPORTED, the message naming one.  The driver (carskit-mi355x) still refuses item.ranking=on for itemknn,
 * userknn, slopeone and nmf: this entry point and its Python binding are the public surface */
int cmi_knn_eval_rankings(cmi_knn_handle h, int knn, double global_mean, int64_t n_train, const int32_t *tu, const int32_t *tj,
                          const int32_t *tctx, const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx,
                          const double *sr, double bin_thold, int num_recs, int num_ignore, int strategy, double out[21],
                          int64_t *n_queries, int32_t *q_user, int32_t *q_ctx, int32_t *q_count, int32_t *top_items, double *top_scores);
/* device time by events of the scoring and selection of the last cmi_knn_eval_rankings; before one -> CMI_E_INVALID */
int cmi_knn_last_rank_ms(cmi_knn_handle h, float *ms);

/* ---- SlopeOne (src/carskit/alg/baseline/cf/SlopeOne.java; slopeone_api.cpp, slopeone_kernels.hip) ----------------------------
 * Rating prediction of the third memory-based baseline over the same 2-D train matrix as ItemKNN.  cmi_slope_build computes
 * SlopeOne.buildModel on the device into two dense n_items x n_items matrices: dev[i][j] is the sum over the users who rated both
 * items, in ascending user order from +0.0 in fp64, of r_ui - r_uj, divided by their count card[i][j] (fp64 and int32: 12 bytes a
 * cell); cells without a common user, the diagonal included, are 0.0 / 0.  cmi_slope_predict_batch is the model's predict(u, j):
 * over the user's items i != j with card[j][i] > 0, in ascending item order, preds += (dev[j][i] + r_ui) * card[j][i] and
 * cards += card[j][i]; preds / cards, or global_mean when nothing was added.  Bit-exact to the reference.  No CPU fallback: without
 * a device cmi_slope_create returns CMI_E_NO_DEVICE. */
typedef struct cmi_slope_instance *cmi_slope_handle;
int cmi_slope_create(int n_users, int n_items, int device, unsigned flags, cmi_slope_handle *out);
int cmi_slope_destroy(cmi_slope_handle h);
const char *cmi_slope_last_error(cmi_slope_handle h);
/* the 2-D train matrix as n cells; a duplicate (u, i) or an id out of range -> CMI_E_INVALID; n >= 2^31 -> CMI_E_UNSUPPORTED */
int cmi_slope_set_ratings(cmi_slope_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r);
/* The two n x n matrices must fit in free device memory, else CMI_E_INVALID with the bytes needed (nothing is built) */
int cmi_slope_build(cmi_slope_handle h);
/* rows [row0, row0 + nrows) of the deviation and the cardinality matrix, dense; either destination may be NULL */
int cmi_slope_get_deviation(cmi_slope_handle h, int32_t row0, int32_t nrows, double *dev, int32_t *card);
/* predict(u, j) of n tuples; bound: clamp to [lo, hi] as Recommender.predict(u, j, c, true).  A user's list may be any length */
int cmi_slope_predict_batch(cmi_slope_handle h, int64_t n, const int32_t *u, const int32_t *j, double global_mean, int bound,
                            double lo, double hi, double *out);
int cmi_slope_last_build_ms(cmi_slope_handle h, float *ms);
/* Recommender.evalRankings (Recommender.java:668-964) with ranking(u, j, c) = predict(u, j, c, false) (Recommender.java:1016-1018) as
 * the scorer: SlopeOne.predict has no ranking branch, so the score is cmi_slope_predict_batch's without the bound.  Arguments, outputs
 * and semantics exactly as cmi_slim_eval_rankings below; the scores of a user are computed once and serve all of the user's contexts.
 * Before cmi_slope_build -> CMI_E_INVALID.  The driver still refuses item.ranking=on for slopeone (see cmi_knn_eval_rankings) */
int cmi_slope_eval_rankings(cmi_slope_handle h, double global_mean, int64_t n_train, const int32_t *tu, const int32_t *tj,
                            const int32_t *tctx, const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj,
                            const int32_t *sctx, const double *sr, double bin_thold, int num_recs, int num_ignore, int strategy,
                            double out[21], int64_t *n_queries, int32_t *q_user, int32_t *q_ctx, int32_t *q_count, int32_t *top_items,
                            double *top_scores);
/* device time by events of the scoring and selection of the last cmi_slope_eval_rankings; before one -> CMI_E_INVALID */
int cmi_slope_last_rank_ms(cmi_slope_handle h, float *ms);

/* ---- NMF (src/carskit/alg/baseline/cf/NMF.java; nmf_api.cpp, nmf_kernels.hip) --------------------------------------------------
 * Lee & Seung's multiplicative updates over the 2-D train matrix V, fp64, bit-exact to the reference: every sum (product(W, u, H, j)
 * over the factors, DenseVector.inner over a row's or a column's entries in ascending index order) is one left-to-right chain from
 * 0.0 without FMA.  State: W (n_users x k) and H (k x n_items, kept item-major on the device), 1 <= k <= 256.  A cell whose value is
 * 0 takes no part (librec's SparseMatrix.row() / column() leave it out).  No CPU fallback: without a device cmi_nmf_create returns
 * CMI_E_NO_DEVICE. */
typedef struct cmi_nmf_instance *cmi_nmf_handle;
/* NMF.java:47-53,58-59 (numFactors, the shapes of W and H) */
int cmi_nmf_create(int k, int n_users, int n_items, int device, unsigned flags, cmi_nmf_handle *out);
int cmi_nmf_destroy(cmi_nmf_handle h);
const char *cmi_nmf_last_error(cmi_nmf_handle h);
/* NMF.java:64 (V = train): the 2-D train matrix as n cells; a duplicate (u, i) or an id out of range -> CMI_E_INVALID; n >= 2^31 ->
 * CMI_E_UNSUPPORTED */
int cmi_nmf_set_ratings(cmi_nmf_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r);
/* NMF.java:58-62: W (n_users x k, row-major) and H (k x n_items, row-major, the reference's layout).  Either may be NULL (left as it
 * is) once both have been set */
int cmi_nmf_set_model(cmi_nmf_handle h, const double *W, const double *H);
int cmi_nmf_get_model(cmi_nmf_handle h, double *W, double *H);
/* NMF.java:71-126, one pass of buildModel's loop: W[u][f] *= real / (estm + 1e-9) for every user with entries, then the same for H's
 * columns with the new W, then *loss = 0.5 * the sum of (predict(u, j) - r)^2 over the cells with r > 0.  W and H are bit-identical
 * to the reference's; the loss is summed in a fixed order that depends on the number of cells alone (block partials, then one chain),
 * not the reference's single chain: the same bits from run to run, and within (cells) * 2^-53, relatively, of the reference's.
 * NaN/Inf loss -> CMI_E_NUMERIC with *loss set */
int cmi_nmf_iterate(cmi_nmf_handle h, double *loss);
/* NMF.java:142-145, predict(u, j) = product(W, u, H, j) of n tuples; bound: clamp to [lo, hi] as Recommender.predict(u, j, c, true) */
int cmi_nmf_predict_batch(cmi_nmf_handle h, int64_t n, const int32_t *u, const int32_t *j, int bound, double lo, double hi, double *out);
/* device time of the last cmi_nmf_iterate, by events: ms[0] the W phase (NMF.java:72-89), ms[1] the H phase (:92-110), ms[2] the loss
 * (:113-126) */
int cmi_nmf_last_iter_ms(cmi_nmf_handle h, float ms[3]);
/* Top-N evaluation of NMF.  (The two names stand outside the cmi_nmf_ prefix: that prefix is the closed set of the training and
 * rating-prediction ABI above.)
 * Recommender.evalRankings (Recommender.java:668-964) with ranking(u, j, c) = predict(u, j, c, false) (Recommender.java:1016-1018) =
 * product(W, u, H, j) (NMF.java:142-145) as the scorer.  Arguments, outputs and semantics exactly as cmi_slim_eval_rankings below; the
 * scores of a user are computed once and serve all of the user's contexts.  Before cmi_nmf_set_model -> CMI_E_INVALID.  The scoring
 * kernel keeps the user's row of W in LDS and takes k <= 128: a model of 129 <= k <= 256 -> CMI_E_UNSUPPORTED.  The driver still refuses
 * item.ranking=on for nmf (see cmi_knn_eval_rankings) */
int cmi_topn_nmf_eval_rankings(cmi_nmf_handle h, int64_t n_train, const int32_t *tu, const int32_t *tj, const int32_t *tctx, const double *tr,
                          int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx, const double *sr, double bin_thold,
                          int num_recs, int num_ignore, int strategy, double out[21], int64_t *n_queries, int32_t *q_user, int32_t *q_ctx,
                          int32_t *q_count, int32_t *top_items, double *top_scores);
/* device time by events of the scoring and selection of the last cmi_topn_nmf_eval_rankings; before one -> CMI_E_INVALID */
int cmi_topn_nmf_last_rank_ms(cmi_nmf_handle h, float *ms);

/* ---- SLIM (src/carskit/alg/baseline/ranking/SLIM.java; slim_api.cpp, slim_kernels.hip) -----------------------------------------
 * Ning & Karypis' sparse linear method for top-N over the 2-D train matrix, fp64, bit-exact to the reference: coordinate descent over
 * the listed cells of the item x item matrix W, column by column, every sum one left-to-right chain from 0.0 without FMA, in the
 * iteration order of the reference's hash collections.  A cell whose value is 0 takes no part.  State: per item j its neighbour list
 * nns(j), in the order SLIM.java walks it, and one weight per list entry, W[i][j].  The caller draws W.init() (SLIM.java:81-82) and
 * hands over the listed cells.  No CPU fallback: without a device cmi_slim_create returns CMI_E_NO_DEVICE. */
typedef struct cmi_slim_instance *cmi_slim_handle;
/* SLIM.java:65-75,81 (W is numItems x numItems) */
int cmi_slim_create(int n_users, int n_items, int device, unsigned flags, cmi_slim_handle *out);
int cmi_slim_destroy(cmi_slim_handle h);
const char *cmi_slim_last_error(cmi_slim_handle h);
/* Recommender.java:1076-1081 (train) and SLIM.java:84 (userCache): the 2-D train matrix as n cells; a duplicate (u, i) or an id out of
 * range -> CMI_E_INVALID; n >= 2^31 -> CMI_E_UNSUPPORTED */
int cmi_slim_set_ratings(cmi_slim_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r);
/* SLIM.java:86-117.  knn > 0: buildCorrs(false) on the device (the kernel of cmi_knn_build; measure, shrinkage, min_rate, max_rate as
 * there), then per item on the host the row's non-zero similarities into a java.util.HashMap in ascending order, the cut to the knn
 * largest (Lists.sortMap's stable descending sort over the map's order, clear(), re-put) and the HashMultimap's value set (a HashSet of
 * 4 slots that doubles at load 0.75); the list is that set's iteration order.  knn <= 0: every list is train.columns(), the items with
 * an entry, ascending, the item itself included.  Device memory is reserved before anything runs: the n x n similarity matrix (knn > 0)
 * and 20 bytes a list entry; what does not fit -> CMI_E_INVALID with the bytes needed (nothing is built).  A list whose map or set
 * would treeify a bin -> CMI_E_UNSUPPORTED.  The weights start at 0.0 */
int cmi_slim_build_neighbors(cmi_slim_handle h, int knn, int measure, int shrinkage, double min_rate, double max_rate);
/* host-only: SLIM.java:96-109 for ONE item, as cmi_slim_build_neighbors runs it per row of the similarity matrix: sims[n] is the item's
 * row (NaN: unset; 0.0 is not a neighbour), knn >= 1; out (room for n entries) receives the list in its iteration order, *n_out its
 * length.  A list whose map or set would treeify a bin -> CMI_E_UNSUPPORTED (cmi_last_error(NULL) has the message) */
int cmi_slim_cut_neighbors(int32_t n, const double *sims, int knn, int32_t *out, int32_t *n_out);
/* the lists: ptr[n_items + 1] and idx[ptr[n_items]]; with idx == NULL only ptr is written (call it so first to size idx) */
int cmi_slim_get_neighbors(cmi_slim_handle h, int64_t *ptr, int32_t *idx);
/* SLIM.java:81-82,93,116: the weights, aligned with idx: w[p] = W[idx[p]][j] for ptr[j] <= p < ptr[j + 1] */
int cmi_slim_set_weights(cmi_slim_handle h, const double *w);
int cmi_slim_get_weights(cmi_slim_handle h, double *w);
/* SLIM.java:127-176, one pass of buildModel's loop: for j ascending and i in nns(j), the coordinate update of W[i][j] from the means of
 * r_ui * e_uj, r_ui^2 and e_uj^2 over column i's users, e_uj = r_uj - predict(u, j, true, i).  l1 and l2 are the DOUBLE values of the
 * reference's float options (-l1 0.1 is (double)0.1f).  *loss is the reference's, bit for bit: one chain over the coordinates.
 * NaN/Inf loss -> CMI_E_NUMERIC with *loss set */
int cmi_slim_iterate(cmi_slim_handle h, double l1, double l2, double *loss);
/* SLIM.java:183-209, predict(u, j) = predict(u, j, true, j) of n tuples: unbounded, context-free */
int cmi_slim_predict_batch(cmi_slim_handle h, int64_t n, const int32_t *u, const int32_t *j, double *out);
/* Recommender.evalRankings (Recommender.java:668-964) with SLIM.predict (SLIM.java:206-209) as the scorer: arguments, outputs and
 * semantics exactly as cmi_eval_rankings above.  The scores of a user are computed once and serve all of the user's contexts */
int cmi_slim_eval_rankings(cmi_slim_handle h, int64_t n_train, const int32_t *tu, const int32_t *tj, const int32_t *tctx,
                           const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx,
                           const double *sr, double bin_thold, int num_recs, int num_ignore, int strategy, double out[21],
                           int64_t *n_queries, int32_t *q_user, int32_t *q_ctx, int32_t *q_count, int32_t *top_items,
                           double *top_scores);
/* device time of the last cmi_slim_build_neighbors' similarity build (SLIM.java:88), by events */
int cmi_slim_last_build_ms(cmi_slim_handle h, float *ms);
/* device time of the last cmi_slim_iterate, by events: ms[0] the sweep (SLIM.java:130-176), ms[1] the loss chain (:160) */
int cmi_slim_last_iter_ms(cmi_slim_handle h, float ms[2]);

/* ---- RankALS (src/carskit/alg/baseline/ranking/RankALS.java; rankals_api.cpp, rankals_kernels.hip) ---------------------------------
 * Takacs & Tikk's alternating least squares for personalised ranking over the 2-D train matrix, fp64, bit-exact to the reference: per
 * iteration one k x k solve per user of train.rows() and one per item, every sum one left-to-right chain from 0.0 without FMA, the
 * solve librec's DenseMatrix.inv() (Gauss-Jordan, first-strictly-greater pivot, the identity as it stands when a column has no pivot)
 * followed by mult().  A cell whose value is 0 takes no part.  The four sums of the Q step that do not read the item are formed once
 * per iteration, in the reference's order, instead of once per item.  No CPU fallback: without a device cmi_rankals_create returns
 * CMI_E_NO_DEVICE. */
typedef struct cmi_rankals_instance *cmi_rankals_handle;
/* RankALS.java:47-79, IterativeRecommender.java:235-236 (numFactors, the shapes of P and Q).  The solve keeps `mat` and `I` in LDS,
 * 16 k^2 bytes: k > 64 -> CMI_E_UNSUPPORTED */
int cmi_rankals_create(int k, int n_users, int n_items, int device, unsigned flags, cmi_rankals_handle *out);
int cmi_rankals_destroy(cmi_rankals_handle h);
const char *cmi_rankals_last_error(cmi_rankals_handle h);
/* Recommender.java:1076-1081 (train) and RankALS.java:73-79 (s_i = train.columnSize(i) or 1, sum_s): the 2-D train matrix as n cells;
 * a duplicate (u, i) or an id out of range -> CMI_E_INVALID; n >= 2^31 -> CMI_E_UNSUPPORTED */
int cmi_rankals_set_ratings(cmi_rankals_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r);
/* IterativeRecommender.java:235-241: P (n_users x k) and Q (n_items x k), row-major, drawn by the caller.  Either may be NULL (left as
 * it is) after the first call */
int cmi_rankals_set_model(cmi_rankals_handle h, const double *P, const double *Q);
int cmi_rankals_get_model(cmi_rankals_handle h, double *P, double *Q);
/* RankALS.java:84-205, one pass of buildModel's loop: sum_sq and sum_sqq (:91-98), P[u] = M.inv().mult(y) for every user of rows()
 * (:100-137), the per-user m_* values (:140-166), Q[i] = M.inv().mult(y) for every item (:168-204).  support_weight: -sw
 * (RankALS.java:71,76) */
int cmi_rankals_iterate(cmi_rankals_handle h, int support_weight);
/* IterativeRecommender.java:126-128, predict(u, j) = DenseMatrix.rowMult(P, u, Q, j) of n tuples: unbounded, context-free */
int cmi_rankals_predict_batch(cmi_rankals_handle h, int64_t n, const int32_t *u, const int32_t *j, double *out);
/* Recommender.evalRankings (Recommender.java:668-964) with that predict as the scorer: arguments, outputs and semantics exactly as
 * cmi_slim_eval_rankings above.  The scores of a user are computed once and serve all of the user's contexts */
int cmi_rankals_eval_rankings(cmi_rankals_handle h, int64_t n_train, const int32_t *tu, const int32_t *tj, const int32_t *tctx,
                              const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx,
                              const double *sr, double bin_thold, int num_recs, int num_ignore, int strategy, double out[21],
                              int64_t *n_queries, int32_t *q_user, int32_t *q_ctx, int32_t *q_count, int32_t *top_items,
                              double *top_scores);
/* device time by events: of the last cmi_rankals_iterate ms[0] the item moments (RankALS.java:91-98), ms[1] the user solves (:100-166),
 * ms[2] the item-independent sums of the Q step (:184-189), ms[3] the item solves (:168-204), 0 before an iteration; ms[4] the scoring
 * and selection of the last cmi_rankals_eval_rankings, 0 before one.  Before both an iteration and an evaluation -> CMI_E_INVALID */
int cmi_rankals_last_iter_ms(cmi_rankals_handle h, float ms[5]);
/* librec DenseMatrix.inv() of n_mats n x n row-major matrices, A -> out, by the device routine both solves use: the pivot paths can be
 * tested directly.  n > 64 -> CMI_E_UNSUPPORTED */
int cmi_rankals_invert(cmi_rankals_handle h, int n_mats, int n, const double *A, double *out);

/* ---- BPR (src/carskit/alg/baseline/ranking/BPR.java; bpr_api.cpp, bpr_kernels.hip, java_math.hpp) -------------------------------------
 * Bayesian personalised ranking on the 2-D train matrix, fp64, bit-exact against the reference with Math.exp / Math.log defined as
 * StrictMath's (fdlibm).  Every iteration draws n_users * 100 triples (u, i, j) from one java.util.Random stream -- on the device by
 * speculation at every stream position and list ranking, or by the sequential host walk, which defines the sampler and takes over
 * whenever the device form's reservation, draw cap or memory does not suffice -- and applies them in the reference's order by
 * levels of row-disjoint samples.  1 <= k <= 128.  No CPU fallback: without a device cmi_bpr_create returns CMI_E_NO_DEVICE. */
typedef struct cmi_bpr_instance *cmi_bpr_handle;
#define CMI_BPR_FLAG_STRICT 0x1u       /* the loss as one chain in (sample, term) order: the reference's sum bit for bit (small data) */
#define CMI_BPR_FLAG_HOST_SAMPLER 0x2u /* every iteration's triples by the host walk */
#define CMI_BPR_FLAG_MIN_SLACK 0x4u    /* reserve 3 draws a sample and no more: three redraws or more in an iteration send it to the host walk (tests) */
int cmi_bpr_create(int k, int n_users, int n_items, int device, unsigned flags, cmi_bpr_handle *out);
int cmi_bpr_destroy(cmi_bpr_handle h);
const char *cmi_bpr_last_error(cmi_bpr_handle h);
/* the 2-D train matrix as n cells (zero-valued cells take no part, as in train.row(u)); a duplicate (u, i) or an id out of range ->
 * CMI_E_INVALID; a user whose row holds every item (the reference would draw j for ever), or no user with a cell -> CMI_E_INVALID */
int cmi_bpr_set_ratings(cmi_bpr_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r);
int cmi_bpr_set_model(cmi_bpr_handle h, const double *P, const double *Q);
int cmi_bpr_get_model(cmi_bpr_handle h, double *P, double *Q);
/* the 48-bit state of the java.util.Random stream the sampler draws from (a seed's state is (seed ^ 0x5DEECE66D) & (2^48 - 1)): the
 * driver's fold splitter and BPR share one stream */
int cmi_bpr_set_random_state(cmi_bpr_handle h, int64_t state);
int cmi_bpr_get_random_state(cmi_bpr_handle h, int64_t *state);
/* one iteration's n_users * 100 triples from the handle's stream state, which stays as it is; on_device: the device form (falling
 * back as cmi_bpr_iterate does), else the host walk.  *state_after: the state after the last consumed draw */
int cmi_bpr_sample(cmi_bpr_handle h, int on_device, int32_t *u, int32_t *i, int32_t *j, int64_t *state_after);
/* BPR.java:59-103: one iteration (sample, level build, epoch, loss); the stream state moves on.  NaN/Inf loss -> CMI_E_NUMERIC with
 * *loss set */
int cmi_bpr_iterate(cmi_bpr_handle h, double lrate, double regU, double regI, double *loss);
int cmi_bpr_predict_batch(cmi_bpr_handle h, int64_t n, const int32_t *u, const int32_t *j, double *out);
/* arguments, outputs and semantics exactly as cmi_slim_eval_rankings above */
int cmi_bpr_eval_rankings(cmi_bpr_handle h, int64_t n_train, const int32_t *tu, const int32_t *tj, const int32_t *tctx,
                          const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx, const double *sr,
                          double bin_thold, int num_recs, int num_ignore, int strategy, double out[21], int64_t *n_queries,
                          int32_t *q_user, int32_t *q_ctx, int32_t *q_count, int32_t *top_items, double *top_scores);
/* of the last cmi_bpr_iterate: ms[0] the sampler, ms[1] the level build (host), ms[2] the epoch, ms[3] the loss (0 before an
 * iteration); ms[4] the last cmi_bpr_eval_rankings.  Before both -> CMI_E_INVALID */
int cmi_bpr_last_iter_ms(cmi_bpr_handle h, float ms[5]);
/* of the last cmi_bpr_iterate: out[0] levels, out[1] levels launched alone, out[2] runs of narrow levels, out[3] the widest level;
 * out[4] the iterations and samplings so far that asked for the device form and were sampled by the host walk (the list left the
 * reservation, met an overflow, or the reservation could not be allocated); a handle created with CMI_BPR_FLAG_HOST_SAMPLER never
 * counts: its device form is switched off, nothing falls back */
int cmi_bpr_last_schedule(cmi_bpr_handle h, int64_t out[5]);
/* without a device or a handle: the level schedule of n triples (order: n sample ids sorted by level; level_of: n levels, 1-based);
 * *n_levels, *max_chain (the most samples on one row) */
int cmi_bpr_levels(int n_users, int n_items, int64_t n, const int32_t *u, const int32_t *i, const int32_t *j, int32_t *order,
                   int32_t *level_of, int32_t *n_levels, int64_t *max_chain);
/* without a device or a handle: the host walk over n_samples samples of the n cells' matrix from *state, which moves on */
int cmi_bpr_sample_host(int n_users, int n_items, int64_t n, const int32_t *u, const int32_t *i, const double *r, int64_t *state,
                        int64_t n_samples, int32_t *ou, int32_t *oi, int32_t *oj);
/* stream positions per ranking block of the device sampler */
int cmi_bpr_rank_block(void);
/* probes of java_math.hpp: n values of java.util.Random.nextInt(bound) from *state, which moves on; StrictMath.exp and log of n
 * arguments.  on_device: by the device's functions (nextInt at every position by jump-ahead, the list walked on the host) */
int cmi_java_next_ints(int64_t *state, int32_t bound, int64_t n, int32_t *out, int on_device);
int cmi_java_exp_log(int64_t n, const double *x, double *exp_out, double *log_out, int on_device);

/* ---- LRMF (src/carskit/alg/baseline/ranking/LRMF.java; lrmf_api.cpp, lrmf_host.hpp, lrmf_kernels.hip) -------------------------------
 * List-wise matrix factorisation on the 2-D train matrix, fp64, bit-exact against the reference with Math.exp / Math.log defined as
 * StrictMath's (fdlibm).  An iteration visits every stored cell (u, j, r) in the matrix iterator's order -- stored zeros included -- and
 * recomputes uexp = sum_i exp(P[u] . Q[i]) over getColumns(u) -- stored zeros excluded -- for each.  A unit is one user's cells; one
 * workgroup runs a unit with P[u] and the user's item rows in LDS (or, past cmi_lrmf_lds_rows(k) cells, the rows in memory), and the
 * units run by levels that share no row.  1 <= k <= 128.  No CPU fallback: without a device cmi_lrmf_create returns CMI_E_NO_DEVICE. */
typedef struct cmi_lrmf_instance *cmi_lrmf_handle;
#define CMI_LRMF_FLAG_STRICT 0x1u      /* the loss as one chain in (cell, term) order: the reference's sum bit for bit (small data) */
#define CMI_LRMF_FLAG_GLOBAL_ROWS 0x2u /* every unit leaves its item rows in memory (the form of a unit too large for LDS) */
/* LRMF.java:46-53.  k > 128 -> CMI_E_UNSUPPORTED */
int cmi_lrmf_create(int k, int n_users, int n_items, int device, unsigned flags, cmi_lrmf_handle *out);
int cmi_lrmf_destroy(cmi_lrmf_handle h);
const char *cmi_lrmf_last_error(cmi_lrmf_handle h);
/* the 2-D train matrix as n cells, zero-valued cells among them; a duplicate (u, i) or an id out of range -> CMI_E_INVALID.
 * LRMF.java:55-67 (userExp) and the model-independent part of :70-110: A = Math.exp(r) / userExp[u] per cell by the host's fdlibm exp,
 * the unit schedule.  A user whose only cells are stored zeros is accepted: its uexp is 0.0 and the iteration reports CMI_E_NUMERIC */
int cmi_lrmf_set_ratings(cmi_lrmf_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r);
/* IterativeRecommender.java:239-245 (initByNorm = false): the caller draws P (n_users x k) and Q (n_items x k); NULL keeps one */
int cmi_lrmf_set_model(cmi_lrmf_handle h, const double *P, const double *Q);
int cmi_lrmf_get_model(cmi_lrmf_handle h, double *P, double *Q);
/* LRMF.java:74-104: one iteration (the epoch, then the loss).  NaN/Inf loss -> CMI_E_NUMERIC with *loss set */
int cmi_lrmf_iterate(cmi_lrmf_handle h, double lrate, double regU, double regI, double *loss);
/* IterativeRecommender.predict(u, j) = DenseMatrix.rowMult(P, u, Q, j) */
int cmi_lrmf_predict_batch(cmi_lrmf_handle h, int64_t n, const int32_t *u, const int32_t *j, double *out);
/* Recommender.java:630-860; arguments, outputs and semantics exactly as cmi_slim_eval_rankings above */
int cmi_lrmf_eval_rankings(cmi_lrmf_handle h, int64_t n_train, const int32_t *tu, const int32_t *tj, const int32_t *tctx,
                           const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx, const double *sr,
                           double bin_thold, int num_recs, int num_ignore, int strategy, double out[21], int64_t *n_queries,
                           int32_t *q_user, int32_t *q_ctx, int32_t *q_count, int32_t *top_items, double *top_scores);
/* device time by events: ms[0] the epoch and ms[1] the loss of the last cmi_lrmf_iterate (0 before an iteration); ms[2] the last
 * cmi_lrmf_eval_rankings.  Before both -> CMI_E_INVALID */
int cmi_lrmf_last_iter_ms(cmi_lrmf_handle h, float ms[3]);
/* of the matrix set: out[0] levels, out[1] levels launched alone (several units, a workgroup each), out[2] runs of consecutive
 * single-unit levels (one workgroup each), out[3] the widest level, out[4] the units that run in the global form */
int cmi_lrmf_last_schedule(cmi_lrmf_handle h, int64_t out[5]);
/* without a device or a handle: the unit schedule of n cells (order: the users that store a cell sorted by level, at most n_users
 * of them; level_of: n_users levels, 1-based, 0 for a user without a cell); *n_levels, *max_chain (the most users on one column) */
int cmi_lrmf_levels(int n_users, int n_items, int64_t n, const int32_t *u, const int32_t *i, int32_t *order, int32_t *level_of,
                    int32_t *n_levels, int64_t *max_chain);
/* the most cells of a unit that keeps its item rows in LDS at k factors, from the kernel's LDS use (0: k out of range); the threads
 * of its workgroup (the item lanes of one pass of a cell's sum) */
int cmi_lrmf_lds_rows(int k);
int cmi_lrmf_block(void);

/* ---- RankSGD (src/carskit/alg/baseline/ranking/RankSGD.java; ranksgd_api.cpp, ranksgd_host.hpp, ranksgd_kernels.hip) ----------------
 * Pairwise ranking SGD on the 2-D train matrix, fp64, bit-exact against the reference.  An iteration visits every non-zero cell (u, i,
 * rui) in row order, draws an item j from the popularity list (RankSGD.java:66-75, :94-112) until !Ru.contains(j), and applies
 * e = (pui - puj) - rui to P[u], Q[i], Q[j] (:113-132).  The tries of the draw are computed at every stream position on the device;
 * the walk that assigns them to cells is sequential and stays on the host; the updates run in the reference's order by levels of
 * row-disjoint samples.  1 <= k <= 128.  No CPU fallback: without a device cmi_ranksgd_create returns CMI_E_NO_DEVICE.
 *
 * numRates: Recommender.java:141 declares the field that RankSGD.java:71 divides by, and no file of the reference assigns it.  So by
 * default the divisor is 0, as there: every item with a cell has probability +Infinity, the list is in java.util.HashMap iteration
 * order and EVERY draw returns its first item; a matrix in which some user's row contains() that item is refused, because the
 * reference would not end.  CMI_RANKSGD_FLAG_NUM_RATES_SIZE divides by the number of non-zero cells instead (LibRec's numRates =
 * trainMatrix.size(), what the algorithm's description means): a popularity-weighted draw. */
typedef struct cmi_ranksgd_instance *cmi_ranksgd_handle;
#define CMI_RANKSGD_FLAG_STRICT 0x1u         /* the loss as one chain in cell order: the reference's sum bit for bit (small data) */
#define CMI_RANKSGD_FLAG_HOST_SAMPLER 0x2u   /* every try by the host */
#define CMI_RANKSGD_FLAG_NUM_RATES_SIZE 0x4u /* RankSGD.java:71 divides by the number of non-zero cells, not by the unassigned field */
/* RankSGD.java:53-59.  k > 128 -> CMI_E_UNSUPPORTED */
int cmi_ranksgd_create(int k, int n_users, int n_items, int device, unsigned flags, cmi_ranksgd_handle *out);
int cmi_ranksgd_destroy(cmi_ranksgd_handle h);
const char *cmi_ranksgd_last_error(cmi_ranksgd_handle h);
/* the 2-D train matrix as n cells (zero-valued cells take no part: not in columnSize(), rows() or row(u)) and RankSGD.java:62-76, the
 * item list.  A duplicate (u, i), an id out of range, no non-zero cell, or a user whose row contains() every item a draw can return
 * (the reference would draw for ever) -> CMI_E_INVALID; items that would treeify the HashMap, or more than 2^31-1 expected tries ->
 * CMI_E_UNSUPPORTED */
int cmi_ranksgd_set_ratings(cmi_ranksgd_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r);
/* IterativeRecommender.java:235-241 (initByNorm = true): the caller draws P (n_users x k) and Q (n_items x k); NULL keeps one */
int cmi_ranksgd_set_model(cmi_ranksgd_handle h, const double *P, const double *Q);
int cmi_ranksgd_get_model(cmi_ranksgd_handle h, double *P, double *Q);
/* the 48-bit state of the java.util.Random stream that Randoms.random() draws from (RankSGD.java:97), as cmi_bpr_set_random_state */
int cmi_ranksgd_set_random_state(cmi_ranksgd_handle h, int64_t state);
int cmi_ranksgd_get_random_state(cmi_ranksgd_handle h, int64_t *state);
/* RankSGD.java:85-112 of one iteration from the handle's stream state, which stays as it is: (u, i, j, rui) per non-zero cell in cell
 * order (arrays of as many entries as non-zero cells were set).  on_device: the first max_device_tries tries (0: the handle's
 * reservation) by the device, the rest by the host; else all by the host.  *state_after: the state after the last consumed draw */
int cmi_ranksgd_sample(cmi_ranksgd_handle h, int on_device, int64_t max_device_tries, int32_t *u, int32_t *i, int32_t *j, double *r,
                       int64_t *state_after);
/* RankSGD.java:80-137: one iteration (tries, walk, level build, epoch, loss); the stream state moves on.  NaN/Inf loss, or no list
 * entry reaching the random number on a cell's first try (:116 would predict(u, -1)) -> CMI_E_NUMERIC */
int cmi_ranksgd_iterate(cmi_ranksgd_handle h, double lrate, double *loss);
/* IterativeRecommender.predict(u, j) = DenseMatrix.rowMult(P, u, Q, j) */
int cmi_ranksgd_predict_batch(cmi_ranksgd_handle h, int64_t n, const int32_t *u, const int32_t *j, double *out);
/* Recommender.java:630-860; arguments, outputs and semantics exactly as cmi_slim_eval_rankings above */
int cmi_ranksgd_eval_rankings(cmi_ranksgd_handle h, int64_t n_train, const int32_t *tu, const int32_t *tj, const int32_t *tctx,
                              const double *tr, int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx,
                              const double *sr, double bin_thold, int num_recs, int num_ignore, int strategy, double out[21],
                              int64_t *n_queries, int32_t *q_user, int32_t *q_ctx, int32_t *q_count, int32_t *top_items,
                              double *top_scores);
/* of the last cmi_ranksgd_iterate: ms[0] the device tries and their copy (:97-107), ms[1] the host walk (:85-112), ms[2] the level
 * build (host), ms[3] the epoch (:113-132), ms[4] the loss (0 before an iteration); ms[5] the last cmi_ranksgd_eval_rankings.  Before
 * both -> CMI_E_INVALID */
int cmi_ranksgd_last_iter_ms(cmi_ranksgd_handle h, float ms[6]);
/* of the last cmi_ranksgd_iterate: out[0] levels, out[1] levels launched alone, out[2] runs of narrow levels, out[3] the widest level;
 * out[4] the tries so far that the walk needed past the device's and the host supplied (a handle created with
 * CMI_RANKSGD_FLAG_HOST_SAMPLER never counts) */
int cmi_ranksgd_last_schedule(cmi_ranksgd_handle h, int64_t out[5]);
/* without a device or a handle.  RankSGD.java:66-75 of the n cells' matrix: the list's keys and the running sums of :102 along it
 * (n_items entries of room), *n_out entries.  flags: CMI_RANKSGD_FLAG_NUM_RATES_SIZE or 0 */
int cmi_ranksgd_item_table(int n_users, int n_items, int64_t n, const int32_t *u, const int32_t *i, const double *r, unsigned flags,
                           int32_t *item_out, double *cum_out, int32_t *n_out);
/* RankSGD.java:97-107: out[t], t < n <= 2^24: the item of the try that starts 2t draws after `state` over the given list, or -1 when
 * no sum reaches the random number.  on_device: by the device's kernel (CMI_E_NO_DEVICE without one) */
int cmi_ranksgd_tries(int64_t state, int32_t n_table, const int32_t *item, const double *cum, int64_t n, int32_t *out, int on_device);
/* RankSGD.java:85-112 over the n cells' matrix with the tries given as an array: j per non-zero cell in cell order, *tries_used.
 * -1 on a cell's first try -> CMI_E_NUMERIC; the array used up -> CMI_E_UNSUPPORTED */
int cmi_ranksgd_assign_host(int n_users, int n_items, int64_t n, const int32_t *u, const int32_t *i, const double *r, int64_t n_tries,
                            const int32_t *try_item, int32_t *j_out, int64_t *tries_used);
/* cmi_ranksgd_sample by the host alone, with cmi_ranksgd_set_ratings' refusals: outputs of n entries of room, *n_cells of them set;
 * *state moves on */
int cmi_ranksgd_sample_host(int n_users, int n_items, int64_t n, const int32_t *u, const int32_t *i, const double *r, unsigned flags,
                            int64_t *state, int32_t *ou, int32_t *oi, int32_t *oj, double *orr, int64_t *n_cells, int64_t *tries_used);

/* ---- CPTF (src/carskit/alg/cars/adaptation/independent/CPTF.java on src/carskit/generic/TensorRecommender.java; cptf_api.cpp,
 * cptf_kernels.hip) ---------------------------------------------------------------------------------------------------------------
 * CP tensor factorisation, fp64: one factor matrix M[d] (dims[d] x k) per dimension of the rating tensor -- dimension 0 the user,
 * 1 the item, one more per context dimension -- and pred(keys) = sum_f prod_d M[d][keys[d]][f].  An iteration sweeps the train
 * entries in the tensor's iterator order; nearly every entry touches the same few context rows, so the sweep is one dependency chain
 * and runs as one wave that owns the factors (cptf_kernels.hip).  The caller supplies the entries' keys as the reference's tensor holds
 * them and, for ranking, the keys TensorRecommender.getKeys gives every context id: the two differ in the reference
 * (DataDAO.java:456-462 gives a condition that is already listed the LAST index of its dimension's list, getKeys uses indexOf).
 * 1 <= k <= 128, 2 <= n_dims <= 10.  No CPU fallback: without a device cmi_cptf_create returns CMI_E_NO_DEVICE. */
typedef struct cmi_cptf_instance *cmi_cptf_handle;
#define CMI_CPTF_FLAG_STRICT 0x1u     /* pred as the reference's chain over f, the loss as its chain over (entry, f, d): bit for bit; a slot
                                       * per loss term, at most CMI_CPTF_STRICT_MAX_TERMS of them (small data) */
#define CMI_CPTF_STRICT_MAX_TERMS (1LL << 27) /* 1 GiB of slots, summed by one thread */
#define CMI_CPTF_FLAG_GLOBAL_CTX 0x2u /* context rows travel through memory even where they would fit the LDS budget */
/* CPTF.java:46-55, TensorRecommender.java:62-84.  dims: n_dims sizes.  k > 128, n_dims < 2 or > 10 -> CMI_E_UNSUPPORTED */
int cmi_cptf_create(int k, int n_dims, const int32_t *dims, int device, unsigned flags, cmi_cptf_handle *out);
int cmi_cptf_destroy(cmi_cptf_handle h);
const char *cmi_cptf_last_error(cmi_cptf_handle h);
/* trainTensor as CPTF.java:81 iterates it: keys (n x n_dims, row-major) and the rates.  An entry with rate <= 0 takes no part
 * (:85-86).  A key outside its dimension -> CMI_E_INVALID; with CMI_CPTF_FLAG_STRICT more than CMI_CPTF_STRICT_MAX_TERMS loss terms
 * (entries x (1 + k x n_dims)) -> CMI_E_UNSUPPORTED */
int cmi_cptf_set_entries(cmi_cptf_handle h, int64_t n, const int32_t *keys, const double *r);
/* TensorRecommender.java:189-205: the keys of the dimensions 2 .. n_dims - 1 for every context id (n_ctx x (n_dims - 2)), what
 * CPTF.predict(u, j, c) and so evalRankings use.  A key outside its dimension -> CMI_E_INVALID */
int cmi_cptf_set_context_keys(cmi_cptf_handle h, int32_t n_ctx, const int32_t *ctx_keys);
/* minRate and maxRate, which CPTF.java:133-136 clamps the ranking score to (Recommender.java's rating scale) */
int cmi_cptf_set_rating_range(cmi_cptf_handle h, double min_rate, double max_rate);
/* CPTF.java:46-55: M[0] .. M[n_dims - 1] concatenated, each dims[d] x k row-major; the caller draws them */
int cmi_cptf_set_model(cmi_cptf_handle h, const double *M);
int cmi_cptf_get_model(cmi_cptf_handle h, double *M);
/* CPTF.java:80-111: one iteration; *loss as after :111.  NaN/Inf loss (:103 divides by an element without a guard) -> CMI_E_NUMERIC
 * with *loss set */
int cmi_cptf_iterate(cmi_cptf_handle h, double lrate, double reg, double *loss);
/* CPTF.java:141-155 of n key tuples (n x n_dims), the sum in the reference's order; bound: clamped to [lo, hi] as
 * TensorRecommender.java:86-164 bounds what it evaluates */
int cmi_cptf_predict_batch(cmi_cptf_handle h, int64_t n, const int32_t *keys, int bound, double lo, double hi, double *out);
/* Recommender.java:630-860 with ranking(u, j, c) = CPTF.predict(u, j, c) (CPTF.java:119-139: getKeys' keys, clamped); arguments,
 * outputs and semantics exactly as cmi_eval_rankings.  A context id with no keys set -> CMI_E_INVALID */
int cmi_cptf_eval_rankings(cmi_cptf_handle h, int64_t n_train, const int32_t *tu, const int32_t *tj, const int32_t *tctx, const double *tr,
                           int64_t n_test, const int32_t *su, const int32_t *sj, const int32_t *sctx, const double *sr, double bin_thold,
                           int num_recs, int num_ignore, int strategy, double out[21], int64_t *n_queries, int32_t *q_user, int32_t *q_ctx,
                           int32_t *q_count, int32_t *top_items, double *top_scores);
/* by events: ms[0] the epoch and ms[1] the loss sum of the last cmi_cptf_iterate (0 before one), ms[2] the last
 * cmi_cptf_eval_rankings.  Before both -> CMI_E_INVALID */
int cmi_cptf_last_iter_ms(cmi_cptf_handle h, float ms[3]);
/* 1: the last iteration kept the context rows in LDS; 0: in memory */
int cmi_cptf_ctx_in_lds(cmi_cptf_handle h);
/* without a device or a handle: DataDAO.toSparseTensor (DataDAO.java:423-481), the fold split of TensorRecommender's constructor
 * (TensorRecommender.java:62-84) and getKeys (:189-205).
 * In: rateMatrix as n_cells cells (pair, ctx, rate) in its iteration order (rows = user-item pairs, then columns = contexts); the
 * pairs' users and items; context c's conditions ctx_conds[ctx_ptr[c] .. ctx_ptr[c + 1]) in list order, one per dimension; cond_dim:
 * condition -> context dimension (0 .. D - 1); testMatrix as the pair of each of its n_test cells, in its order.
 * flags: 0 builds the keys as the reference does (DataDAO.java:461: a condition already listed gets its list's LAST index);
 * CMI_CPTF_FLAG_KEYS_INDEXOF gives the condition's own index.
 * Out: *n_dims = 2 + D and dims; dimension d's condition list dim_list[dim_list_ptr[d] .. dim_list_ptr[d + 1]) (D + 1 and n_conds
 * entries of room); the rate tensor's keys (n_cells x n_dims) and vals; the train and the test tensor of the fold in iterator order
 * (n_cells entries of room each; every context of a test pair moves to the test tensor, and contexts of a pair that share keys are
 * one test entry with the value set last); ctx_keys (n_ctx x D): getKeys' keys of every context.
 * dims[0] and dims[1] count the DISTINCT users and items, as the reference does, while the keys are the ids: an id not below that count
 * builds here as there and is refused by cmi_cptf_set_entries (the reference indexes its factor matrix out of range).
 * A context whose getKeys gives -1 (named with its dimension and condition) -> CMI_E_INVALID; no context dimension (librec's SparseTensor refuses fewer than 3
 * dimensions), more than 10 dimensions, a HashSet of positions with a tree bin -> CMI_E_UNSUPPORTED.  The message: cmi_cptf_last_error(NULL) */
#define CMI_CPTF_FLAG_KEYS_INDEXOF 0x4u
int cmi_cptf_tensor_build(int64_t n_cells, const int32_t *pair, const int32_t *ctx, const double *rate, int32_t n_pairs,
                          const int32_t *pair_user, const int32_t *pair_item, int32_t n_ctx, const int32_t *ctx_ptr, const int32_t *ctx_conds,
                          int32_t n_conds, const int32_t *cond_dim, int64_t n_test, const int32_t *test_pair, unsigned flags,
                          int32_t *n_dims, int32_t *dims, int32_t *dim_list_ptr, int32_t *dim_list, int32_t *keys, double *vals,
                          int64_t *n_train, int32_t *train_keys, double *train_vals, int64_t *n_test_out, int32_t *test_keys,
                          double *test_vals, int32_t *ctx_keys);

/* ---- BPMF (src/carskit/alg/baseline/cf/BPMF.java; bpmf_api.cpp, bpmf_kernels.hip, bpmf_host.hpp) -----------------------------------
 * Bayesian PMF by Gibbs sampling over the 2-D train matrix, fp64, bit for bit: per iteration the hyper-parameter step of both sides
 * (on the host: two k x k Wishart draws), then two Gibbs passes, each over every user and then every item -- a row's posterior is
 * a k x k solve (Gram matrix, DenseMatrix.inv(), DenseMatrix.cholesky(), k normal draws), a workgroup per row.
 * Two random streams: P and Q are drawn by the caller (DenseMatrix.init draws from librec.util.Randoms); the gaussian and gamma draws
 * of buildModel come from happy.coding.math.Randoms, whose state -- the 48-bit LCG state and the cached second value of
 * nextGaussian()'s last pair -- is the handle's stream.  1 <= k <= 64 (two k x k matrices of doubles in LDS).  No CPU fallback:
 * without a device cmi_bpmf_create returns CMI_E_NO_DEVICE. */
typedef struct cmi_bpmf_instance *cmi_bpmf_handle;
#define CMI_BPMF_FLAG_STRICT 0x1u /* the loss as one chain in cell order: the reference's sum bit for bit (small data); else a fixed tree */
/* BPMF.java:44-75 (numFactors, the shapes of P and Q).  k > 64 -> CMI_E_UNSUPPORTED */
int cmi_bpmf_create(int k, int n_users, int n_items, int device, unsigned flags, cmi_bpmf_handle *out);
int cmi_bpmf_destroy(cmi_bpmf_handle h);
const char *cmi_bpmf_last_error(cmi_bpmf_handle h);
/* `train` as n cells.  A stored 0.0 is no entry of train.row(u) / train.column(j) (BPMF.java:157-158, :196-197: a user whose only cell
 * is a stored zero has count == 0 and is skipped) but is a term of the loss (:233: the matrix iterator gives it).  Sets globalMean to
 * the mean of the non-zero cells, one chain in cell order */
int cmi_bpmf_set_ratings(cmi_bpmf_handle h, int64_t n, const int32_t *u, const int32_t *i, const double *r);
/* globalMean (Recommender.java:265: the mean of the CONTEXTUAL train matrix, which the caller holds), read by :168, :206 and predict */
int cmi_bpmf_set_global_mean(cmi_bpmf_handle h, double global_mean);
int cmi_bpmf_get_global_mean(cmi_bpmf_handle h, double *global_mean);
/* BPMF.java:71-75: P and Q, drawn by the caller with init(0, 1); and any later injection */
int cmi_bpmf_set_model(cmi_bpmf_handle h, const double *P, const double *Q);
int cmi_bpmf_get_model(cmi_bpmf_handle h, double *P, double *Q);
/* the stream of happy.coding.math.Randoms: state (0 .. 2^48 - 1; after Randoms.seed(s): (s ^ 0x5DEECE66D) & (2^48 - 1)), have_cached
 * and cached (java.util.Random's haveNextNextGaussian and nextNextGaussian) */
int cmi_bpmf_set_stream(cmi_bpmf_handle h, int64_t state, int have_cached, double cached);
int cmi_bpmf_get_stream(cmi_bpmf_handle h, int64_t *state, int *have_cached, double *cached);
/* BPMF.java:77-83: mu_u / mu_m = the column means, alpha_u / alpha_m = cov().inv(), of the model as it stands */
int cmi_bpmf_init_hyper(cmi_bpmf_handle h);
/* alpha_u (k x k), mu_u (k), alpha_m, mu_m as they stand; any may be null */
int cmi_bpmf_get_hyper(cmi_bpmf_handle h, double *alpha_u, double *mu_u, double *alpha_m, double *mu_m);
int cmi_bpmf_set_hyper(cmi_bpmf_handle h, const double *alpha_u, const double *mu_u, const double *alpha_m, const double *mu_m);
/* BPMF.java:97-242: one iteration -- both hyper steps, two Gibbs passes over the users and the items, the loss (*loss as after :242).
 * Before set_ratings, set_model or init_hyper -> CMI_E_INVALID.  NaN / Inf loss -> CMI_E_NUMERIC with *loss set */
int cmi_bpmf_iterate(cmi_bpmf_handle h, double *loss);
/* of the last cmi_bpmf_iterate: ms[0] the moments of P and Q (:99-100, :126-127; device, by events), ms[1] the hyper steps (:102-122,
 * :129-149; host, wall clock), ms[2] the two user passes and ms[3] the two item passes (gaussians, rows and the read-back of the null
 * flags; by events), ms[4] the loss */
int cmi_bpmf_last_iter_ms(cmi_bpmf_handle h, float ms[5]);
/* BPMF.java:325-327: globalMean + DenseMatrix.rowMult(P, u, Q, j) of n tuples; bound: clamped to [lo, hi] (Recommender.predict(u, j, c,
 * true)), which the rating evaluation takes */
int cmi_bpmf_predict_batch(cmi_bpmf_handle h, int64_t n, const int32_t *u, const int32_t *j, int bound, double lo, double hi, double *out);
/* one Gibbs pass of one side alone with the caller's hyper-parameters (side 0: BPMF.java:155-191, the users, writes P; side 1:
 * :194-229, the items, writes Q).  null_flags (n_users or n_items ints; may be null): 1 where the row has entries and
 * covar.cholesky() is null -- the row keeps its value and takes no draw.  *draws: the gaussians taken.  The handle's stream moves on */
int cmi_bpmf_sample_side(cmi_bpmf_handle h, int side, const double *alpha, const double *mu, int32_t *null_flags, int64_t *draws);
/* the parts alone.  The message of a failure: cmi_bpmf_last_error(NULL).
 * java.util.Random.nextGaussian() n times on the device from (*state, *have_cached, *cached), which are left as after the last one */
int cmi_java_next_gaussians(int64_t *state, int *have_cached, double *cached, int64_t n, double *out);
/* the attempts of the polar method the device makes at first for n_pairs accepted ones; where fewer are accepted it goes on */
int64_t cmi_bpmf_gauss_attempts(int64_t n_pairs);
/* DenseMatrix.columnMean(f) of every f and DenseMatrix.cov() of X (rows x k), on the device (on_device) or by the host loop */
int cmi_bpmf_moments(const double *X, int rows, int k, double *mean, double *cov, int on_device);
/* BPMF.java:102-122 (or :129-149) of one side with `rows` rows, on the host: x_bar = mean, S_bar = cov; alpha (k x k) and mu (k) in
 * place; the stream in place */
int cmi_bpmf_hyper_host(int k, int rows, const double *mean, const double *cov, double *alpha, double *mu, int64_t *state, int *have_cached,
                        double *cached);

#ifdef __cplusplus
}
#endif
#endif
