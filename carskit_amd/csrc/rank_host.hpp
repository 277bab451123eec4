// rank_host.hpp -- model-agnostic core of the ranking evaluation (Recommender.evalRankings,
// src/carskit/generic/Recommender.java:668-964): host bookkeeping (candidates, queries, exclusions), the device scoring driver, the
// metric formulas.  Shared by cmi_eval_rankings (the MF family: BiasedMF, PMF, CAMF_*, SVD++, CAMF_ICS / LCS / MCS),
// cmi_fm_eval_rankings (FM) and cmi_slim_eval_rankings (SLIM).  A new model calls rank_evaluate with a `score` that runs one of the
// three forms of the device loop: rank_run_device with its operand builders when its score is a contraction, rank_run_device_slab
// with a fill when it is not.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <functional>
#include <memory>
#include <string>
#include <utility>
#include <vector>

namespace cmi {

struct RankPlan {
    std::vector<int32_t> cand;            // candidate position -> item id (HashSet<Integer> order, minus ignored)
    std::vector<int32_t> qu, qc;          // query -> user, context
    std::vector<int32_t> gu, qg, gq0;     // query groups = runs of one user: group -> user; query -> group; group -> first query (+ end)
    std::vector<int32_t> truth_items;     // per query: its positive test items that are candidates (sorted)
    std::vector<int64_t> truth_ptr;
    std::vector<int32_t> excl_idx;        // per query: candidate positions rated by the user in that context (training)
    std::vector<int64_t> excl_ptr;
};

struct RankTuples {
    int64_t n;
    const int32_t *u, *j, *ctx;
    const double *r; // may be null for training tuples (all non-zero)
};

// ids must already be range-checked by the caller
void rank_build_plan(int n_users, int n_items, const RankTuples &train, const RankTuples &test, double bin_thold,
                     int num_ignore, RankPlan &plan);

// operand builders of a model: B[c] rows for candidates, A[q] rows + per-row constants for a batch of queries
template <typename T>
struct RankOperands {
    int k_logical; // un-padded operand length
    int hot0 = 0, hot1 = 0; // its one-hot columns [hot0, hot1), the last of the k_logical (RankHot, rank_kernels.hpp); hot1 <= hot0: none
    std::function<hipError_t(T *dB, const int32_t *dcand, int nc, int kp, hipStream_t)> build_items;
    std::function<hipError_t(T *dA, T *drc, const int32_t *dqu, const int32_t *dqc, int n, int kp, hipStream_t)> build_queries;
    // optional, in place of build_queries: also writes dscale[q], the factor the row's finished scores are multiplied by when it is an
    // infinity or a NaN (rank_launch_score: row_scale); 1 for every other row
    std::function<hipError_t(T *dA, T *drc, T *dscale, const int32_t *dqu, const int32_t *dqc, int n, int kp, hipStream_t)> build_scaled_queries;
    // optional: the candidates whose operand row holds an infinity or a NaN in the columns [0, mend_cols) are listed once per evaluation
    // (`listed`: [0] their number, then their positions), and mend computes the scores of a batch's n queries for them again, behind the
    // contraction and in front of the mask: for a model whose reference forms such a score from other terms than the contraction does
    int mend_cols = 0;
    std::function<hipError_t(T *dS, const int32_t *dqu, int n, const int32_t *dcand, int nc, const int32_t *listed, hipStream_t)> mend;
};

// A growable store of HIP events, made on first use and kept for the next evaluation.
struct RankEvents {
    explicit RankEvents(bool timing) : flags(timing ? hipEventDefault : hipEventDisableTiming) {}
    hipError_t grow(size_t n);                          // events 0 .. n - 1 exist
    hipEvent_t at(size_t i) const { return v[i]; }      // an event that grow / record has made
    hipError_t record(size_t i, hipStream_t stream);    // (grows to i + 1)
    void destroy();

  private:
    unsigned flags;
    std::vector<hipEvent_t> v;
};

// Device and pinned-host buffers of an evaluation, owned by the handle and reused (grow-only) by the next one: allocating and
// freeing ~1 GiB per call costs milliseconds and a device synchronisation each.
struct RankWorkspace {
    struct Buf {
        void *p = nullptr;
        size_t cap = 0;
        uint64_t plan_gen = 0; // the plan (RankWorkspace::plan_gen) whose array this buffer holds; 0: none
    };
    // Every buffer is an entry of `dev` / `pin`: release() frees the arrays, so a buffer declared here cannot leak.
    enum Dev {
        DA, DB, DS, DRC,                       // operand rows of a batch of queries / of the candidates, the score slab, the per-row constants
        DCAND, DQU, DQC, DEXPTR, DEXCL,        // the plan's cand, qu, qc, excl_ptr, excl_idx
        DTOP, DSCORE, DCOUNT,                  // the lists
        DQG, DGU,                              // the plan's qg, gu (split form; the slab form shares DGU)
        DGQ0,                                  // the plan's gq0 (slab form)
        DDC, DQD,                              // split form: the distinct contexts and every query's index into them (v_dctx, v_qd)
        DB2, DA2, DS2, DSCR,                   // split form: the S2 contraction's operands and slab; a zeroed per-row constant
        DCOLC,                                 // split form: itemBias of the candidates (the S1 contraction adds it at the end)
        DSB, DAB,                              // split form: the second slab / operand buffer (batch b + 1 is contracted while batch b is selected)
        DM1, DM1B, DM2,                        // split form: per-row maxima of S1 (per slab) / S2 over tiles of 64 candidates (the selection's tile pruning)
        DHOT,                                  // the candidates whose one-hot columns hold an infinity or a NaN (RankHot::count_list)
        DSCALE,                                // per query of a batch: the scale applied to its finished scores (RankOperands::build_scaled_queries)
        N_DEV
    };
    enum Pin { H_TOP, H_SCORE, H_COUNT, N_PIN }; // pinned host: the lists as they come back
    Buf dev[N_DEV], pin[N_PIN];
    template <typename T>
    T *d(Dev b) const { return (T *)dev[b].p; }
    template <typename T>
    T *h(Pin b) const { return (T *)pin[b].p; }
    hipError_t need(Dev b, size_t bytes); // (a re-allocation forgets the plan array the buffer held)
    hipError_t need(Pin b, size_t bytes);
    void release(); // the caller has made the owning device current

    hipStream_t sel_stream = nullptr;                   // split form: the selection's stream
    RankEvents ev01{true};                              // [0], [1]: around the device loop (timing)
    RankEvents evb{false};                              // one per batch: its lists have arrived on the host
    RankEvents evgemm{false}, evsel{false};             // split form, per batch: contraction done (main stream), selection done (selection stream)
    RankEvents evk{true};                               // split form, four per batch: around the contraction, around the selection
    RankPlan plan;                                      // the last evaluation's plan (capacity is reused)
    std::vector<int32_t> v_dctx, v_qd;                  // split form: context index arrays (capacity is reused)
    bool ctx_ready = false;                             // v_dctx / v_qd hold this evaluation's contexts (rank_split_usable)
    // Repeated evaluations of the same (train, test) tuples (`--early-stop` on a ranking measure evaluates after every epoch,
    // IterativeRecommender.java:149-161): the plan depends on the tuples alone, so it is kept, keyed by their sizes and a 64-bit
    // content hash, and so are the index arrays it put on the device.
    struct PlanKey {
        int64_t n_train = -1, n_test = -1, n_users = 0, n_items = 0;
        double bin_thold = 0;
        int num_ignore = 0;
        uint64_t hash = 0;
        bool operator==(const PlanKey &o) const {
            return n_train == o.n_train && n_test == o.n_test && n_users == o.n_users && n_items == o.n_items && bin_thold == o.bin_thold &&
                   num_ignore == o.num_ignore && hash == o.hash;
        }
    } plan_key;
    bool plan_valid = false; // `plan` belongs to plan_key
    // Residency is kept per buffer: rank_evaluate counts the plans it builds (plan_gen), a buffer remembers the plan whose array was
    // copied into it (Buf::plan_gen), and upload_plan copies only when the two differ.  A buffer holds one array of the plan whichever
    // form fills it, so one handle may alternate forms on the same plan (a topN above 64, or CMI_RANK_NO_SPLIT, takes the per-query
    // form): each form finds resident exactly the arrays that some earlier evaluation of this plan uploaded and uploads the rest.
    // `always`: copy, then tag, whatever the tag says (the per-query form: see rank_run_device).
    uint64_t plan_gen = 0;
    hipError_t upload_plan(Dev b, const void *host, size_t bytes, hipStream_t stream, bool always = false);
    void forget_uploads(); // after a HIP error: nothing is taken to be on the device
    struct HostVals { // per-query measures, uninitialised and grow-only (38 MB for 270 K queries: not re-faulted per call)
        std::unique_ptr<double[]> p;
        size_t cap = 0;
        double *need(size_t n) {
            if (n > cap) {
                p.reset(new double[n + n / 8]);
                cap = n + n / 8;
            }
            return p.get();
        }
    } vals, umeans; // umeans: per-user means of the ucu strategy (rank_fold_users)
    double kernel_ms[2] = {0, 0}; // last evaluation: contraction, selection (summed over the batches)
    // host wall clock of the last evaluation, ms: [0] plan, [1] setup (buffers, uploads, item operands), [2] scoring loop incl. the
    // overlapped per-batch measures, [3] tail (last batch's measures + the averages), [4] total
    double host_ms[5] = {0, 0, 0, 0, 0};
    // waits for the batches in order and hands each to on_batch while the device works on the later ones; fills host_ms[2], [3]
    hipError_t consume_batches(hipError_t e, const std::vector<std::pair<int64_t, int64_t>> &batches,
                               const std::function<void(int64_t, int64_t)> &on_batch, std::chrono::steady_clock::time_point t_loop);
};

// The three forms of the device loop.  All run on one skeleton (rank_run_batches in rank_api.cpp: batch size, list buffers, uploads of
// the plan's arrays, the lists' way back, timing) and supply only their scoring.
// on_batch(q0, q1): the lists of queries [q0, q1) have arrived in the pinned H_TOP / H_SCORE / H_COUNT (absolute query indexing);
// called on the host while the device scores the next batch
using RankBatchFn = std::function<void(int64_t, int64_t)>;

// The per-query form: one contraction row per query, from the model's operand builders.
template <typename T>
hipError_t rank_run_device(hipStream_t stream, RankWorkspace &ws, const RankPlan &plan, const RankOperands<T> &ops, double thold, int topn,
                           const RankBatchFn &on_batch, float *ms, double *flops);

// The split form for the MF family in fp32 (rank_kernels.hip): S1 per distinct query user, S2 per distinct context, added by the selection.
struct RankSplitArgs;
hipError_t rank_run_device_split(hipStream_t stream, RankWorkspace &ws, const RankPlan &plan, RankSplitArgs base, double thold, int topn,
                                 const RankBatchFn &on_batch, float *ms, double *flops);
// whether the split form applies: S2 must stay small (distinct contexts x candidates) and the lists must fit the register selection
bool rank_split_usable(const RankPlan &plan, int topn, RankWorkspace &ws);

// The slab form, for a model whose scores are no contraction (SLIM: slim_kernels.hip): fill(dS, dcand, nc, dgu, dgq0, g0, g1, q0, nq,
// stream) writes the fp64 scores of the queries [q0, q0 + nq), whose groups are g0 .. g1 (a group at a batch boundary comes in both
// batches), into dS[(q - q0) * nc + c]; the exclusions are masked and the lists selected as in rank_run_device.
using RankSlabFn = std::function<hipError_t(double *, const int32_t *, int, const int32_t *, const int32_t *, int, int, int64_t, int64_t, hipStream_t)>;
hipError_t rank_run_device_slab(hipStream_t stream, RankWorkspace &ws, const RankPlan &plan, const RankSlabFn &fill, double thold, int topn,
                                const RankBatchFn &on_batch, float *ms);

// the 18 measures of the lists of queries [q0, q1) -> vals[q * 18 + m] (threads over ranges of queries); optional per-query outputs
void rank_measures_range(const RankPlan &plan, int num_recs, const int32_t *top_idx, const double *top_score, const int32_t *top_count,
                         int64_t q0, int64_t q1, double *vals, int32_t *q_user, int32_t *q_ctx, int32_t *q_count, int32_t *top_items,
                         double *top_scores);
// averaged per strategy, in query order (Recommender.java:850-960).  ucu: rank_fold_users writes every user's mean over its contexts
// into `umeans` (18 doubles per user, user order) and may run batch by batch behind the device for the users a batch completes;
// rank_average folds what is left and sums over the users.
struct RankFolded {
    int64_t q = 0, u = 0; // first query not folded yet; users folded so far
    // the serial sum over users (ucu) / queries (uc), advanced batch by batch behind the device in the order rank_average would take
    int64_t summed = 0;   // users (ucu) or queries (uc) already in s / c
    double s[18] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int64_t c[18] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
};
// uc: add the queries [f.summed, q_to) to the running sums (query order)
void rank_sum_queries(const int32_t *top_count, const double *vals, RankFolded &f, int64_t q_to);
void rank_fold_users(const RankPlan &plan, const int32_t *top_count, const double *vals, double *umeans, RankFolded &f, int64_t q_to, bool last);
void rank_average(const RankPlan &plan, int strategy, const int32_t *top_count, const double *vals, double *umeans, RankFolded f,
                  double *out /*[21]*/);

// the arguments of cmi_eval_rankings / cmi_fm_eval_rankings (include/carskit_mi355x.h)
struct RankEvalIO {
    RankTuples train, test;
    double bin_thold;
    int num_recs, num_ignore, strategy;
    double *out;
    int64_t *n_queries;
    int32_t *q_user, *q_ctx, *q_count, *top_items;
    double *top_scores;
};
// Recommender.evalRankings around a model's scorer, shared by every model's eval_rankings entry point: the argument checks, the id
// checks (context ids below ctx_bound; INT64_MAX: any non-negative id), the plan (kept while the tuples are the same, by content hash),
// the measures and the users' means folded batch by batch behind the device, the averages.  `ready` checks the model's preconditions
// and makes its device current; `score` runs the device loop over the plan and hands every batch of lists to on_batch.  Messages go
// to `err`, prefixed "<what>: ".
int rank_evaluate(std::string &err, const char *what, RankWorkspace &ws, int n_users, int n_items, int64_t ctx_bound, const RankEvalIO &io,
                  const std::function<int()> &ready, const std::function<hipError_t(const RankPlan &, const RankBatchFn &)> &score);

} // namespace cmi
