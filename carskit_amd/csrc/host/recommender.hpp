// recommender.hpp -- C++ host layer above the C ABI, mirroring the reference's plugin interface for the accelerated
// path (same class names, hooks and lifecycle as src/carskit/generic/{Recommender,IterativeRecommender,
// ContextRecommender}.java and the model classes).  It uses ONLY include/carskit_mi355x.h -- it is what a JVM-less
// deployment links, and it shows the boundary is sufficient for a complete host -- and ../java_math.hpp, the header-only JDK
// arithmetic (fdlibm log, the java.util.Random LCG and its jump-ahead) that the library's host and device code share.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/carskit_mi355x.h"
#include "../java_math.hpp"
#include "configer.hpp"

namespace carskit {

// StrictMath.log = fdlibm __ieee754_log (java_math.hpp, shared with the device): glibc's log is correctly rounded and differs from
// fdlibm in the last ulp for some arguments, which would desynchronise nextGaussian().
using cmi::fdlibm_log;

// java.util.Random (published algorithm): fold assignment follows the reference's stream
// (happy.coding.math.Randoms.seed(n) -> new Random(n); uniform() -> nextDouble()).
class JavaRandom {
  public:
    explicit JavaRandom(int64_t seed) : seed_(((uint64_t)seed ^ 0x5DEECE66DULL) & ((1ULL << 48) - 1)) {}
    int32_t next(int bits) {
        seed_ = (seed_ * 0x5DEECE66DULL + 0xBULL) & ((1ULL << 48) - 1);
        return (int32_t)((int64_t)seed_ >> (48 - bits));
    }
    double nextDouble() { return (double)(((int64_t)next(26) << 27) + next(27)) * 0x1.0p-53; }
    int32_t nextInt(int32_t bound) { // bound > 0: java_math.hpp's one statement of the JDK algorithm, on this stream
        cmi::JavaStream s{seed_, 0};
        const int32_t r = s.nextInt(bound, INT64_MAX);
        seed_ = s.state;
        return r;
    }
    double nextGaussian() { // polar method with StrictMath.log / StrictMath.sqrt
        if (have_) {
            have_ = false;
            return cached_;
        }
        double v1, v2, s;
        do {
            v1 = 2 * nextDouble() - 1;
            v2 = 2 * nextDouble() - 1;
            s = v1 * v1 + v2 * v2;
        } while (s >= 1 || s == 0);
        const double m = std::sqrt(-2 * fdlibm_log(s) / s);
        cached_ = v2 * m;
        have_ = true;
        return v1 * m;
    }

  private:
    uint64_t seed_;
    double cached_ = 0;
    bool have_ = false;
};

// The (user-item x context) rating matrix as flat tuples in MatrixIterator (CRS) order + the id-space sizes.
struct RatingData {
    int32_t n_users = 0, n_items = 0, n_conds = 0, n_dims = 0;
    std::vector<int32_t> u, j, ctx;
    std::vector<double> r;
    std::vector<int32_t> pair;        // the tuple's row of rateMatrix (its user-item pair id); empty where the source has none
    std::vector<int32_t> cond_dim;    // condition -> context dimension (DataDAO.condDimensionMap)
    std::vector<int32_t> ctx_ptr, ctx_conds;
    std::vector<int32_t> empty_conds; // EmptyContextConditions (DataDAO.java:213-214): the ":na" conditions in header order
    double min_rate = 1, max_rate = 5;
    int64_t n() const { return (int64_t)r.size(); }
    RatingData subset(const std::vector<int64_t> &idx) const {
        RatingData d = *this;
        d.u.clear(), d.j.clear(), d.ctx.clear(), d.r.clear(), d.pair.clear();
        for (int64_t t : idx) {
            if (!pair.empty()) d.pair.push_back(pair[(size_t)t]);
            d.u.push_back(u[(size_t)t]);
            d.j.push_back(j[(size_t)t]);
            d.ctx.push_back(ctx[(size_t)t]);
            d.r.push_back(r[(size_t)t]);
        }
        return d;
    }
};

// DataSplitter.splitFolds (src/carskit/data/processor/DataSplitter.java:102-133): fold label 1..k per matrix entry
inline std::vector<int> split_folds(int64_t n, int k_fold, int64_t seed, int *num_fold) {
    const int nf = (int64_t)k_fold > n ? (int)n : k_fold;
    JavaRandom rnd(seed);
    std::vector<double> rdm((size_t)n);
    std::vector<int> fold((size_t)n);
    const double indv = ((double)n + 0.0) / nf;
    for (int64_t i = 0; i < n; ++i) {
        rdm[(size_t)i] = rnd.nextDouble();
        fold[(size_t)i] = (int)((double)i / indv) + 1;
    }
    std::vector<int64_t> ord((size_t)n);
    std::iota(ord.begin(), ord.end(), 0);
    std::stable_sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return rdm[(size_t)a] < rdm[(size_t)b]; });
    std::vector<int> out((size_t)n);
    for (int64_t i = 0; i < n; ++i) out[(size_t)i] = fold[(size_t)ord[(size_t)i]];
    *num_fold = nf;
    return out;
}

// static hyper-parameters (Recommender.java:194-247, IterativeRecommender.java:80-103, FM.java:53-54)
struct Conf {
    int numFactors = 10, numIters = 100;
    double initLRate = java_float("0.01"), maxLRate = -1, decay = -1;
    bool isBoldDriver = false, verbose = true;
    double regU = java_float("0.01"), regI = regU, regB = regU, regC = regU, regLw = 0, regLf = 0;
    std::string earlyStop; // "", "Loss", "MAE", "RMSE"
    int64_t randSeed = 1;
    unsigned flags = 0;
    int device = 0;
    int deviceShare = 1;       // recommenders training concurrently on `device` (`cv -p on`: the folds that landed on it): cmi_set_device_share
    int shards = 1;            // --shards N: ONE recommender sharded by user over N GPUs (cmi_group_*; the Java host's -Dcarskit.shards)
    double shardsLrScale = 0;  // local learning-rate scale of a sharded run; 0 = sqrt(shards)
    // item.ranking / ratings.setup -threshold / eval.strategy (Recommender.java:211-217,242; CARSKit.java:262)
    bool isRankingPred = false;
    int numRecs = 10, numIgnore = -1;
    double binThold = -1.0;
    std::string evalStrategy = "ucu";
    int numF = 10; // `-f` of the recommender line (CAMF_LCS.java:37: algoOptions.getInt("-f", 10))
    // `output.setup ... --save-model` (Recommender.java:240,364-365) and the reference's loadModel() branch of execute()
    // (Recommender.java:332-338: reachable only with Debug.OFF there; here the driver's --load-model flag)
    bool isSaveModel = false, loadModel = false;
    std::string workingPath;
    // ItemKNN / UserKNN: num.neighbors, similarity, num.shrinkage (Recommender.java:244-246,426)
    int knn = 20, knnShrinkage = 0;
    bool knnShrinkageSet = false, knnShrinkagePresent = false;
    std::string similarity = "PCC", knnShrinkageRaw;
    // SLIM=-l1 -l2 -k (SLIM.java:71-74): the regularisers are Java floats, held here as the doubles they widen to
    double slimL1 = 0, slimL2 = 0;
    int slimKnn = 0;
    // RankALS=-sw on|off (RankALS.java:71: algoOptions.isOn("-sw")); without the RankALS key the reference's algoOptions is null
    bool rankalsSw = false, rankalsSet = false;
    // RankSGD=-numrates size|reference: what RankSGD.java:71 divides by.  `reference` (and the absent key) is the reference as it stands:
    // numRates is never assigned (Recommender.java:141), so the divisor is 0; `size` is the number of ratings of the 2-D train matrix
    bool ranksgdNumRatesSize = false;
    // CPTF=-keys reference|indexof: the keys of the training tensor.  `reference` (and the absent key) is DataDAO.java:461 as it stands
    // (a condition already listed gets its list's last index); `indexof` gives the condition's own index, what getKeys uses
    bool cptfKeysIndexOf = false;
    double reg = java_float("0.01"); // reg.lambda's main parameter (Recommender.java: reg), what CPTF.java:104-106 uses
    std::shared_ptr<int64_t> bprStream; // BPR: the 48-bit state of happy.coding's Randoms stream, shared by the folds of a run (null: from randSeed)
    Conf() {}
    explicit Conf(const FileConfiger &cf) {
        if (cf.contains("learn.rate")) {
            LineConfiger lc = cf.getParamOptions("learn.rate");
            initLRate = java_float(lc.getMainParam());
            maxLRate = lc.getFloat("-max", -1);
            isBoldDriver = lc.contains("-bold-driver");
            decay = lc.getFloat("-decay", -1);
        }
        if (cf.contains("reg.lambda")) {
            LineConfiger ro = cf.getParamOptions("reg.lambda");
            reg = java_float(ro.getMainParam());
            regU = ro.getFloat("-u", reg);
            regI = ro.getFloat("-i", reg);
            regB = ro.getFloat("-b", reg);
            regC = ro.getFloat("-c", reg);
        }
        numFactors = cf.getInt("num.factors", 10);
        numIters = cf.getInt("num.max.iter", 100);
        if (cf.contains("evaluation.setup")) {
            LineConfiger ev = cf.getParamOptions("evaluation.setup");
            const std::string es = lower(ev.getString("--early-stop"));
            earlyStop = es == "loss" ? "Loss" : es == "mae" ? "MAE" : es == "rmse" ? "RMSE" : "";
            randSeed = ev.getLong("--rand-seed", 1);
        }
        if (cf.contains("output.setup")) {
            verbose = cf.getParamOptions("output.setup").isOn("-verbose", true);
            isSaveModel = cf.getParamOptions("output.setup").contains("--save-model");
        }
        if (cf.contains("item.ranking")) {
            LineConfiger rk = cf.getParamOptions("item.ranking");
            isRankingPred = rk.isMainOn();
            numRecs = rk.getInt("-topN", -1);
            if (numRecs < 0) numRecs = 10;
            numIgnore = rk.getInt("-ignore", -1);
            if (rk.contains("-diverse")) throw std::runtime_error("item.ranking -diverse is not on the accelerated path");
        }
        if (cf.contains("ratings.setup")) binThold = cf.getParamOptions("ratings.setup").getFloat("-threshold", -1);
        evalStrategy = lower(cf.getString("eval.strategy", "ucu"));
        if (cf.contains("recommender")) numF = cf.getParamOptions("recommender").getInt("-f", 10);
        knn = cf.getInt("num.neighbors", 20);
        similarity = cf.getString("similarity", "PCC");
        if (cf.contains("num.shrinkage")) { // Integer.parseInt: an optional sign and decimal digits only
            knnShrinkagePresent = true;
            knnShrinkageRaw = cf.getString("num.shrinkage");
            const std::string &v = knnShrinkageRaw;
            size_t p = (!v.empty() && (v[0] == '-' || v[0] == '+')) ? 1 : 0;
            knnShrinkageSet = p < v.size() && v.find_first_not_of("0123456789", p) == std::string::npos;
            if (knnShrinkageSet) knnShrinkage = (int)std::strtol(v.c_str(), nullptr, 10);
        }
        if (cf.contains("SLIM")) { // SLIM.java:71-74: getFloat("-l1"), getFloat("-l2"), getInt("-k")
            LineConfiger sl = cf.getParamOptions("SLIM");
            slimL1 = sl.getFloat("-l1", 0);
            slimL2 = sl.getFloat("-l2", 0);
            slimKnn = sl.getInt("-k", 0);
        }
        if (cf.contains("RankALS")) {
            rankalsSet = true;
            rankalsSw = cf.getParamOptions("RankALS").isOn("-sw", false);
        }
        if (cf.contains("RankSGD")) {
            const std::string v = lower(cf.getParamOptions("RankSGD").getString("-numrates", "reference"));
            if (v != "size" && v != "reference") throw std::runtime_error("RankSGD=-numrates " + v + ": size or reference");
            ranksgdNumRatesSize = v == "size";
        }
        if (cf.contains("CPTF")) {
            const std::string v = lower(cf.getParamOptions("CPTF").getString("-keys", "reference"));
            if (v != "indexof" && v != "reference") throw std::runtime_error("CPTF=-keys " + v + ": indexof or reference");
            cptfKeysIndexOf = v == "indexof";
        }
        if (cf.contains("FM")) {
            LineConfiger fm = cf.getParamOptions("FM");
            regLw = fm.getFloat("-lw", 0);
            regLf = fm.getFloat("-lf", 0);
        }
    }
};

typedef std::map<std::string, double> Measures;
typedef std::function<void(const std::string &)> Logger;

inline void check(int rc, cmi_handle h, const char *what) {
    if (rc != CMI_OK) throw std::runtime_error(std::string(what) + ": " + cmi_last_error(h));
}

// carskit.generic.Recommender + IterativeRecommender (+ ContextRecommender), for the models libcarskit_mi355x runs
class IterativeRecommender {
  public:
    IterativeRecommender(int model, const char *name, bool is_cars, const RatingData &train, const RatingData &test, int fold,
                         const Conf &conf, Logger log)
        : algoName(name), model_(model), isCARS_(is_cars), trainMatrix(train), testMatrix(test), fold_(fold), conf_(conf),
          log_(log) {
        lRate = conf.initLRate;
        double s = 0;
        int64_t cnt = 0;
        for (double v : train.r) { // SparseMatrix.getGlobalAvg: sum / #non-zero
            s += v;
            if (v != 0.0) ++cnt;
        }
        globalMean = cnt ? s / (double)cnt : std::nan("");
    }
    virtual ~IterativeRecommender() {
        if (g_) cmi_group_destroy(g_);
        if (h_) cmi_destroy(h_);
    }

    // ---- hooks, named as in the reference ---------------------------------------------------------------------
    virtual void initModel() { // IterativeRecommender.java:232-247 + the model class: P, Q ~ N(0,0.1), then the biases
        JavaRandom rnd(conf_.randSeed);   // the reference's init stream is unseeded: any stream is as faithful
        auto gauss = [&](std::vector<double> &v, size_t n) {
            v.resize(n);
            for (double &x : v) x = 0.0 + 0.1 * rnd.nextGaussian();
        };
        auto unif = [&](std::vector<double> &v, size_t n) {
            v.resize(n);
            for (double &x : v) x = rnd.nextDouble();
        };
        const size_t nu = (size_t)trainMatrix.n_users, ni = (size_t)trainMatrix.n_items, nc = (size_t)trainMatrix.n_conds,
                     k = (size_t)conf_.numFactors;
        gauss(state[CMI_STATE_P], nu * k);
        gauss(state[CMI_STATE_Q], ni * k);
        switch (model_) {
        case CMI_MODEL_BIASEDMF:
            gauss(state[CMI_STATE_USER_BIAS], nu);
            gauss(state[CMI_STATE_ITEM_BIAS], ni);
            break;
        case CMI_MODEL_CAMF_C:
            gauss(state[CMI_STATE_USER_BIAS], nu);
            gauss(state[CMI_STATE_ITEM_BIAS], ni);
            gauss(state[CMI_STATE_COND_BIAS], nc);
            break;
        case CMI_MODEL_CAMF_CI:
            gauss(state[CMI_STATE_USER_BIAS], nu);
            unif(state[CMI_STATE_IC_BIAS], ni * nc); // icBias.init() = uniform(0,1), CAMF_CI.java:60
            break;
        case CMI_MODEL_CAMF_CU:
            gauss(state[CMI_STATE_ITEM_BIAS], ni);
            unif(state[CMI_STATE_UC_BIAS], nu * nc);
            break;
        case CMI_MODEL_CAMF_CUCI:
            gauss(state[CMI_STATE_UC_BIAS], nu * nc);
            gauss(state[CMI_STATE_IC_BIAS], ni * nc);
            break;
        case CMI_MODEL_SVDPP: // SVDPlusPlus.java:46-53: BiasedMF.initModel, then Y.init(initMean, initStd)
            gauss(state[CMI_STATE_USER_BIAS], nu);
            gauss(state[CMI_STATE_ITEM_BIAS], ni);
            gauss(state[CMI_STATE_Y], ni * k);
            break;
        case CMI_MODEL_CAMF_ICS: // CAMF_ICS.java:36-51: isRankingPred -> P.init(), Q.init() (uniform) on top of the gaussian draws
            unif(state[CMI_STATE_P], nu * k);
            unif(state[CMI_STATE_Q], ni * k);
            state[CMI_STATE_CC_MATRIX].assign(nc * nc, 1.0);
            break;
        case CMI_MODEL_CAMF_LCS: // CAMF_LCS.java:34-41: cfMatrix_LCS.init() = uniform(0,1)
            unif(state[CMI_STATE_CF_MATRIX], nc * (size_t)conf_.numF);
            break;
        case CMI_MODEL_CAMF_MCS: { // CAMF_MCS.java:41-52: cVector_MCS.init(upbound) = uniform(0, 1/sqrt(numContextDims))
            const double up = 1.0 / std::sqrt((double)std::max(1, trainMatrix.n_dims));
            unif(state[CMI_STATE_C_VECTOR], nc);
            for (double &x : state[CMI_STATE_C_VECTOR]) x *= up;
            break;
        }
        default: break;
        }
    }

    // --shards N (N > 1, models whose ratings commute): the epochs run on a cmi_group -- the library cuts the ratings by user, runs the
    // shards' epochs concurrently and merges the item-side moves (RCCL reduce-scatter + all-gather, or in-process when shards share a
    // device) -- steered by the unchanged isConverged(); `--early-stop MAE|RMSE` scores the shards' resident test tuples.  Afterwards the
    // model is copied back and lives on in a plain handle, so evaluation / ranking / --save-model are the single-GPU code below.
    void trainSharded(unsigned flags) {
        auto gcheck = [&](int rc, const char *what) {
            if (rc != CMI_OK) throw std::runtime_error(std::string(what) + ": " + cmi_group_last_error(g_));
        };
        int rc = cmi_group_create(model_, conf_.numFactors, trainMatrix.n_users, trainMatrix.n_items, trainMatrix.n_conds, conf_.shards, nullptr,
                                  flags, &g_);
        if (rc != CMI_OK) throw std::runtime_error(std::string("cmi_group_create: ") + cmi_group_last_error(nullptr));
        gcheck(cmi_group_set_hparams(g_, conf_.regU, conf_.regI, conf_.regB, conf_.regC, globalMean), "cmi_group_set_hparams");
        if (isCARS_) {
            gcheck(cmi_group_set_ratings(g_, trainMatrix.n(), trainMatrix.u.data(), trainMatrix.j.data(), trainMatrix.ctx.data(),
                                         trainMatrix.r.data(), (int32_t)trainMatrix.ctx_ptr.size() - 1, trainMatrix.ctx_ptr.data(),
                                         trainMatrix.ctx_conds.data()),
                   "cmi_group_set_ratings");
        } else {
            std::vector<int32_t> u2, j2;
            std::vector<double> r2;
            to2d(trainMatrix, u2, j2, r2);
            gcheck(cmi_group_set_ratings(g_, (int64_t)r2.size(), u2.data(), j2.data(), nullptr, r2.data(), 0, nullptr, nullptr), "cmi_group_set_ratings");
        }
        for (auto &kv : state) gcheck(cmi_group_set_state(g_, kv.first, kv.second.data(), (int64_t)kv.second.size(), CMI_DTYPE_F64), "cmi_group_set_state");
        gcheck(cmi_group_set_lr_scale(g_, conf_.shardsLrScale > 0 ? conf_.shardsLrScale : std::sqrt((double)conf_.shards)), "cmi_group_set_lr_scale");
        if (conf_.earlyStop == "MAE" || conf_.earlyStop == "RMSE") {
            gcheck(cmi_group_set_eval_ratings(g_, testMatrix.n(), testMatrix.u.data(), testMatrix.j.data(), isCARS_ ? testMatrix.ctx.data() : nullptr,
                                              testMatrix.r.data()),
                   "cmi_group_set_eval_ratings");
            evalResident_ = testMatrix.n() > 0;
        }
        for (int iter = 1; iter <= conf_.numIters; ++iter) {
            gcheck(cmi_group_train_epoch(g_, lRate, &loss), "cmi_group_train_epoch");
            losses.push_back(loss);
            itersDone = iter;
            if (isConverged(iter)) break;
        }
        for (auto &kv : state) gcheck(cmi_group_get_state(g_, kv.first, kv.second.data(), (int64_t)kv.second.size(), CMI_DTYPE_F64), "cmi_group_get_state");
        cmi_group_destroy(g_);
        g_ = nullptr;
        evalResident_ = false;
    }

    virtual void buildModel() {
        const bool chained = model_ == CMI_MODEL_CAMF_C || (model_ >= CMI_MODEL_SVDPP && model_ <= CMI_MODEL_CAMF_MCS);
        unsigned flags = conf_.flags | (chained ? CMI_FLAG_SCHED_SERIAL : 0u); // one dependent chain in CRS order
        const bool sharded = conf_.shards > 1 && !chained && !conf_.loadModel;
        if (sharded) trainSharded(flags);
        int rc = cmi_create(model_, conf_.numFactors, trainMatrix.n_users, trainMatrix.n_items, trainMatrix.n_conds,
                            conf_.device, flags, &h_);
        if (rc != CMI_OK) throw std::runtime_error(std::string("cmi_create: ") + cmi_last_error(nullptr));
        check(cmi_set_hparams(h_, conf_.regU, conf_.regI, conf_.regB, conf_.regC, globalMean), h_, "cmi_set_hparams");
        if (conf_.deviceShare > 1) check(cmi_set_device_share(h_, conf_.deviceShare), h_, "cmi_set_device_share");
        if (model_ >= CMI_MODEL_CAMF_ICS && model_ <= CMI_MODEL_CAMF_MCS)
            check(cmi_set_sim_params(h_, conf_.numF, std::max(1, trainMatrix.n_dims), trainMatrix.empty_conds.data(),
                                     (int)trainMatrix.empty_conds.size()),
                  h_, "cmi_set_sim_params");
        if (isCARS_) {
            check(cmi_set_ratings(h_, trainMatrix.n(), trainMatrix.u.data(), trainMatrix.j.data(), trainMatrix.ctx.data(),
                                  trainMatrix.r.data(), (int32_t)trainMatrix.ctx_ptr.size() - 1, trainMatrix.ctx_ptr.data(),
                                  trainMatrix.ctx_conds.data()),
                  h_, "cmi_set_ratings");
        } else { // Recommender.initModel (:1076-1081): the 2-D train matrix, mean over contexts per (user,item)
            std::vector<int32_t> u2, j2;
            std::vector<double> r2;
            to2d(trainMatrix, u2, j2, r2);
            check(cmi_set_ratings(h_, (int64_t)r2.size(), u2.data(), j2.data(), nullptr, r2.data(), 0, nullptr, nullptr), h_,
                  "cmi_set_ratings");
        }
        if (*cmi_schedule_note(h_) && log_) log_(std::string("note: ") + cmi_schedule_note(h_));
        for (auto &kv : state) // copy-in
            check(cmi_set_state(h_, kv.first, kv.second.data(), (int64_t)kv.second.size(), CMI_DTYPE_F64), h_, "cmi_set_state");
        if (!sharded && (conf_.earlyStop == "MAE" || conf_.earlyStop == "RMSE")) { // evaluated after every epoch: keep the test tuples on the device
            check(cmi_set_eval_ratings(h_, testMatrix.n(), testMatrix.u.data(), testMatrix.j.data(),
                                       isCARS_ ? testMatrix.ctx.data() : nullptr, testMatrix.r.data()),
                  h_, "cmi_set_eval_ratings");
            evalResident_ = testMatrix.n() > 0;
        }
        if (conf_.loadModel) { // Recommender.execute's loadModel() branch (:332-338): the stored model instead of initModel + the epochs
            int done = 0;
            check(cmi_load_model(h_, modelPath().c_str(), &lRate, &last_loss, &done), h_, "cmi_load_model");
            itersDone = done;
            if (log_) log_("A recommender model is loaded from " + modelPath());
        } else if (!sharded) {
            for (int iter = 1; iter <= conf_.numIters; ++iter) {
                check(cmi_train_epoch(h_, lRate, &loss), h_, "cmi_train_epoch"); // the for(MatrixEntry me : trainMatrix) body
                losses.push_back(loss);
                itersDone = iter;
                if (isConverged(iter)) break;
            }
        }
        for (auto &kv : state) // copy-back
            check(cmi_get_state(h_, kv.first, kv.second.data(), (int64_t)kv.second.size(), CMI_DTYPE_F64), h_, "cmi_get_state");
    }

    virtual Measures evalRatings() { // Recommender.java:504-594 (numeric part)
        double out[5] = {0, 0, 0, 0, 0};
        int64_t cnt = 0;
        if (evalResident_ && g_) {
            if (cmi_group_eval_resident(g_, trainMatrix.min_rate, trainMatrix.max_rate, out, &cnt) != CMI_OK)
                throw std::runtime_error(std::string("cmi_group_eval_resident: ") + cmi_group_last_error(g_));
        } else if (evalResident_)
            check(cmi_eval_resident(h_, trainMatrix.min_rate, trainMatrix.max_rate, out, &cnt), h_, "cmi_eval_resident");
        else
        check(cmi_eval_ratings(h_, testMatrix.n(), testMatrix.u.data(), testMatrix.j.data(),
                               isCARS_ ? testMatrix.ctx.data() : nullptr, testMatrix.r.data(), trainMatrix.min_rate,
                               trainMatrix.max_rate, out, &cnt),
              h_, "cmi_eval_ratings");
        return Measures{{"MAE", out[0]}, {"RMSE", out[1]}, {"NMAE", out[2]}, {"rMAE", out[3]}, {"rRMSE", out[4]}, {"MPE", 0.0}};
    }

    virtual Measures evalRankings() { // Recommender.java:668-964
        static const char *names[CMI_RANK_MEASURES] = {"Pre5", "Pre10", "PreN", "Rec5", "Rec10", "RecN", "AUC5", "AUC10", "AUCN",
                                                       "MAP5", "MAP10", "MAPN", "NDCG5", "NDCG10", "NDCGN", "MRR5", "MRR10",
                                                       "MRRN", "D5", "D10", "DN"};
        double out[CMI_RANK_MEASURES];
        int64_t nq = 0;
        check(cmi_eval_rankings(h_, trainMatrix.n(), trainMatrix.u.data(), trainMatrix.j.data(), trainMatrix.ctx.data(),
                                trainMatrix.r.data(), testMatrix.n(), testMatrix.u.data(), testMatrix.j.data(),
                                testMatrix.ctx.data(), testMatrix.r.data(), conf_.binThold, conf_.numRecs, conf_.numIgnore,
                                conf_.evalStrategy == "uc" ? CMI_RANK_UC : CMI_RANK_UCU, out, &nq, nullptr, nullptr, nullptr,
                                nullptr, nullptr),
              h_, "cmi_eval_rankings");
        Measures m;
        for (int i = 0; i < CMI_RANK_MEASURES; ++i) m[names[i]] = out[i];
        return m;
    }

    Measures execute() { // Recommender.java:319-366
        auto t0 = std::chrono::steady_clock::now();
        initModel();
        buildModel();
        auto t1 = std::chrono::steady_clock::now();
        measures = conf_.isRankingPred ? evalRankings() : evalRatings(); // :346
        auto t2 = std::chrono::steady_clock::now();
        measures["TrainTime"] = std::chrono::duration<double, std::milli>(t1 - t0).count();
        measures["TestTime"] = std::chrono::duration<double, std::milli>(t2 - t1).count();
        if (conf_.isSaveModel) saveModel(); // :364-365
        return measures;
    }

    // <workingPath>/<algoName>/model<foldInfo>.cmi -- the reference writes <workingPath>/<algoName>/{userFactors,itemFactors,userBiases,
    // itemBiases}<foldInfo>.bin as Java object streams and forgets the context tables (IterativeRecommender.java:249-270); here ONE
    // cmi_save_model file holds every container plus the loop's resume state (lRate, last loss, epochs done)
    std::string modelPath() const {
        return conf_.workingPath + algoName + "/model" + (fold_ > 0 ? " fold [" + std::to_string(fold_) + "]" : "") + ".cmi";
    }
    virtual void saveModel() {
        if (!h_) { // FM keeps its model behind a cmi_fm_handle, which has no persistence entry point
            if (log_) log_("--save-model: not available for " + algoName);
            return;
        }
        const std::string mk = "mkdir -p '" + conf_.workingPath + algoName + "'";
        if (std::system(mk.c_str()) != 0) throw std::runtime_error("cannot create " + conf_.workingPath + algoName);
        check(cmi_save_model(h_, modelPath().c_str(), lRate, last_loss, itersDone), h_, "cmi_save_model");
        if (log_) log_("Learned models are saved to folder \"" + conf_.workingPath + algoName + "/\"");
    }
    int itersDone = 0;

    bool isConverged(int iter) { // IterativeRecommender.java:145-199
        const float delta_loss = (float)(last_loss - loss);
        if (conf_.earlyStop == "Loss") {
            measure = loss;
            last_measure = last_loss;
        } else if (conf_.earlyStop == "MAE" || conf_.earlyStop == "RMSE") {
            measure = evalRatings()[conf_.earlyStop];
        }
        const float delta_measure = (float)(last_measure - measure);
        if (conf_.verbose && log_) {
            char buf[256];
            int len = snprintf(buf, sizeof buf, "%s%s iter %d: loss = %g, delta_loss = %g", algoName.c_str(),
                               fold_ > 0 ? (" fold [" + std::to_string(fold_) + "]").c_str() : "", iter, (double)(float)loss,
                               (double)delta_loss);
            if (lRate > 0 && len > 0 && len < (int)sizeof buf) // :169: no learning rate, no ", learn_rate" (NMF sets lRate = -1)
                snprintf(buf + len, sizeof buf - (size_t)len, ", learn_rate = %g", (double)(float)lRate);
            log_(buf);
        }
        if (std::isnan(loss) || std::isinf(loss))
            throw std::runtime_error("Loss = NaN or Infinity: current settings does not fit the recommender! Change the settings and try again!");
        const bool converged = std::fabs(loss) < 1e-5 || (delta_measure > 0 && delta_measure < 1e-5);
        if (!converged) updateLRate(iter);
        last_loss = loss;
        last_measure = measure;
        return converged;
    }

    void updateLRate(int iter) { // IterativeRecommender.java:216-229
        if (lRate <= 0) return;
        if (conf_.isBoldDriver && iter > 1) lRate = std::fabs(last_loss) > std::fabs(loss) ? lRate * 1.05 : lRate * 0.5;
        else if (conf_.decay > 0 && conf_.decay < 1) lRate *= conf_.decay;
        if (conf_.maxLRate > 0 && lRate > conf_.maxLRate) lRate = conf_.maxLRate;
    }

    static void to2d(const RatingData &d, std::vector<int32_t> &u2, std::vector<int32_t> &j2, std::vector<double> &r2) {
        // DataDAO.toTraditionalSparseMatrix: the mean of a (user, item) pair's ratings over its contexts, pairs in (user, item) order.
        // (key, tuple) pairs sorted: a cell's ratings are then added in tuple order, as a map keyed by the pair would add them.
        std::vector<std::pair<uint64_t, int64_t>> ord((size_t)d.n());
        for (int64_t t = 0; t < d.n(); ++t)
            ord[(size_t)t] = {((uint64_t)(uint32_t)d.u[(size_t)t] << 32) | (uint32_t)d.j[(size_t)t], t};
        std::sort(ord.begin(), ord.end());
        for (size_t a = 0; a < ord.size();) {
            double sum = 0.0, cnt = 0.0;
            size_t b = a;
            for (; b < ord.size() && ord[b].first == ord[a].first; ++b) {
                sum += d.r[(size_t)ord[b].second];
                cnt += 1.0;
            }
            u2.push_back((int32_t)(ord[a].first >> 32));
            j2.push_back((int32_t)(ord[a].first & 0xffffffffu));
            r2.push_back(sum / cnt);
            a = b;
        }
    }

    // Recommender.evalRatings (Recommender.java:504-594, numeric part) over bounded predictions of the test tuples, in their order;
    // NaN predictions are skipped
    Measures evalPredictions(const std::vector<double> &pred) const {
        double sa = 0, ss = 0, sra = 0, srs = 0;
        int64_t n = 0;
        for (size_t t = 0; t < pred.size(); ++t) {
            if (std::isnan(pred[t])) continue;
            const double rp = std::floor(pred[t] / trainMatrix.min_rate + 0.5) * trainMatrix.min_rate;
            const double e = std::fabs(testMatrix.r[t] - pred[t]), re = std::fabs(testMatrix.r[t] - rp);
            sa += e, ss += e * e, sra += re, srs += re * re;
            ++n;
        }
        const double mae = sa / (double)n;
        return Measures{{"MAE", mae}, {"RMSE", std::sqrt(ss / (double)n)}, {"NMAE", mae / (trainMatrix.max_rate - trainMatrix.min_rate)},
                        {"rMAE", sra / (double)n}, {"rRMSE", std::sqrt(srs / (double)n)}, {"MPE", 0.0}};
    }

    std::string algoName;
    Measures measures;
    bool evalResident_ = false;
    std::map<int, std::vector<double>> state; // CMI_STATE_* -> container (P, Q, userBias, ...)
    std::vector<double> losses;
    double lRate = 0, loss = 0, last_loss = 0, measure = 0, last_measure = 0, globalMean = 0;

  protected:
    int model_;
    bool isCARS_;
    RatingData trainMatrix, testMatrix;
    int fold_;
    Conf conf_;
    Logger log_;
    cmi_handle h_ = nullptr;
    cmi_group_handle g_ = nullptr; // live only inside trainSharded()
};

#define CARSKIT_MODEL(cls, id, cars) CARSKIT_NAMED_MODEL(cls, #cls, id, cars)
#define CARSKIT_NAMED_MODEL(cls, name, id, cars)                                                                      \
    class cls : public IterativeRecommender {                                                                          \
      public:                                                                                                          \
        cls(const RatingData &tr, const RatingData &te, int fold, const Conf &c, Logger log = nullptr)                 \
            : IterativeRecommender(id, name, cars, tr, te, fold, c, log) {}                                            \
    };
CARSKIT_MODEL(BiasedMF, CMI_MODEL_BIASEDMF, false)  // src/carskit/alg/baseline/cf/BiasedMF.java
CARSKIT_MODEL(PMF, CMI_MODEL_PMF, false)            // src/carskit/alg/baseline/cf/PMF.java
CARSKIT_MODEL(CAMF_C, CMI_MODEL_CAMF_C, true)       // src/carskit/alg/cars/adaptation/dependent/dev/CAMF_C.java
CARSKIT_MODEL(CAMF_CI, CMI_MODEL_CAMF_CI, true)     // .../dev/CAMF_CI.java
CARSKIT_MODEL(CAMF_CU, CMI_MODEL_CAMF_CU, true)     // .../dev/CAMF_CU.java
CARSKIT_MODEL(CAMF_CUCI, CMI_MODEL_CAMF_CUCI, true) // .../dev/CAMF_CUCI.java
CARSKIT_NAMED_MODEL(SVDPlusPlus, "SVD++", CMI_MODEL_SVDPP, false) // src/carskit/alg/baseline/cf/SVDPlusPlus.java:42 (algoName = "SVD++"; 2-D train matrix)
#undef CARSKIT_MODEL
#undef CARSKIT_NAMED_MODEL

// The similarity-based CAMF models are top-N recommenders: their constructors set the static isRankingPred = true
// (CAMF_ICS.java:31, CAMF_LCS.java:31, CAMF_MCS.java:37), so execute() evaluates with evalRankings() whatever item.ranking says.
#define CARSKIT_SIM_MODEL(cls, id)                                                                                     \
    class cls : public IterativeRecommender {                                                                          \
      public:                                                                                                          \
        cls(const RatingData &tr, const RatingData &te, int fold, const Conf &c, Logger log = nullptr)                 \
            : IterativeRecommender(id, #cls, true, tr, te, fold, c, log) {                                             \
            conf_.isRankingPred = true;                                                                                \
        }                                                                                                              \
    };
CARSKIT_SIM_MODEL(CAMF_ICS, CMI_MODEL_CAMF_ICS) // src/carskit/alg/cars/adaptation/dependent/sim/CAMF_ICS.java
CARSKIT_SIM_MODEL(CAMF_LCS, CMI_MODEL_CAMF_LCS) // .../sim/CAMF_LCS.java
CARSKIT_SIM_MODEL(CAMF_MCS, CMI_MODEL_CAMF_MCS) // .../sim/CAMF_MCS.java
#undef CARSKIT_SIM_MODEL

// src/carskit/alg/cars/adaptation/dependent/FM.java: w0 = 0, w ~ U(0,1), V ~ N(0,0.1) (:65-70); numIters ALS sweeps, no
// convergence check; evaluation through the generic evalRatings recipe on bounded predictions.
class FM : public IterativeRecommender {
  public:
    FM(const RatingData &tr, const RatingData &te, int fold, const Conf &c, Logger log = nullptr)
        : IterativeRecommender(-1, "FM", true, tr, te, fold, c, log) {}
    ~FM() override {
        if (fm_) cmi_fm_destroy(fm_);
    }
    void initModel() override {
        JavaRandom rnd(conf_.randSeed);
        const size_t p = (size_t)trainMatrix.n_users + trainMatrix.n_items + trainMatrix.n_conds;
        w.resize(p);
        for (double &x : w) x = rnd.nextDouble();
        V.resize(p * (size_t)conf_.numFactors);
        for (double &x : V) x = 0.0 + 0.1 * rnd.nextGaussian();
        w0 = 0.0;
    }
    void buildModel() override {
        if (cmi_fm_create(conf_.numFactors, trainMatrix.n_users, trainMatrix.n_items, trainMatrix.n_conds,
                          std::max(1, trainMatrix.n_dims), conf_.device, 0, &fm_) != CMI_OK)
            throw std::runtime_error(std::string("cmi_fm_create: ") + cmi_fm_last_error(nullptr));
        fmcheck(cmi_fm_set_hparams(fm_, conf_.regLw, conf_.regLf, 0), "cmi_fm_set_hparams");
        fmcheck(cmi_fm_set_ratings(fm_, trainMatrix.n(), trainMatrix.u.data(), trainMatrix.j.data(), trainMatrix.ctx.data(),
                                   trainMatrix.r.data()), "cmi_fm_set_ratings");
        fmcheck(cmi_fm_set_model(fm_, w0, w.data(), V.data()), "cmi_fm_set_model");
        fmcheck(cmi_fm_train(fm_, conf_.numIters), "cmi_fm_train");
        fmcheck(cmi_fm_get_model(fm_, &w0, w.data(), V.data()), "cmi_fm_get_model");
    }
    Measures evalRankings() override { // Recommender.java:668-964 with FM.predict
        static const char *names[CMI_RANK_MEASURES] = {"Pre5", "Pre10", "PreN", "Rec5", "Rec10", "RecN", "AUC5", "AUC10", "AUCN",
                                                       "MAP5", "MAP10", "MAPN", "NDCG5", "NDCG10", "NDCGN", "MRR5", "MRR10",
                                                       "MRRN", "D5", "D10", "DN"};
        double out[CMI_RANK_MEASURES];
        int64_t nq = 0;
        if (cmi_fm_eval_rankings(fm_, trainMatrix.n(), trainMatrix.u.data(), trainMatrix.j.data(), trainMatrix.ctx.data(),
                                 trainMatrix.r.data(), testMatrix.n(), testMatrix.u.data(), testMatrix.j.data(),
                                 testMatrix.ctx.data(), testMatrix.r.data(), conf_.binThold, conf_.numRecs, conf_.numIgnore,
                                 conf_.evalStrategy == "uc" ? CMI_RANK_UC : CMI_RANK_UCU, out, &nq, nullptr, nullptr, nullptr,
                                 nullptr, nullptr) != CMI_OK)
            throw std::runtime_error(std::string("cmi_fm_eval_rankings: ") + cmi_fm_last_error(fm_));
        Measures m;
        for (int i = 0; i < CMI_RANK_MEASURES; ++i) m[names[i]] = out[i];
        return m;
    }
    Measures evalRatings() override {
        std::vector<double> pred((size_t)testMatrix.n());
        fmcheck(cmi_fm_predict_batch(fm_, testMatrix.n(), testMatrix.u.data(), testMatrix.j.data(), testMatrix.ctx.data(), 1,
                                     trainMatrix.min_rate, trainMatrix.max_rate, pred.data()), "cmi_fm_predict_batch");
        return evalPredictions(pred);
    }
    double w0 = 0;
    std::vector<double> w, V;

  private:
    void fmcheck(int rc, const char *what) {
        if (rc != CMI_OK) throw std::runtime_error(std::string(what) + ": " + cmi_fm_last_error(fm_));
    }
    cmi_fm_handle fm_ = nullptr;
};

// What ItemKNN, UserKNN, SlopeOne, NMF, SLIM and RankALS share: a model of the 2-D train matrix behind a handle H of the C ABI.  The
// defaults here are those of the rating models: nothing to initialise, nothing to save (the reference's saveModel() of the memory-based
// models is empty), evaluation through the generic evalRatings recipe on bounded predictions.  NMF, SLIM and RankALS draw their own
// model in initModel(); the top-N models SLIM and RankALS evaluate through evalRankings() and refuse predictBounded(); RankALS saves
// the P and Q it trains.
template <typename H, int (*destroy)(H), const char *(*last_error)(H),
          int (*set_ratings)(H, int64_t, const int32_t *, const int32_t *, const double *)>
class PairRecommender : public IterativeRecommender {
  public:
    PairRecommender(const char *name, const RatingData &tr, const RatingData &te, int fold, const Conf &c, Logger log)
        : IterativeRecommender(-1, name, false, tr, te, fold, c, log) {}
    ~PairRecommender() override {
        if (h_) destroy(h_);
    }
    void initModel() override {}
    Measures evalRatings() override { // Recommender.java:504-594 (numeric part); NaN predictions are skipped
        std::vector<double> pred((size_t)testMatrix.n());
        predictBounded(pred.data());
        return evalPredictions(pred);
    }
    void saveModel() override {}

  protected:
    virtual void predictBounded(double *pred) = 0; // the test tuples, bounded to the train matrix's rating scale
    void setRatings(const char *what) {
        std::vector<int32_t> u2, j2;
        std::vector<double> r2;
        to2d(trainMatrix, u2, j2, r2);
        check(set_ratings(h_, (int64_t)r2.size(), u2.data(), j2.data(), r2.data()), what);
    }
    // Recommender.java:668-964 with the handle's predict(u, j) as the scorer (eval: the handle's cmi_*_eval_rankings)
    template <typename Eval>
    Measures evalRankingsWith(Eval eval, const char *what) {
        static const char *names[CMI_RANK_MEASURES] = {"Pre5", "Pre10", "PreN", "Rec5", "Rec10", "RecN", "AUC5", "AUC10", "AUCN",
                                                       "MAP5", "MAP10", "MAPN", "NDCG5", "NDCG10", "NDCGN", "MRR5", "MRR10",
                                                       "MRRN", "D5", "D10", "DN"};
        double out[CMI_RANK_MEASURES];
        int64_t nq = 0;
        check(eval(h_, trainMatrix.n(), trainMatrix.u.data(), trainMatrix.j.data(), trainMatrix.ctx.data(), trainMatrix.r.data(),
                   testMatrix.n(), testMatrix.u.data(), testMatrix.j.data(), testMatrix.ctx.data(), testMatrix.r.data(), conf_.binThold,
                   conf_.numRecs, conf_.numIgnore, conf_.evalStrategy == "uc" ? CMI_RANK_UC : CMI_RANK_UCU, out, &nq, nullptr, nullptr,
                   nullptr, nullptr, nullptr), what);
        Measures m;
        for (int i = 0; i < CMI_RANK_MEASURES; ++i) m[names[i]] = out[i];
        return m;
    }
    // IterativeRecommender.java:249-270 writes P and Q, which the factor models of this family train: they go through the writer of the
    // MF classes, as the states of a PMF handle with fp64 state (the same two containers, no bit lost), into modelPath()
    void saveFactors(const std::vector<double> &P, const std::vector<double> &Q) {
        cmi_handle m = nullptr;
        if (cmi_create(CMI_MODEL_PMF, conf_.numFactors, trainMatrix.n_users, trainMatrix.n_items, 0, conf_.device, CMI_FLAG_STATE_F64,
                       &m) != CMI_OK)
            throw std::runtime_error(std::string("cmi_create: ") + cmi_last_error(nullptr));
        try {
            carskit::check(cmi_set_state(m, CMI_STATE_P, P.data(), (int64_t)P.size(), CMI_DTYPE_F64), m, "cmi_set_state");
            carskit::check(cmi_set_state(m, CMI_STATE_Q, Q.data(), (int64_t)Q.size(), CMI_DTYPE_F64), m, "cmi_set_state");
            const std::string mk = "mkdir -p '" + conf_.workingPath + algoName + "'";
            if (std::system(mk.c_str()) != 0) throw std::runtime_error("cannot create " + conf_.workingPath + algoName);
            carskit::check(cmi_save_model(m, modelPath().c_str(), lRate, last_loss, itersDone), m, "cmi_save_model");
        } catch (...) {
            cmi_destroy(m);
            throw;
        }
        cmi_destroy(m);
        if (log_) log_("Learned models are saved to folder \"" + conf_.workingPath + algoName + "/\"");
    }
    void check(int rc, const char *what) { // (a failed create leaves h_ null: the thread's message)
        if (rc != CMI_OK) throw std::runtime_error(std::string(what) + ": " + last_error(h_));
    }
    H h_ = nullptr;
};

// src/carskit/alg/baseline/cf/{ItemKNN,UserKNN}.java: the similarity matrix of the 2-D train matrix (buildCorrs) and the
// neighbourhood predict(u, j).
// num.neighbors (default 20) and similarity (default PCC) as Recommender.java:244-245 reads them; num.shrinkage as correlation() reads it
// (Recommender.java:426: cf.getInt(key) = Integer.parseInt(value), so a missing or non-integer value fails the model there and here).
class KNNRecommender : public PairRecommender<cmi_knn_handle, cmi_knn_destroy, cmi_knn_last_error, cmi_knn_set_ratings> {
  public:
    KNNRecommender(int kind, const char *name, const RatingData &tr, const RatingData &te, int fold, const Conf &c, Logger log)
        : PairRecommender(name, tr, te, fold, c, log), kind_(kind) {}
    void buildModel() override {
        if (!conf_.knnShrinkageSet) // the reference: Integer.parseInt(null) -> "null", Integer.parseInt("x") -> For input string: "x"
            throw std::runtime_error(!conf_.knnShrinkagePresent ? std::string("null (num.shrinkage is not set)")
                                                                     : "For input string: \"" + conf_.knnShrinkageRaw + "\" (num.shrinkage)");
        check(cmi_knn_create(kind_, trainMatrix.n_users, trainMatrix.n_items, conf_.device, 0, &h_), "cmi_knn_create");
        setRatings("cmi_knn_set_ratings");
        check(cmi_knn_build(h_, cmi_knn_measure(conf_.similarity.c_str()), conf_.knnShrinkage, trainMatrix.min_rate,
                            trainMatrix.max_rate), "cmi_knn_build");
    }

  private:
    void predictBounded(double *pred) override {
        check(cmi_knn_predict_batch(h_, testMatrix.n(), testMatrix.u.data(), testMatrix.j.data(), conf_.knn, globalMean, 1,
                                    trainMatrix.min_rate, trainMatrix.max_rate, pred), "cmi_knn_predict_batch");
    }
    int kind_;
};
class ItemKNN : public KNNRecommender {
  public:
    ItemKNN(const RatingData &tr, const RatingData &te, int fold, const Conf &c, Logger log = nullptr)
        : KNNRecommender(CMI_KNN_ITEM, "ItemKNN", tr, te, fold, c, log) {}
};
class UserKNN : public KNNRecommender {
  public:
    UserKNN(const RatingData &tr, const RatingData &te, int fold, const Conf &c, Logger log = nullptr)
        : KNNRecommender(CMI_KNN_USER, "UserKNN", tr, te, fold, c, log) {}
};

// src/carskit/alg/baseline/cf/SlopeOne.java: the deviation and cardinality matrices of the 2-D train matrix (buildModel) and
// predict(u, j).  No parameters.
class SlopeOne : public PairRecommender<cmi_slope_handle, cmi_slope_destroy, cmi_slope_last_error, cmi_slope_set_ratings> {
  public:
    SlopeOne(const RatingData &tr, const RatingData &te, int fold, const Conf &c, Logger log = nullptr)
        : PairRecommender("SlopeOne", tr, te, fold, c, log) {}
    void buildModel() override {
        check(cmi_slope_create(trainMatrix.n_users, trainMatrix.n_items, conf_.device, 0, &h_), "cmi_slope_create");
        setRatings("cmi_slope_set_ratings");
        check(cmi_slope_build(h_), "cmi_slope_build");
    }

  private:
    void predictBounded(double *pred) override {
        check(cmi_slope_predict_batch(h_, testMatrix.n(), testMatrix.u.data(), testMatrix.j.data(), globalMean, 1, trainMatrix.min_rate,
                                      trainMatrix.max_rate, pred), "cmi_slope_predict_batch");
    }
};

// src/carskit/alg/baseline/cf/NMF.java: W (numUsers x numFactors) and H (numFactors x numItems) by multiplicative updates over the 2-D
// train matrix.  Parameters: num.factors, num.max.iter.  lRate = -1 (NMF.java:51): updateLRate returns at once.
class NMF : public PairRecommender<cmi_nmf_handle, cmi_nmf_destroy, cmi_nmf_last_error, cmi_nmf_set_ratings> {
  public:
    NMF(const RatingData &tr, const RatingData &te, int fold, const Conf &c, Logger log = nullptr)
        : PairRecommender("NMF", tr, te, fold, c, log) {
        lRate = -1;
    }
    void initModel() override { // NMF.java:56-65
        JavaRandom rnd(conf_.randSeed);
        const size_t nu = (size_t)trainMatrix.n_users, ni = (size_t)trainMatrix.n_items, k = (size_t)conf_.numFactors;
        // super.initModel() (IterativeRecommender.java:235-241): P and Q, gaussian.  NMF never reads them, but they move the stream
        for (size_t t = 0; t < (nu + ni) * k; ++t) (void)rnd.nextGaussian();
        W.resize(nu * k);
        H.resize(k * ni);
        for (double &x : W) x = rnd.nextDouble() * 0.01; // W.init(0.01): uniform(0, 0.01)
        for (double &x : H) x = rnd.nextDouble() * 0.01; // H.init(0.01)
    }
    void buildModel() override { // NMF.java:67-131
        check(cmi_nmf_create(conf_.numFactors, trainMatrix.n_users, trainMatrix.n_items, conf_.device, 0, &h_), "cmi_nmf_create");
        setRatings("cmi_nmf_set_ratings");
        check(cmi_nmf_set_model(h_, W.data(), H.data()), "cmi_nmf_set_model");
        for (int iter = 1; iter <= conf_.numIters; ++iter) {
            const int rc = cmi_nmf_iterate(h_, &loss); // W phase, H phase, loss
            if (rc != CMI_E_NUMERIC) check(rc, "cmi_nmf_iterate"); // a NaN / Inf loss: isConverged reports it, as in the reference
            losses.push_back(loss);
            itersDone = iter;
            if (isConverged(iter)) break;
        }
        check(cmi_nmf_get_model(h_, W.data(), H.data()), "cmi_nmf_get_model");
    }
    // the reference's saveModel() writes P and Q (IterativeRecommender.java:249-270), which NMF never trains, and neither W nor H: there
    // is nothing of the model to save
    void saveModel() override {}
    std::vector<double> W, H; // numUsers x numFactors; numFactors x numItems

  private:
    void predictBounded(double *pred) override {
        check(cmi_nmf_predict_batch(h_, testMatrix.n(), testMatrix.u.data(), testMatrix.j.data(), 1, trainMatrix.min_rate,
                                    trainMatrix.max_rate, pred), "cmi_nmf_predict_batch");
    }
};

// src/carskit/alg/baseline/cf/BPMF.java: P and Q by Gibbs sampling over the 2-D train matrix.  Parameters: num.factors, num.max.iter.
// lRate = -1 (BPMF.java:47).  Two random streams: P.init(0, 1) and Q.init(0, 1) draw from librec.util.Randoms, the gaussian and gamma
// draws of buildModel from happy.coding.math.Randoms; both are seeded with --rand-seed, and the second is the handle's stream.
class BPMF : public PairRecommender<cmi_bpmf_handle, cmi_bpmf_destroy, cmi_bpmf_last_error, cmi_bpmf_set_ratings> {
  public:
    BPMF(const RatingData &tr, const RatingData &te, int fold, const Conf &c, Logger log = nullptr)
        : PairRecommender("BPMF", tr, te, fold, c, log) {
        lRate = -1;
    }
    // BPMF.java:71-75: P.init(0, 1), Q.init(0, 1), row by row (super.initModel()'s own draw of P and Q, IterativeRecommender.java:235-241,
    // comes first on the same stream and is overwritten)
    void initModel() override {
        JavaRandom rnd(conf_.randSeed);
        const size_t nu = (size_t)trainMatrix.n_users, ni = (size_t)trainMatrix.n_items, k = (size_t)conf_.numFactors;
        for (size_t t = 0; t < (nu + ni) * k; ++t) (void)rnd.nextGaussian();
        P.resize(nu * k);
        Q.resize(ni * k);
        for (double &x : P) x = 0.0 + 1.0 * rnd.nextGaussian();
        for (double &x : Q) x = 0.0 + 1.0 * rnd.nextGaussian();
    }
    void buildModel() override { // BPMF.java:52-247
        // the loss as the reference's one chain up to 2^18 terms, as BPR; else the fixed tree
        const bool small = (int64_t)trainMatrix.n() <= ((int64_t)1 << 18);
        check(cmi_bpmf_create(conf_.numFactors, trainMatrix.n_users, trainMatrix.n_items, conf_.device, small ? CMI_BPMF_FLAG_STRICT : 0u, &h_),
              "cmi_bpmf_create");
        setRatings("cmi_bpmf_set_ratings");
        check(cmi_bpmf_set_global_mean(h_, globalMean), "cmi_bpmf_set_global_mean");
        check(cmi_bpmf_set_model(h_, P.data(), Q.data()), "cmi_bpmf_set_model");
        check(cmi_bpmf_set_stream(h_, (int64_t)cmi::java_lcg_scramble(conf_.randSeed), 0, 0.0), "cmi_bpmf_set_stream");
        check(cmi_bpmf_init_hyper(h_), "cmi_bpmf_init_hyper");
        for (int iter = 1; iter <= conf_.numIters; ++iter) {
            const int rc = cmi_bpmf_iterate(h_, &loss); // both hyper steps, two Gibbs passes of each side, the loss
            if (rc != CMI_E_NUMERIC) check(rc, "cmi_bpmf_iterate"); // a NaN / Inf loss: isConverged reports it, as in the reference
            losses.push_back(loss);
            itersDone = iter;
            if (isConverged(iter)) break;
        }
        check(cmi_bpmf_get_model(h_, P.data(), Q.data()), "cmi_bpmf_get_model");
    }
    void saveModel() override { saveFactors(P, Q); }
    std::vector<double> P, Q; // numUsers x numFactors; numItems x numFactors

  private:
    void predictBounded(double *pred) override {
        check(cmi_bpmf_predict_batch(h_, testMatrix.n(), testMatrix.u.data(), testMatrix.j.data(), 1, trainMatrix.min_rate,
                                     trainMatrix.max_rate, pred), "cmi_bpmf_predict_batch");
    }
};

// src/carskit/alg/baseline/ranking/SLIM.java: the item x item weights W by coordinate descent over each item's neighbour list, for
// top-N.  Parameters: SLIM=-l1 -l2 -k, similarity, num.shrinkage, num.max.iter.  The constructor sets the static isRankingPred = true
// (SLIM.java:68), so execute() evaluates with evalRankings() whatever item.ranking says.
class SLIM : public PairRecommender<cmi_slim_handle, cmi_slim_destroy, cmi_slim_last_error, cmi_slim_set_ratings> {
  public:
    SLIM(const RatingData &tr, const RatingData &te, int fold, const Conf &c, Logger log = nullptr)
        : PairRecommender("SLIM", tr, te, fold, c, log) {
        conf_.isRankingPred = true;
    }
    // SLIM.java:78-118.  The lists come first here (they do not touch the random stream); then the stream as the reference draws it:
    // P and Q (IterativeRecommender.java:235-241, gaussian, never read), then W.init(): numItems^2 uniform draws, row by row, of which
    // the listed cells are kept (no other cell is ever read); the diagonal is 0 (:93, :116).
    void initModel() override {
        if (conf_.slimKnn > 0 && !conf_.knnShrinkageSet) // buildCorrs -> correlation(): Integer.parseInt of num.shrinkage, as for the KNN models
            throw std::runtime_error(!conf_.knnShrinkagePresent ? std::string("null (num.shrinkage is not set)")
                                                                     : "For input string: \"" + conf_.knnShrinkageRaw + "\" (num.shrinkage)");
        check(cmi_slim_create(trainMatrix.n_users, trainMatrix.n_items, conf_.device, 0, &h_), "cmi_slim_create");
        setRatings("cmi_slim_set_ratings");
        check(cmi_slim_build_neighbors(h_, conf_.slimKnn, cmi_knn_measure(conf_.similarity.c_str()), conf_.knnShrinkage, trainMatrix.min_rate,
                                       trainMatrix.max_rate), "cmi_slim_build_neighbors");
        const size_t nu = (size_t)trainMatrix.n_users, ni = (size_t)trainMatrix.n_items, k = (size_t)conf_.numFactors;
        ptr.resize(ni + 1);
        check(cmi_slim_get_neighbors(h_, ptr.data(), nullptr), "cmi_slim_get_neighbors");
        idx.resize((size_t)ptr[ni]);
        check(cmi_slim_get_neighbors(h_, ptr.data(), idx.data()), "cmi_slim_get_neighbors");
        // per column its list positions by ascending neighbour: the walk below meets the cells of a row in column order
        std::vector<int64_t> byRow(idx.size()), cur(ni);
        for (size_t j = 0; j < ni; ++j) {
            std::iota(byRow.begin() + ptr[j], byRow.begin() + ptr[j + 1], ptr[j]);
            std::sort(byRow.begin() + ptr[j], byRow.begin() + ptr[j + 1], [&](int64_t a, int64_t b) { return idx[(size_t)a] < idx[(size_t)b]; });
            cur[j] = ptr[j];
        }
        JavaRandom rnd(conf_.randSeed);
        for (size_t t = 0; t < (nu + ni) * k; ++t) (void)rnd.nextGaussian();
        W.assign(idx.size(), 0.0);
        for (size_t i = 0; i < ni; ++i)
            for (size_t j = 0; j < ni; ++j) {
                const double v = rnd.nextDouble(); // W.init(): uniform(0, 1)
                if (cur[j] < ptr[j + 1] && (size_t)idx[(size_t)byRow[(size_t)cur[j]]] == i) W[(size_t)byRow[(size_t)cur[j]++]] = i == j ? 0.0 : v;
            }
        check(cmi_slim_set_weights(h_, W.data()), "cmi_slim_set_weights");
    }
    void buildModel() override { // SLIM.java:121-181, with its own isConverged (:212-220)
        last_loss = 0;
        for (int iter = 1; iter <= conf_.numIters; ++iter) {
            const int rc = cmi_slim_iterate(h_, conf_.slimL1, conf_.slimL2, &loss);
            if (rc != CMI_E_NUMERIC) check(rc, "cmi_slim_iterate"); // the reference goes on with a NaN loss (its isConverged has no check)
            losses.push_back(loss);
            itersDone = iter;
            const double delta_loss = last_loss - loss;
            last_loss = loss;
            if (conf_.verbose && log_) {
                char buf[256];
                snprintf(buf, sizeof buf, "%s%s iter %d: loss = %.17g, delta_loss = %.17g", algoName.c_str(),
                         fold_ > 0 ? (" fold [" + std::to_string(fold_) + "]").c_str() : "", iter, loss, delta_loss);
                log_(buf);
            }
            if (iter > 1 && delta_loss < 1e-5) break;
        }
        check(cmi_slim_get_weights(h_, W.data()), "cmi_slim_get_weights");
    }
    Measures evalRankings() override { // Recommender.java:668-964 with SLIM.predict
        static const char *names[CMI_RANK_MEASURES] = {"Pre5", "Pre10", "PreN", "Rec5", "Rec10", "RecN", "AUC5", "AUC10", "AUCN",
                                                       "MAP5", "MAP10", "MAPN", "NDCG5", "NDCG10", "NDCGN", "MRR5", "MRR10",
                                                       "MRRN", "D5", "D10", "DN"};
        double out[CMI_RANK_MEASURES];
        int64_t nq = 0;
        check(cmi_slim_eval_rankings(h_, trainMatrix.n(), trainMatrix.u.data(), trainMatrix.j.data(), trainMatrix.ctx.data(),
                                     trainMatrix.r.data(), testMatrix.n(), testMatrix.u.data(), testMatrix.j.data(), testMatrix.ctx.data(),
                                     testMatrix.r.data(), conf_.binThold, conf_.numRecs, conf_.numIgnore,
                                     conf_.evalStrategy == "uc" ? CMI_RANK_UC : CMI_RANK_UCU, out, &nq, nullptr, nullptr, nullptr, nullptr,
                                     nullptr), "cmi_slim_eval_rankings");
        Measures m;
        for (int i = 0; i < CMI_RANK_MEASURES; ++i) m[names[i]] = out[i];
        return m;
    }
    // the reference's saveModel() writes P and Q (IterativeRecommender.java:249-270), which SLIM never trains, and not W: there is
    // nothing of the model to save
    void saveModel() override {}
    std::vector<int64_t> ptr; // the lists and their weights, as cmi_slim_get_neighbors / cmi_slim_get_weights give them
    std::vector<int32_t> idx;
    std::vector<double> W;

  private:
    void predictBounded(double *) override { throw std::runtime_error("SLIM is a top-N recommender: it has no rating evaluation"); }
};

// src/carskit/alg/baseline/ranking/RankALS.java: P and Q by alternating least squares for ranking over the 2-D train matrix, for top-N.
// Parameters: num.factors, num.max.iter, RankALS=-sw on|off.  The constructor sets the static isRankingPred = true (RankALS.java:61),
// so execute() evaluates with evalRankings() whatever item.ranking says, and calls checkBinary() (:63; the driver refuses there).
class RankALS : public PairRecommender<cmi_rankals_handle, cmi_rankals_destroy, cmi_rankals_last_error, cmi_rankals_set_ratings> {
  public:
    RankALS(const RatingData &tr, const RatingData &te, int fold, const Conf &c, Logger log = nullptr)
        : PairRecommender("RankALS", tr, te, fold, c, log) {
        conf_.isRankingPred = true;
    }
    // RankALS.java:67-80: super.initModel() draws P and Q, gaussian (IterativeRecommender.java:235-241; initByNorm stays true); s and
    // sum_s are the library's (cmi_rankals_set_ratings)
    void initModel() override {
        if (!conf_.rankalsSet) // algoOptions = getModelParams("RankALS") is null without the key: algoOptions.isOn throws
            throw std::runtime_error("null (RankALS is not set: RankALS=-sw on|off)");
        JavaRandom rnd(conf_.randSeed);
        const size_t nu = (size_t)trainMatrix.n_users, ni = (size_t)trainMatrix.n_items, k = (size_t)conf_.numFactors;
        P.resize(nu * k);
        Q.resize(ni * k);
        for (double &x : P) x = 0.0 + 0.1 * rnd.nextGaussian();
        for (double &x : Q) x = 0.0 + 0.1 * rnd.nextGaussian();
    }
    void buildModel() override { // RankALS.java:83-206: for (iter = 1; iter < numIters; iter++), no loss, no convergence test
        check(cmi_rankals_create(conf_.numFactors, trainMatrix.n_users, trainMatrix.n_items, conf_.device, 0, &h_), "cmi_rankals_create");
        setRatings("cmi_rankals_set_ratings");
        check(cmi_rankals_set_model(h_, P.data(), Q.data()), "cmi_rankals_set_model");
        for (int iter = 1; iter < conf_.numIters; ++iter) {
            if (conf_.verbose && log_)
                log_(algoName + (fold_ > 0 ? " fold [" + std::to_string(fold_) + "]" : "") + " runs at iter = " + std::to_string(iter) + "/" +
                     std::to_string(conf_.numIters));
            check(cmi_rankals_iterate(h_, conf_.rankalsSw ? 1 : 0), "cmi_rankals_iterate");
            itersDone = iter;
        }
        check(cmi_rankals_get_model(h_, P.data(), Q.data()), "cmi_rankals_get_model");
    }
    Measures evalRankings() override { return evalRankingsWith(cmi_rankals_eval_rankings, "cmi_rankals_eval_rankings"); }
    void saveModel() override { saveFactors(P, Q); }
    std::vector<double> P, Q; // numUsers x numFactors; numItems x numFactors

  private:
    void predictBounded(double *) override { throw std::runtime_error("RankALS is a top-N recommender: it has no rating evaluation"); }
};

// src/carskit/alg/baseline/ranking/BPR.java: P and Q by stochastic gradient steps over numUsers * 100 sampled (u, i, j) triples an
// iteration, for top-N.  Parameters: num.factors, num.max.iter, learn.rate, reg.lambda -u -i.  The constructor sets the static
// isRankingPred = true (BPR.java:42) and initByNorm = false (:43).  The triples come from happy.coding's static Randoms stream, which
// the first recommender's constructor seeds with --rand-seed (Recommender.java:194-234, after the splitter's draws): conf.bprStream
// starts at the seed's state and carries the stream from fold to fold.
class BPR : public PairRecommender<cmi_bpr_handle, cmi_bpr_destroy, cmi_bpr_last_error, cmi_bpr_set_ratings> {
  public:
    BPR(const RatingData &tr, const RatingData &te, int fold, const Conf &c, Logger log = nullptr)
        : PairRecommender("BPR", tr, te, fold, c, log) {
        conf_.isRankingPred = true;
    }
    // IterativeRecommender.java:235-241 with initByNorm = false: P.init(), Q.init() = Randoms.uniform() per cell, row by row
    void initModel() override {
        JavaRandom rnd(conf_.randSeed);
        P.resize((size_t)trainMatrix.n_users * (size_t)conf_.numFactors);
        Q.resize((size_t)trainMatrix.n_items * (size_t)conf_.numFactors);
        for (double &x : P) x = rnd.nextDouble();
        for (double &x : Q) x = rnd.nextDouble();
    }
    void buildModel() override { // BPR.java:55-109
        // the loss as the reference's one chain (6 ns a term on an MI355X, profiles/bpr_bench.json) up to 2^18 terms, under 2 ms;
        // else the fixed tree
        const bool small = (int64_t)trainMatrix.n_users * 100 * (conf_.numFactors + 1) <= ((int64_t)1 << 18);
        check(cmi_bpr_create(conf_.numFactors, trainMatrix.n_users, trainMatrix.n_items, conf_.device, small ? CMI_BPR_FLAG_STRICT : 0u, &h_),
              "cmi_bpr_create");
        setRatings("cmi_bpr_set_ratings");
        check(cmi_bpr_set_model(h_, P.data(), Q.data()), "cmi_bpr_set_model");
        const int64_t start = conf_.bprStream ? *conf_.bprStream : (int64_t)cmi::java_lcg_scramble(conf_.randSeed);
        check(cmi_bpr_set_random_state(h_, start), "cmi_bpr_set_random_state");
        for (int iter = 1; iter <= conf_.numIters; ++iter) {
            const int rc = cmi_bpr_iterate(h_, lRate, conf_.regU, conf_.regI, &loss);
            if (rc != CMI_E_NUMERIC) check(rc, "cmi_bpr_iterate"); // a NaN / Inf loss: isConverged reports it, as in the reference
            itersDone = iter;
            if (isConverged(iter)) break;
        }
        if (conf_.bprStream) check(cmi_bpr_get_random_state(h_, conf_.bprStream.get()), "cmi_bpr_get_random_state");
        check(cmi_bpr_get_model(h_, P.data(), Q.data()), "cmi_bpr_get_model");
    }
    Measures evalRankings() override { return evalRankingsWith(cmi_bpr_eval_rankings, "cmi_bpr_eval_rankings"); }
    void saveModel() override { saveFactors(P, Q); }
    std::vector<double> P, Q; // numUsers x numFactors; numItems x numFactors

  private:
    void predictBounded(double *) override { throw std::runtime_error("BPR is a top-N recommender: it has no rating evaluation"); }
};

// src/carskit/alg/baseline/ranking/LRMF.java: P and Q by list-wise gradient steps over every stored cell of the 2-D train matrix, for
// top-N.  Parameters: num.factors, num.max.iter, learn.rate, reg.lambda -u -i.  The constructor sets the static isRankingPred = true
// (LRMF.java:49) and initByNorm = false (:50); userExp (:55-67) is the library's (cmi_lrmf_set_ratings).
class LRMF : public PairRecommender<cmi_lrmf_handle, cmi_lrmf_destroy, cmi_lrmf_last_error, cmi_lrmf_set_ratings> {
  public:
    LRMF(const RatingData &tr, const RatingData &te, int fold, const Conf &c, Logger log = nullptr)
        : PairRecommender("LRMF", tr, te, fold, c, log) {
        conf_.isRankingPred = true;
    }
    // IterativeRecommender.java:239-245 with initByNorm = false: P.init(), Q.init() = Randoms.uniform() per cell, row by row
    void initModel() override {
        JavaRandom rnd(conf_.randSeed);
        P.resize((size_t)trainMatrix.n_users * (size_t)conf_.numFactors);
        Q.resize((size_t)trainMatrix.n_items * (size_t)conf_.numFactors);
        for (double &x : P) x = rnd.nextDouble();
        for (double &x : Q) x = rnd.nextDouble();
    }
    void buildModel() override { // LRMF.java:70-110
        // the loss as the reference's one chain up to 2^18 terms, as BPR; else the fixed tree.  The 2-D matrix has at most as many
        // cells as the train set has tuples
        const bool small = (int64_t)trainMatrix.n() * (conf_.numFactors + 1) <= ((int64_t)1 << 18);
        check(cmi_lrmf_create(conf_.numFactors, trainMatrix.n_users, trainMatrix.n_items, conf_.device, small ? CMI_LRMF_FLAG_STRICT : 0u, &h_),
              "cmi_lrmf_create");
        setRatings("cmi_lrmf_set_ratings");
        check(cmi_lrmf_set_model(h_, P.data(), Q.data()), "cmi_lrmf_set_model");
        for (int iter = 1; iter <= conf_.numIters; ++iter) {
            const int rc = cmi_lrmf_iterate(h_, lRate, conf_.regU, conf_.regI, &loss);
            if (rc != CMI_E_NUMERIC) check(rc, "cmi_lrmf_iterate"); // a NaN / Inf loss: isConverged reports it, as in the reference
            itersDone = iter;
            if (isConverged(iter)) break;
        }
        check(cmi_lrmf_get_model(h_, P.data(), Q.data()), "cmi_lrmf_get_model");
    }
    Measures evalRankings() override { return evalRankingsWith(cmi_lrmf_eval_rankings, "cmi_lrmf_eval_rankings"); }
    void saveModel() override { saveFactors(P, Q); }
    std::vector<double> P, Q; // numUsers x numFactors; numItems x numFactors

  private:
    void predictBounded(double *) override { throw std::runtime_error("LRMF is a top-N recommender: it has no rating evaluation"); }
};

// src/carskit/alg/baseline/ranking/RankSGD.java: P and Q by one stochastic gradient step per rated cell against an item drawn by
// popularity, for top-N.  Parameters: num.factors, num.max.iter, learn.rate; RankSGD=-numrates size|reference (see Conf).  The
// constructor sets the static isRankingPred = true (RankSGD.java:56) and calls checkBinary() (:58; the driver refuses there);
// initByNorm stays true.  The draws come from happy.coding's static Randoms stream, as BPR's do: conf.bprStream.
class RankSGD : public PairRecommender<cmi_ranksgd_handle, cmi_ranksgd_destroy, cmi_ranksgd_last_error, cmi_ranksgd_set_ratings> {
  public:
    RankSGD(const RatingData &tr, const RatingData &te, int fold, const Conf &c, Logger log = nullptr)
        : PairRecommender("RankSGD", tr, te, fold, c, log) {
        conf_.isRankingPred = true;
    }
    // RankSGD.java:62-63: super.initModel() draws P and Q, gaussian (IterativeRecommender.java:235-241); the item list (:65-75) is the
    // library's (cmi_ranksgd_set_ratings)
    void initModel() override {
        JavaRandom rnd(conf_.randSeed);
        P.resize((size_t)trainMatrix.n_users * (size_t)conf_.numFactors);
        Q.resize((size_t)trainMatrix.n_items * (size_t)conf_.numFactors);
        for (double &x : P) x = 0.0 + 0.1 * rnd.nextGaussian();
        for (double &x : Q) x = 0.0 + 0.1 * rnd.nextGaussian();
    }
    void buildModel() override { // RankSGD.java:79-141
        // the loss as the reference's one chain up to 2^18 terms, as BPR; else the fixed tree
        const bool small = (int64_t)trainMatrix.n() <= ((int64_t)1 << 18);
        const unsigned flags = (small ? CMI_RANKSGD_FLAG_STRICT : 0u) | (conf_.ranksgdNumRatesSize ? CMI_RANKSGD_FLAG_NUM_RATES_SIZE : 0u);
        check(cmi_ranksgd_create(conf_.numFactors, trainMatrix.n_users, trainMatrix.n_items, conf_.device, flags, &h_), "cmi_ranksgd_create");
        setRatings("cmi_ranksgd_set_ratings");
        check(cmi_ranksgd_set_model(h_, P.data(), Q.data()), "cmi_ranksgd_set_model");
        const int64_t start = conf_.bprStream ? *conf_.bprStream : (int64_t)cmi::java_lcg_scramble(conf_.randSeed);
        check(cmi_ranksgd_set_random_state(h_, start), "cmi_ranksgd_set_random_state");
        for (int iter = 1; iter <= conf_.numIters; ++iter) {
            const int rc = cmi_ranksgd_iterate(h_, lRate, &loss);
            if (rc != CMI_E_NUMERIC) check(rc, "cmi_ranksgd_iterate"); // a NaN / Inf loss: isConverged reports it, as in the reference
            itersDone = iter;
            if (isConverged(iter)) break;
        }
        if (conf_.bprStream) check(cmi_ranksgd_get_random_state(h_, conf_.bprStream.get()), "cmi_ranksgd_get_random_state");
        check(cmi_ranksgd_get_model(h_, P.data(), Q.data()), "cmi_ranksgd_get_model");
    }
    Measures evalRankings() override { return evalRankingsWith(cmi_ranksgd_eval_rankings, "cmi_ranksgd_eval_rankings"); }
    void saveModel() override { saveFactors(P, Q); }
    std::vector<double> P, Q; // numUsers x numFactors; numItems x numFactors

  private:
    void predictBounded(double *) override { throw std::runtime_error("RankSGD is a top-N recommender: it has no rating evaluation"); }
};

// src/carskit/alg/cars/adaptation/independent/CPTF.java on src/carskit/generic/TensorRecommender.java: one factor matrix per
// dimension of the rating tensor (user, item, one per context dimension).  Parameters: num.factors, num.max.iter, learn.rate,
// reg.lambda (its main parameter); CPTF=-keys reference|indexof (see Conf).  The tensor, the fold's train and test tensors and
// getKeys' table are the library's (cmi_cptf_tensor_build: DataDAO.java:423-481, TensorRecommender.java:62-84, :189-205) over
// rateMatrix = the fold's train and test tuples together, in rateMatrix order (pair, then context).
class CPTF : public IterativeRecommender {
  public:
    CPTF(const RatingData &tr, const RatingData &te, int fold, const Conf &c, Logger log = nullptr)
        : IterativeRecommender(-1, "CPTF", true, tr, te, fold, c, log) {}
    ~CPTF() override {
        if (t_) cmi_cptf_destroy(t_);
    }
    // TensorRecommender.java:53-84 (the tensors), then CPTF.java:46-55: M[d].init(1, 0.1) per dimension in d order, row by row
    void initModel() override {
        buildTensors();
        JavaRandom rnd(conf_.randSeed);
        size_t total = 0;
        for (int32_t d : dims) total += (size_t)d * (size_t)conf_.numFactors;
        M.resize(total);
        for (double &x : M) x = 1.0 + 0.1 * rnd.nextGaussian();
    }
    void buildModel() override { // CPTF.java:75-115
        // pred and the loss as the reference's chains up to 2^18 loss terms; else the fixed tree and the loss by parts
        const int64_t terms = (int64_t)train_vals.size() * (1 + (int64_t)conf_.numFactors * (int64_t)dims.size());
        check(cmi_cptf_create(conf_.numFactors, (int)dims.size(), dims.data(), conf_.device, terms <= ((int64_t)1 << 18) ? CMI_CPTF_FLAG_STRICT : 0u,
                              &t_), "cmi_cptf_create");
        check(cmi_cptf_set_entries(t_, (int64_t)train_vals.size(), train_keys.data(), train_vals.data()), "cmi_cptf_set_entries");
        check(cmi_cptf_set_model(t_, M.data()), "cmi_cptf_set_model");
        for (int iter = 1; iter <= conf_.numIters; ++iter) {
            const int rc = cmi_cptf_iterate(t_, lRate, conf_.reg, &loss);
            if (rc != CMI_E_NUMERIC) check(rc, "cmi_cptf_iterate"); // a NaN / Inf loss: isConverged reports it, as in the reference
            itersDone = iter;
            if (isConverged(iter)) break;
        }
        check(cmi_cptf_get_model(t_, M.data()), "cmi_cptf_get_model");
    }
    // TensorRecommender.java:86-164 (view "all"): the bounded predict(keys) of every entry of the TEST TENSOR in iterator order
    Measures evalRatings() override {
        const double lo = trainMatrix.min_rate, hi = trainMatrix.max_rate;
        std::vector<double> pred(test_vals.size());
        check(cmi_cptf_predict_batch(t_, (int64_t)pred.size(), test_keys.data(), 1, lo, hi, pred.data()), "cmi_cptf_predict_batch");
        double sa = 0, ss = 0, sra = 0, srs = 0;
        int64_t n = 0, pe = 0;
        for (size_t t = 0; t < pred.size(); ++t) {
            if (std::isnan(pred[t])) continue;
            const double rp = std::floor(pred[t] / lo + 0.5) * lo; // Math.round
            const double e = std::fabs(test_vals[t] - pred[t]), re = std::fabs(test_vals[t] - rp);
            sa += e, ss += e * e, sra += re, srs += re * re;
            ++n;
            if (re > 1e-5) ++pe;
        }
        const double mae = sa / (double)n;
        return Measures{{"MAE", mae}, {"RMSE", std::sqrt(ss / (double)n)}, {"NMAE", mae / (hi - lo)}, {"rMAE", sra / (double)n},
                        {"rRMSE", std::sqrt(srs / (double)n)}, {"MPE", ((double)pe + 0.0) / (double)n}};
    }
    // Recommender.java:668-964 with ranking(u, j, c) = CPTF.predict(u, j, c): getKeys' keys, clamped (CPTF.java:119-139)
    Measures evalRankings() override {
        static const char *names[CMI_RANK_MEASURES] = {"Pre5", "Pre10", "PreN", "Rec5", "Rec10", "RecN", "AUC5", "AUC10", "AUCN",
                                                       "MAP5", "MAP10", "MAPN", "NDCG5", "NDCG10", "NDCGN", "MRR5", "MRR10",
                                                       "MRRN", "D5", "D10", "DN"};
        check(cmi_cptf_set_context_keys(t_, (int32_t)(trainMatrix.ctx_ptr.size() - 1), ctx_keys.data()), "cmi_cptf_set_context_keys");
        check(cmi_cptf_set_rating_range(t_, trainMatrix.min_rate, trainMatrix.max_rate), "cmi_cptf_set_rating_range");
        double out[CMI_RANK_MEASURES];
        int64_t nq = 0;
        check(cmi_cptf_eval_rankings(t_, trainMatrix.n(), trainMatrix.u.data(), trainMatrix.j.data(), trainMatrix.ctx.data(),
                                     trainMatrix.r.data(), testMatrix.n(), testMatrix.u.data(), testMatrix.j.data(), testMatrix.ctx.data(),
                                     testMatrix.r.data(), conf_.binThold, conf_.numRecs, conf_.numIgnore,
                                     conf_.evalStrategy == "uc" ? CMI_RANK_UC : CMI_RANK_UCU, out, &nq, nullptr, nullptr, nullptr, nullptr,
                                     nullptr), "cmi_cptf_eval_rankings");
        Measures m;
        for (int i = 0; i < CMI_RANK_MEASURES; ++i) m[names[i]] = out[i];
        return m;
    }
    void saveModel() override {
        if (log_) log_("--save-model: not available for " + algoName);
    }
    std::vector<int32_t> dims, train_keys, test_keys, ctx_keys; // the tensors' sizes, entries in iterator order, getKeys per context
    std::vector<double> train_vals, test_vals, M;               // M[0] .. M[n_dims - 1] concatenated, each dims[d] x numFactors

  private:
    void check(int rc, const char *what) { // (a failed create, and the tensor build, leave t_ null: the thread's message)
        if (rc != CMI_OK) throw std::runtime_error(std::string(what) + ": " + cmi_cptf_last_error(t_));
    }
    void buildTensors() {
        if (trainMatrix.pair.size() != trainMatrix.r.size() || testMatrix.pair.size() != testMatrix.r.size())
            throw std::runtime_error("CPTF: the rating tensor is built from one rating matrix; a separate test set has no rows in it");
        // rateMatrix: the train and test tuples together in its iteration order (row = pair, then column = context)
        struct Cell { int32_t pair, ctx; double r; };
        std::vector<Cell> cells;
        int32_t n_pairs = 0;
        for (const RatingData *d : {&trainMatrix, &testMatrix})
            for (size_t t = 0; t < d->r.size(); ++t) {
                cells.push_back({d->pair[t], d->ctx[t], d->r[t]});
                n_pairs = std::max(n_pairs, d->pair[t] + 1);
            }
        std::sort(cells.begin(), cells.end(), [](const Cell &a, const Cell &b) { return a.pair != b.pair ? a.pair < b.pair : a.ctx < b.ctx; });
        std::vector<int32_t> pair(cells.size()), ctx(cells.size()), pu((size_t)n_pairs, 0), pi((size_t)n_pairs, 0);
        std::vector<double> rate(cells.size());
        for (size_t t = 0; t < cells.size(); ++t) pair[t] = cells[t].pair, ctx[t] = cells[t].ctx, rate[t] = cells[t].r;
        for (const RatingData *d : {&trainMatrix, &testMatrix})
            for (size_t t = 0; t < d->r.size(); ++t) pu[(size_t)d->pair[t]] = d->u[t], pi[(size_t)d->pair[t]] = d->j[t];
        const size_t n = cells.size(), n_ctx = trainMatrix.ctx_ptr.size() - 1, w = 2 + (size_t)std::max(1, trainMatrix.n_dims);
        int32_t nd = 0;
        int64_t n_train = 0, n_test = 0;
        std::vector<int32_t> d10(16), lptr(16), lst(trainMatrix.cond_dim.size() + 1), keys(n * w + 1);
        std::vector<double> vals(n + 1);
        train_keys.assign(n * w + 1, 0), test_keys.assign(n * w + 1, 0), train_vals.assign(n + 1, 0.0), test_vals.assign(n + 1, 0.0);
        ctx_keys.assign(n_ctx * w + 1, 0);
        check(cmi_cptf_tensor_build((int64_t)n, pair.data(), ctx.data(), rate.data(), n_pairs, pu.data(), pi.data(), (int32_t)n_ctx,
                                    trainMatrix.ctx_ptr.data(), trainMatrix.ctx_conds.data(), (int32_t)trainMatrix.cond_dim.size(),
                                    trainMatrix.cond_dim.data(), testMatrix.n(), testMatrix.pair.data(),
                                    conf_.cptfKeysIndexOf ? CMI_CPTF_FLAG_KEYS_INDEXOF : 0u, &nd, d10.data(), lptr.data(), lst.data(), keys.data(),
                                    vals.data(), &n_train, train_keys.data(), train_vals.data(), &n_test, test_keys.data(), test_vals.data(),
                                    ctx_keys.data()), "cmi_cptf_tensor_build");
        dims.assign(d10.begin(), d10.begin() + nd);
        train_keys.resize((size_t)n_train * (size_t)nd), train_vals.resize((size_t)n_train);
        test_keys.resize((size_t)n_test * (size_t)nd), test_vals.resize((size_t)n_test);
        ctx_keys.resize(n_ctx * (size_t)(nd - 2));
    }
    cmi_cptf_handle t_ = nullptr;
};

// the factory switch of CARSKit.getRecommender (src/carskit/main/CARSKit.java:461-469,700-712,742), lower-cased names
inline std::unique_ptr<IterativeRecommender> getRecommender(const std::string &name, const RatingData &tr, const RatingData &te,
                                                            int fold, const Conf &c, Logger log) {
    const std::string n = lower(name);
    if (n == "biasedmf") return std::unique_ptr<IterativeRecommender>(new BiasedMF(tr, te, fold, c, log));
    if (n == "pmf") return std::unique_ptr<IterativeRecommender>(new PMF(tr, te, fold, c, log));
    if (n == "camf_c") return std::unique_ptr<IterativeRecommender>(new CAMF_C(tr, te, fold, c, log));
    if (n == "camf_ci") return std::unique_ptr<IterativeRecommender>(new CAMF_CI(tr, te, fold, c, log));
    if (n == "camf_cu") return std::unique_ptr<IterativeRecommender>(new CAMF_CU(tr, te, fold, c, log));
    if (n == "camf_cuci") return std::unique_ptr<IterativeRecommender>(new CAMF_CUCI(tr, te, fold, c, log));
    if (n == "fm") return std::unique_ptr<IterativeRecommender>(new FM(tr, te, fold, c, log));
    if (n == "svd++") return std::unique_ptr<IterativeRecommender>(new SVDPlusPlus(tr, te, fold, c, log));   // CARSKit.java:469
    if (n == "camf_ics") return std::unique_ptr<IterativeRecommender>(new CAMF_ICS(tr, te, fold, c, log));   // CARSKit.java:708
    if (n == "camf_lcs") return std::unique_ptr<IterativeRecommender>(new CAMF_LCS(tr, te, fold, c, log));   // CARSKit.java:710
    if (n == "camf_mcs") return std::unique_ptr<IterativeRecommender>(new CAMF_MCS(tr, te, fold, c, log));   // CARSKit.java:712
    if (n == "slim") return std::unique_ptr<IterativeRecommender>(new SLIM(tr, te, fold, c, log));           // CARSKit.java:471-472
    if (n == "itemknn") return std::unique_ptr<IterativeRecommender>(new ItemKNN(tr, te, fold, c, log));
    if (n == "userknn") return std::unique_ptr<IterativeRecommender>(new UserKNN(tr, te, fold, c, log));
    if (n == "slopeone") return std::unique_ptr<IterativeRecommender>(new SlopeOne(tr, te, fold, c, log));
    if (n == "nmf") return std::unique_ptr<IterativeRecommender>(new NMF(tr, te, fold, c, log));             // CARSKit.java:467
    if (n == "bpmf") return std::unique_ptr<IterativeRecommender>(new BPMF(tr, te, fold, c, log));           // CARSKit.java:465-466
    if (n == "rankals") return std::unique_ptr<IterativeRecommender>(new RankALS(tr, te, fold, c, log));   // CARSKit.java:477-478
    if (n == "bpr") return std::unique_ptr<IterativeRecommender>(new BPR(tr, te, fold, c, log));
    if (n == "lrmf") return std::unique_ptr<IterativeRecommender>(new LRMF(tr, te, fold, c, log));
    if (n == "cptf") return std::unique_ptr<IterativeRecommender>(new CPTF(tr, te, fold, c, log));         // CARSKit.java:693-697
    if (n == "ranksgd") return std::unique_ptr<IterativeRecommender>(new RankSGD(tr, te, fold, c, log));   // CARSKit.java:479-480
    throw std::runtime_error("recommender '" + name + "' is not on the accelerated path (biasedmf, pmf, svd++, camf_c, camf_ci, camf_cu, camf_cuci, camf_ics, camf_lcs, camf_mcs, fm, cptf, bpmf, slim, rankals, bpr, lrmf, ranksgd, itemknn, userknn, slopeone, nmf)");
}

} // namespace carskit
