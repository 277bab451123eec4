// ranksgd_kernels.hpp -- device side of RankSGD (ranksgd_kernels.hip), launched by ranksgd_api.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "bpr_kernels.hpp"
#include "java_math.hpp"

namespace cmi {

// ---- the tries ----------------------------------------------------------------------------------------------------------------------
// out[t] = ranksgd_try from the state 2t draws after state0 over the list (item / cum, n_table entries), t < n_tries
hipError_t ranksgd_launch_tries(uint64_t state0, const JavaLcgJump &jump, const int32_t *item, const double *cum, int32_t n_table,
                                int64_t n_tries, int32_t *out, hipStream_t s);

// ---- the epoch ----------------------------------------------------------------------------------------------------------------------
struct RanksgdEpoch {
    int k = 0;
    double *P = nullptr, *Q = nullptr;
    const int32_t *u = nullptr, *i = nullptr, *j = nullptr; // the samples by cell
    const double *r = nullptr;                              // rui
    const int32_t *order = nullptr;     // samples sorted by level, ascending inside a level
    const int32_t *level_ptr = nullptr; // n_levels + 1 offsets into order
    double *slots = nullptr;            // one per sample: e * e
    double lrate = 0.0;
};
// as bpr_launch_level / bpr_launch_run: a level of any width (a 16-lane group per sample, BPR_WG_SAMPLES a workgroup), or a run of
// levels no wider than BPR_WG_SAMPLES each in one workgroup with a barrier between them
hipError_t ranksgd_launch_level(const RanksgdEpoch &a, int32_t begin, int32_t end, hipStream_t s);
hipError_t ranksgd_launch_run(const RanksgdEpoch &a, int32_t l0, int32_t l1, hipStream_t s);

} // namespace cmi
