// bpr_kernels.hpp -- device side of BPR (bpr_kernels.hip), launched by bpr_api.cpp, and the one definition of a sample's draws that
// the host sampler and the device sampler share.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <vector>

#include "java_math.hpp"

namespace cmi {

constexpr int BPR_MAX_K = 128;       // factors: a 16-lane group holds a row in 8 registers per lane
constexpr int BPR_GROUP = 16;        // lanes per sample
constexpr int BPR_BLOCK = 256;       // threads per workgroup of the epoch
constexpr int BPR_WG_SAMPLES = BPR_BLOCK / BPR_GROUP; // samples a workgroup updates at once: a wider level is launched alone
constexpr int BPR_DRAW_CAP = 255;    // draws one sample may consume on the device (its length is stored in a byte); more -> overflow
constexpr int BPR_RANK_BLOCK = 1024; // stream positions per ranking block (and threads per workgroup of the ranking kernel)
constexpr int BPR_RANK_ENTRIES = 256; // entry points kept per ranking block: a sample ends at most BPR_DRAW_CAP past a block's border
constexpr int BPR_LOSS_PARTS = 256;  // partial sums (workgroups) of the default loss
constexpr uint16_t BPR_OVERFLOW = 0xFFFF;

// librec SparseVector.contains(key) of a row built by SparseMatrix.row(): Arrays.binarySearch over the WHOLE index array, whose
// capacity is the next power of two >= count with a zero tail, so an entry of the upper half can be missed (pair_contains_flags)
CMI_JM_HD inline bool bpr_contains(const int32_t *idx, int32_t cnt, int32_t key) {
    int32_t cap = 1;
    while (cap < cnt) cap <<= 1;
    int32_t low = 0, high = (cnt == 0 ? 0 : cap) - 1;
    while (low <= high) {
        const int32_t mid = (int32_t)((uint32_t)(low + high) >> 1);
        const int32_t v = mid < cnt ? idx[mid] : 0;
        if (v < key) low = mid + 1;
        else if (v > key) high = mid - 1;
        else return true;
    }
    return false;
}

// BPR.java:65-80: one (u, i, j) from the stream.  rptr / ridx: the rows of train without their zero-valued cells (what
// userCache.get(u) holds: getCount() == getIndex().length).  false: the sample would take a draw past `cap`
CMI_JM_HD inline bool bpr_draw(JavaStream &rng, int32_t n_users, int32_t n_items, const int32_t *rptr, const int32_t *ridx, int64_t cap,
                               int32_t &u, int32_t &i, int32_t &j) {
    for (;;) {
        u = rng.nextInt(n_users, cap);
        if (u < 0) return false;
        const int32_t b0 = rptr[u], cnt = rptr[u + 1] - b0;
        if (cnt == 0) continue;
        const int32_t t = rng.nextInt(cnt, cap);
        if (t < 0) return false;
        i = ridx[b0 + t];
        do {
            j = rng.nextInt(n_items, cap);
            if (j < 0) return false;
        } while (bpr_contains(ridx + b0, cnt, j));
        return true;
    }
}

// ---- the sampler --------------------------------------------------------------------------------------------------------------------
struct BprSampler {
    int32_t n_users = 0, n_items = 0;
    const int32_t *rptr = nullptr, *ridx = nullptr;
    uint64_t state0 = 0;   // stream state before the iteration's first draw
    int64_t L = 0, S = 0;  // stream positions speculated on; samples wanted
    int64_t n_blocks = 0;  // ceil(L / BPR_RANK_BLOCK)
    uint8_t *len = nullptr;      // L: draws the sample starting at position d consumes, 0 = overflow (more than BPR_DRAW_CAP)
    // n_blocks x BPR_RANK_ENTRIES: from entry e of block b, where the list leaves the block (offset past its start; BPR_OVERFLOW: it
    // meets an overflow or the end of L) and how many samples it holds before that
    uint16_t *exit_off = nullptr, *cnt = nullptr;
    int32_t *entry = nullptr;    // n_blocks: the list's entry offset into block b, -1 past the list's end
    int64_t *base = nullptr;     // n_blocks: samples of the list before block b
    int64_t *result = nullptr;   // [0] samples found (>= S: enough), [1] draws consumed by the first S samples
    int64_t *pos = nullptr;      // S: stream position of sample s
    int32_t *u = nullptr, *i = nullptr, *j = nullptr; // S
};
// (b) the length of the sample that would start at every position, (c) the ranking (per block, over blocks, expansion).
// result[0] < S afterwards: the list left L or met an overflow -- the caller samples on the host
hipError_t bpr_launch_sampler(const BprSampler &a, const JavaLcgJump &jump, hipStream_t s);
// once result[0] >= S has been read: u, i, j of the first S nodes and result[1]
hipError_t bpr_launch_emit(const BprSampler &a, const JavaLcgJump &jump, hipStream_t s);

// ---- the epoch ----------------------------------------------------------------------------------------------------------------------
struct BprEpoch {
    int k = 0;
    double *P = nullptr, *Q = nullptr;
    const int32_t *u = nullptr, *i = nullptr, *j = nullptr; // the triples by sample
    const int32_t *order = nullptr;     // samples sorted by level, ascending inside a level
    const int32_t *level_ptr = nullptr; // n_levels + 1 offsets into order
    double *slots = nullptr;            // S x (k + 1): -log(g(xuij)) and the k regularisation terms of sample s
    double lrate = 0.0, regU = 0.0, regI = 0.0;
};
// the levels [l0, l1): l1 == l0 + 1 and any width (a grid of workgroups), or a run of levels no wider than BPR_WG_SAMPLES each
// (one workgroup, a barrier between levels).  begin / end: offsets into order of a level launched alone
hipError_t bpr_launch_level(const BprEpoch &a, int32_t begin, int32_t end, hipStream_t s);
hipError_t bpr_launch_run(const BprEpoch &a, int32_t l0, int32_t l1, hipStream_t s);
// the launch list of a level schedule: a level wider than wg_samples on its own (level(begin, end): offsets into order), a run of
// consecutive narrower levels in one launch of one workgroup (run(l0, l1)).  sched: levels, levels alone, runs, the widest level
template <class Level, class Run>
inline hipError_t launch_triple_levels(const std::vector<int32_t> &level_ptr, int32_t n_levels, int32_t wg_samples, Level &&level, Run &&run,
                                       int64_t sched[4]) {
    int64_t alone = 0, runs = 0, widest = 0;
    for (int32_t l = 0; l < n_levels;) {
        const int32_t w = level_ptr[(size_t)l + 1] - level_ptr[(size_t)l];
        widest = std::max<int64_t>(widest, w);
        if (w > wg_samples) {
            if (hipError_t e = level(level_ptr[(size_t)l], level_ptr[(size_t)l + 1])) return e;
            ++alone, ++l;
            continue;
        }
        int32_t e = l + 1;
        for (; e < n_levels && level_ptr[(size_t)e + 1] - level_ptr[(size_t)e] <= wg_samples; ++e)
            widest = std::max<int64_t>(widest, level_ptr[(size_t)e + 1] - level_ptr[(size_t)e]);
        if (hipError_t err = run(l, e)) return err;
        ++runs, l = e;
    }
    sched[0] = n_levels, sched[1] = alone, sched[2] = runs, sched[3] = widest;
    return hipSuccess;
}

// loss: strict = one chain over the n slots in order (the reference's sum bit for bit); else a fixed tree (parts: BPR_LOSS_PARTS doubles)
hipError_t bpr_launch_loss(const double *slots, int64_t n, bool strict, double *parts, double *out, hipStream_t s);

// ---- probes -------------------------------------------------------------------------------------------------------------------------
// val[d], used[d]: nextInt(bound) started d draws after `state` and the draws it took, d < n
hipError_t bpr_launch_next_ints(uint64_t state, int32_t bound, int64_t n, const JavaLcgJump &jump, int32_t *val, int32_t *used,
                                hipStream_t s);
hipError_t bpr_launch_exp_log(int64_t n, const double *x, double *e, double *l, hipStream_t s);

} // namespace cmi
