// pair_walk.hpp -- the device side that the pair-co-occurrence models share (ItemKNN / UserKNN: knn_kernels.hip, SlopeOne:
// slopeone_kernels.hip): the CSR they read and the walk over the common entries of an anchor row and its partners.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace cmi {

// one side of the 2-D train matrix, CSR, ascending: the compared rows ("entities": items for ItemKNN and SlopeOne's build, users for
// UserKNN) over the contracted index, or the lists a prediction takes its candidates from
struct PairCsr {
    const int32_t *ptr = nullptr; // n + 1
    const int32_t *idx = nullptr;
    const double *val = nullptr;
    // ItemKNN / UserKNN rows only: does librec's SparseVector.contains find the entry in its own row?  contains() binary-searches the
    // whole index array, which set() grows to the next power of two with a zero tail, so some entries of the upper half are never
    // found.  nullptr: every entry counts.
    const uint8_t *ok = nullptr;
};

constexpr int PAIR_TILE = 4096; // contracted indices per LDS tile of the anchor's vector: 48 KiB of LDS with the tags, 3 workgroups a CU
constexpr int PAIR_BUILD_BLOCK = 256;

// which of the anchor's entries enter a tile
enum class PairOk {
    ALL,    // every entry; R.ok is never loaded
    FOUND,  // the entries with R.ok set (correlation(): iv.contains(idx) misses the others)
    BESIDE, // every entry, its R.ok byte beside it in T.ok (cos-binary)
};

// the anchor's tile in LDS.  An entry is valid when its tag equals the current generation, so a tile is never cleared.
template <PairOk F>
struct PairTile {
    double lv[PAIR_TILE];
    int32_t tag[PAIR_TILE];
    uint8_t ok[F == PairOk::BESIDE ? PAIR_TILE : 1];
    int32_t s_qb;
};

// before the first sweep of a workgroup: no tag is a generation.  `gen` starts at 0 and runs on through every sweep of the workgroup.
template <PairOk F>
__device__ __forceinline__ void pair_tile_init(PairTile<F> &T) {
    for (int i = threadIdx.x; i < PAIR_TILE; i += blockDim.x) T.tag[i] = -1;
}

// One sweep of the anchor's tiles, by the whole workgroup.  The anchor's entries [a0, a1) are scattered into LDS one tile of PAIR_TILE
// contracted indices at a time (only tiles where the anchor has entries: no common entry lies elsewhere); a lane with a partner (act)
// walks its partner's entries [b0, b1) of that tile in ascending order and probes the tile, so visit(va, vb, slot, cur) meets the
// common entries in ascending order: va the anchor's value, vb = R.val[cur] the partner's, slot the entry's place in T.  The visitor's
// running sums stay in the lane's registers across tiles.
template <PairOk F, class Visit>
__device__ __forceinline__ void pair_sweep(const PairCsr &R, int a0, int a1, int b0, int b1, bool act, PairTile<F> &T, int &gen,
                                           Visit &&visit) {
    int cur = b0;
    for (int qa = a0; qa < a1;) {
        const int lo = R.idx[qa] / PAIR_TILE * PAIR_TILE, hi = lo + PAIR_TILE;
        __syncthreads(); // the previous tile's readers are done
        if (threadIdx.x == 0) { // the anchor's entries of this tile: [qa, qb)
            int l = qa, r = a1;
            while (l < r) {
                const int m = (l + r) >> 1;
                if (R.idx[m] < hi) l = m + 1;
                else r = m;
            }
            T.s_qb = l;
        }
        __syncthreads();
        const int qb = T.s_qb;
        for (int q = qa + (int)threadIdx.x; q < qb; q += blockDim.x) {
            if constexpr (F == PairOk::FOUND)
                if (!R.ok[q]) continue;
            T.lv[R.idx[q] - lo] = R.val[q];
            T.tag[R.idx[q] - lo] = gen;
            if constexpr (F == PairOk::BESIDE) T.ok[R.idx[q] - lo] = R.ok[q];
        }
        __syncthreads();
        if (act) {
            int l = cur, r = b1; // skip the partner's entries below the tile
            while (l < r) {
                const int m = (l + r) >> 1;
                if (R.idx[m] < lo) l = m + 1;
                else r = m;
            }
            for (cur = l; cur < b1; ++cur) {
                const int x = R.idx[cur];
                if (x >= hi) break;
                if (T.tag[x - lo] != gen) continue;
                visit(T.lv[x - lo], R.val[cur], x - lo, cur);
            }
        }
        ++gen;
        qa = qb;
    }
}

} // namespace cmi
