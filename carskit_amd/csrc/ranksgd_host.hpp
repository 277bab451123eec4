// ranksgd_host.hpp -- what RankSGD (carskit/alg/baseline/ranking/RankSGD.java) prepares and decides on the host: the item list and its
// running sums (RankSGD.java:66-75), one try of the draw (:97-107, shared with the device), the sequential walk over the cells that
// consumes tries (:85-112), the reservation for the device tries and the matrices that are refused.  No HIP calls.
//
// numRates.  Recommender.java:141 declares the field and no file of the reference assigns it, so :71 divides by 0 there: every item
// with a cell has prob = +Infinity, the list keeps the HashMap's iteration order, the first running sum is +Infinity and every try
// returns the list's first item.  `num_rates` below is that divisor: 0 is the reference as it stands, the number of non-zero cells is
// LibRec's numRates = trainMatrix.size() (CMI_RANKSGD_FLAG_NUM_RATES_SIZE).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

#include "bpr_kernels.hpp" // bpr_contains
#include "java_hash.hpp"
#include "java_math.hpp"

namespace cmi {

struct RanksgdTable {
    std::vector<int32_t> item; // itemProbs' keys in list order
    std::vector<double> prob;  // their values
    std::vector<double> cum;   // sum += prob from 0.0 along the list
    bool tree = false;         // a put would have built a tree bin: the HashMap's iteration order is not modelled
};

// RankSGD.java:66-75.  col_size[j] = train.columnSize(j): the non-zero cells of column j
inline RanksgdTable ranksgd_item_table(int32_t n_items, const int32_t *col_size, int64_t num_rates) {
    RanksgdTable t;
    std::vector<int32_t> key;
    std::vector<double> prob;
    for (int32_t j = 0; j < n_items; ++j) {
        const double x = (double)col_size[j] + 0.0;
        // Java's double division: x / 0.0 is +Infinity for x > 0 and NaN for 0.0 / 0.0
        const double p = num_rates != 0 ? x / (double)num_rates : (x > 0.0 ? INFINITY : NAN);
        if (p > 0) key.push_back(j), prob.push_back(p);
    }
    const size_t n = key.size();
    auto hash_at = [&](size_t s) { return (uint32_t)key[s]; }; // Integer.hashCode()
    JavaHashTable table(16);
    table.fill(hash_at, n);
    t.tree = table.tree;
    std::vector<size_t> pos = table.order(hash_at, n);
    // Lists.sortMap(map): new ArrayList(entrySet()), Collections.sort with Lists$1 (Double.compareTo of the values): stable
    std::stable_sort(pos.begin(), pos.end(), [&](size_t a, size_t b) { return prob[a] < prob[b]; });
    double sum = 0.0;
    for (size_t x : pos) {
        sum += prob[x];
        t.item.push_back(key[x]), t.prob.push_back(prob[x]), t.cum.push_back(sum);
    }
    return t;
}

// RankSGD.java:97-107 from the stream state before the try: rand = Randoms.random() (two draws), then the first entry whose running
// sum reaches it; -1: none does
CMI_JM_HD inline int32_t ranksgd_try(uint64_t state, const int32_t *item, const double *cum, int32_t n) {
    JavaStream rng{state, 0};
    const double rand = 0.0 + (1.0 - 0.0) * rng.nextDouble(); // Randoms.uniform(0.0, 1.0)
    int32_t lo = 0, hi = n;
    while (lo < hi) {
        const int32_t mid = (int32_t)((uint32_t)(lo + hi) >> 1);
        if (cum[mid] < rand) lo = mid + 1;
        else hi = mid;
    }
    return lo < n ? item[lo] : -1;
}

// can a try return entry x?  rand is a multiple of 2^-53 in [0, 1 - 2^-53]
inline bool ranksgd_reachable(const double *cum, int32_t x) {
    const double max_rand = 1.0 - 0x1.0p-53;
    return x == 0 || (cum[x - 1] < cum[x] && cum[x - 1] < max_rand);
}

enum { RANKSGD_OK = 0, RANKSGD_FIRST_TRY_MISS = 1, RANKSGD_OUT_OF_TRIES = 2 };

// RankSGD.java:85-112: the cells in order (rptr / ridx: train.row(u), the non-zero cells, items ascending), each taking tries
// get(t), t = 0, 1, ..., until !Ru.contains(j).  A try of -1 leaves j as it was: -1 on a cell's first try (the reference's
// predict(u, -1) throws: RANKSGD_FIRST_TRY_MISS, *bad the cell), the rejected item on a later one (one more rejection).
// max_tries: RANKSGD_OUT_OF_TRIES rather than a try at or past it
template <class Get>
inline int ranksgd_assign(int32_t n_users, const int32_t *rptr, const int32_t *ridx, Get &&get, int64_t max_tries, int32_t *j_out,
                          int64_t *tries_used, int64_t *bad) {
    int64_t t = 0, c = 0;
    for (int32_t u = 0; u < n_users; ++u) {
        const int32_t b0 = rptr[u], cnt = rptr[u + 1] - b0;
        for (int32_t q = 0; q < cnt; ++q, ++c) {
            int32_t j = -1;
            for (;;) {
                if (t >= max_tries) {
                    *tries_used = t, *bad = c;
                    return RANKSGD_OUT_OF_TRIES;
                }
                const int32_t x = get(t++);
                if (x >= 0) j = x;
                if (j < 0) {
                    *tries_used = t, *bad = c;
                    return RANKSGD_FIRST_TRY_MISS;
                }
                if (!bpr_contains(ridx + b0, cnt, j)) break;
            }
            j_out[c] = j;
        }
    }
    *tries_used = t;
    return RANKSGD_OK;
}

// the first user with a cell whose row contains() every entry a try can return: RankSGD.java:94-112 would not end; -1: none
inline int32_t ranksgd_endless_user(int32_t n_users, const int32_t *rptr, const int32_t *ridx, const RanksgdTable &t) {
    std::vector<int32_t> reach;
    for (int32_t x = 0; x < (int32_t)t.item.size(); ++x)
        if (ranksgd_reachable(t.cum.data(), x)) reach.push_back(t.item[(size_t)x]);
    for (int32_t u = 0; u < n_users; ++u) {
        const int32_t b0 = rptr[u], cnt = rptr[u + 1] - b0;
        if (cnt == 0 || (size_t)cnt < reach.size()) continue; // contains() finds stored items only
        bool all = true;
        for (size_t x = 0; all && x < reach.size(); ++x) all = bpr_contains(ridx + b0, cnt, reach[x]);
        if (all) return u;
    }
    return -1;
}

// tries to compute ahead on the device: the cells, the expected rejections sum_u n_u p_u / (1 - p_u) with p_u the probability that a
// try is contained in row u, a twentieth more, and 1 024.  Only a guess that reserves memory
inline double ranksgd_reservation(int32_t n_users, int32_t n_items, const int32_t *rptr, const int32_t *ridx, const RanksgdTable &t) {
    std::vector<double> p_item((size_t)n_items, 0.0);
    for (size_t x = 0; x < t.item.size(); ++x) {
        const double lo = x == 0 ? 0.0 : std::min(t.cum[x - 1], 1.0), hi = std::min(t.cum[x], 1.0);
        p_item[(size_t)t.item[x]] = hi - lo; // the share of [0, 1) that lands on entry x
    }
    double cells = 0.0, rejected = 0.0;
    for (int32_t u = 0; u < n_users; ++u) {
        const int32_t b0 = rptr[u], cnt = rptr[u + 1] - b0;
        double p = 0.0;
        for (int32_t q = 0; q < cnt; ++q)
            if (bpr_contains(ridx + b0, cnt, ridx[b0 + q])) p += p_item[(size_t)ridx[b0 + q]];
        p = std::min(p, 0.999);
        cells += cnt, rejected += (double)cnt * p / (1.0 - p);
    }
    return std::ceil((cells + rejected) * 1.05) + 1024.0;
}

} // namespace cmi
