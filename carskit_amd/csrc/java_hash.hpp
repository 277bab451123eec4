// java_hash.hpp -- the iteration order of a java.util.HashMap / HashSet (JDK 8), stated once for the host and the device (DESIGN.md,
// "java.util.HashMap iteration order").  A bin holds its nodes in insertion order and a resize keeps the order inside a bin, so a table
// without a tree bin iterates by (bucket at the final capacity, insertion).  What is modelled here is therefore the table's growth
// and the put that would build a tree bin; keys and values stay with the caller, who names a key by its position in put order.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <vector>

namespace cmi {

// HashMap.hash(): the bucket of hashCode h in a table of cap slots is java_spread(h) & (cap - 1)
__host__ __device__ inline uint32_t java_spread(uint32_t h) { return h ^ (h >> 16); }

// Tables below 64 slots, serially.  The distinct keys whose hashCodes are hash_at(0..n-1) are put in that order into a table of (cap,
// thr) that holds none; returns how many puts were consumed when the table reached 64 slots (n: it never did), with (cap, thr) as the
// last of them left it.  A put that makes a bin of 9 nodes doubles such a table (treeifyBin -> resize), then ++size > thr doubles it.
// cnt: 64 bin counts of scratch.
template <class H>
__host__ __device__ inline int java_walk_below_64(H hash_at, int n, int &cap, int &thr, int32_t *cnt) {
    int t = 0;
    auto recount = [&](int upto) {
        for (int b = 0; b < 64; ++b) cnt[b] = 0;
        for (int s = 0; s < upto; ++s) ++cnt[java_spread(hash_at(s)) & (cap - 1)];
    };
    if (cap < 64) recount(0);
    while (t < n && cap < 64) {
        const int b = java_spread(hash_at(t)) & (cap - 1);
        const bool grow = ++cnt[b] >= 9; // treeifyBin on a small table: resize()
        ++t;
        const int before = cap;
        if (grow) cap <<= 1, thr <<= 1;
        if (t > thr) cap <<= 1, thr <<= 1; // ++size > threshold
        if (cap != before && cap < 64) recount(t);
    }
    return t;
}

// The host's model of one table.  slots 16: new HashMap() / new HashSet(); 4: new HashSet(3), what guava's HashMultimap keeps per key.
struct JavaHashTable {
    size_t cap, thr; // thr = 0.75 x cap
    bool tree = false; // sticky: some put made a bin of 9 nodes in a table of 64 slots or more (the table in force for that put)
    explicit JavaHashTable(int slots) : cap((size_t)slots), thr((size_t)slots * 3 / 4) {}

    // the distinct keys whose hashCodes are hash_at(0..n-1), put in that order into this table while it holds none: a new table, or
    // one kept by clear().  Equal hashCodes are separate nodes.  O(n) amortised: the bins are counted again after each doubling.
    template <class H>
    void fill(H hash_at, size_t n) {
        size_t t = 0;
        if (cap < 64) {
            int32_t small[64];
            int c = (int)cap, th = (int)thr;
            t = (size_t)java_walk_below_64(hash_at, (int)(n < 64 ? n : 64), c, th, small);
            cap = (size_t)c, thr = (size_t)th;
        }
        if (t == n) return;
        std::vector<uint32_t> cnt;
        auto recount = [&] {
            cnt.assign(cap, 0);
            for (size_t s = 0; s < t; ++s) ++cnt[java_spread(hash_at(s)) & (cap - 1)];
        };
        recount();
        while (t < n) {
            if (++cnt[java_spread(hash_at(t)) & (cap - 1)] >= 9) tree = true; // treeifyBin builds the tree bin; no resize
            if (++t > thr) cap <<= 1, thr <<= 1, recount();
        }
    }

    // positions 0..n-1 of the keys last filled in, in iteration order: stably by bucket at the final capacity
    template <class H>
    std::vector<size_t> order(H hash_at, size_t n) const {
        std::vector<size_t> start(cap + 1, 0), pos(n);
        for (size_t i = 0; i < n; ++i) ++start[(java_spread(hash_at(i)) & (cap - 1)) + 1];
        for (size_t b = 0; b < cap; ++b) start[b + 1] += start[b];
        for (size_t i = 0; i < n; ++i) pos[start[java_spread(hash_at(i)) & (cap - 1)]++] = i;
        return pos;
    }
};

} // namespace cmi
