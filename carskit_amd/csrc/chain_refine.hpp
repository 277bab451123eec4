// chain_refine.hpp -- where a hub row's chain is cut into units, refined within the schedule's slack.  ONE definition of the rule,
// compiled for the host builder (level_schedule.cpp) and for the device builder (sched_device.hip): the two give the same schedule.
//
// The greedy walk (chain_pass) places every tuple as early as possible and closes a unit whenever the spoke row's previous tuple sits at
// the unit's level or later.  The order-exactness argument needs less: per hub row and per spoke row the (level, position in unit) order
// of the row's tuples must be the CRS order.  So a tuple may run at ANY level strictly below its spoke successor's, as long as its hub
// chain stays in order -- and tuples that rise into the level of the hub's next unit share that unit's round trip of the hub row.
//
// One PASS reads the levels of the previous pass only (double-buffered) and handles every hub row on its own, walking the row's chain
// BACKWARD: a group of consecutive tuples becomes one unit at level L = the old level of its last member (the highest old level in the
// group) if it has <= max_chain members, L < the old level of every member's spoke successor, and L < the level of the hub's following
// unit.  Levels only rise, and only against the snapshot: a tuple's spoke successor ends the pass at or above its snapshot level, its
// spoke predecessor rises to below the tuple's snapshot level at most -- so rows may be handled in any order or at the same time and the
// result is a pure function of the input.  A unit that takes nobody in keeps its level (max_chain 1: nothing moves).  Two members with
// the same spoke row never meet in a group: the earlier one's spoke successor is the later one or lies before it, at a level <= L.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#if defined(__HIPCC__)
#define CMI_HD __host__ __device__
#else
#define CMI_HD
#endif

namespace cmi {

// passes of the refinement; CMI_CHAIN_REFINE=<passes> (read when a schedule is built), 0 keeps the greedy cut
inline int chain_refine_passes() {
    if (const char *env = getenv("CMI_CHAIN_REFINE")) {
        const int v = atoi(env);
        return v < 0 ? 0 : (v > 16 ? 16 : v);
    }
    return 4;
}

// One hub row, one pass.  The row's chain is list positions [b, e) (CRS order).  lev_in[i] = level of list entry i, ub[i] = snapshot level
// of its spoke successor - 1 (no successor: any value >= the number of levels).  Writes lev_out[b..e).  last pass (lt != nullptr; lt[i] =
// CRS index of list entry i): also the units -- per tuple the CRS index of its unit's first tuple and its position inside the unit, per
// first tuple the unit's level and length (the other entries of unit_level are zero already).
CMI_HD inline void chain_recut_row(int32_t b, int32_t e, int max_chain, const int32_t *lev_in, const int32_t *ub, int32_t *lev_out, const int32_t *lt,
                                   int32_t *unit_of, uint8_t *pos, int32_t *unit_level, uint8_t *unit_len) {
    int32_t next_level = INT32_MAX; // level of the hub's following unit
    for (int32_t i = e - 1; i >= b;) {
        const int32_t L = lev_in[i];
        int32_t hi = ub[i] < next_level - 1 ? ub[i] : next_level - 1; // (>= L: the input is a valid schedule)
        int32_t first = i;
        while (first > b && i - first + 1 < max_chain) {
            const int32_t h2 = ub[first - 1] < hi ? ub[first - 1] : hi;
            if (h2 < L) break;
            hi = h2;
            --first;
        }
        for (int32_t k = first; k <= i; ++k) lev_out[k] = L;
        if (lt) {
            const int32_t t0 = lt[first];
            for (int32_t k = first; k <= i; ++k) {
                unit_of[lt[k]] = t0;
                pos[lt[k]] = (uint8_t)(k - first);
            }
            unit_level[t0] = L;
            unit_len[t0] = (uint8_t)(i - first + 1);
        }
        next_level = L;
        i = first - 1;
    }
}

} // namespace cmi
