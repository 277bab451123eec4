// lrmf_host.hpp -- what cmi_lrmf_set_ratings prepares on the host, once per matrix (LRMF.java:55-67 and everything of :70-110 that does
// not depend on the model): userExp, A = exp(r) / userExp[u] per cell, the unit schedule and its launches.  No HIP: plain C++ over
// java_math.hpp and level_schedule.hpp, so a stand-alone program can run it under a sanitizer.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "java_math.hpp"
#include "level_schedule.hpp"

namespace cmi {

constexpr int LRMF_MAX_K = 128;            // factors: a lane per factor applies a cell's update
constexpr int LRMF_BLOCK = 256;            // threads per workgroup: item lanes of one pass of a cell's sum
constexpr int LRMF_LDS_BYTES = 160 * 1024; // LDS of a gfx950 compute unit; a unit of the most rows takes it whole
// doubles every workgroup holds beside the item rows: P[u], two buffers of one pass's exps, and the cell's scalars (uexp, pred, exp(pred), g(pred),
// g(-pred), B; two spare)
constexpr int LRMF_LDS_FIXED = LRMF_MAX_K + 2 * LRMF_BLOCK + 8;

// doubles between two item rows in LDS: odd, so the 32 lanes of a half-wave, a row each, read one factor from 32 different 8-byte
// slots of the 64 banks
constexpr int lrmf_stride(int k) { return k | 1; }
// rows of k factors that fit beside the fixed part
constexpr int lrmf_lds_rows(int k) { return (LRMF_LDS_BYTES / 8 - LRMF_LDS_FIXED) / lrmf_stride(k); }
// LDS bytes of a launch whose largest LDS-form unit has `rows` cells
constexpr size_t lrmf_lds_bytes(int k, int rows) { return ((size_t)LRMF_LDS_FIXED + (size_t)rows * lrmf_stride(k)) * 8; }

struct LrmfLaunch {
    int32_t x0, x1; // units order[x0, x1)
    int32_t rows;   // the most cells among their LDS-form units
    bool run;       // single-unit levels in one workgroup; else one level, a workgroup per unit
};

struct LrmfPlan {
    std::vector<double> user_exp, A;
    std::vector<uint8_t> nz;
    std::vector<int32_t> order, level_ptr;
    std::vector<LrmfLaunch> launches;
    int64_t n_levels = 0, alone = 0, runs = 0, widest = 0, global_units = 0, max_chain = 0;
};

// ptr / idx / val: the train matrix by user, columns ascending inside a row, stored zeros included (the MatrixEntry iterator's order).
// lds_rows: units of more cells run in the global form (0: all of them)
inline void lrmf_prepare(int32_t n_users, int32_t n_items, const int32_t *ptr, const int32_t *idx, const double *val, int32_t lds_rows,
                         LrmfPlan &p) {
    const size_t n = (size_t)ptr[n_users];
    p.user_exp.assign((size_t)n_users, 0.0);
    p.A.resize(n), p.nz.resize(n);
    for (int32_t u = 0; u < n_users; ++u) // LRMF.java:60-65: userExp.add(u, Math.exp(ruj)) in iterator order
        for (int32_t c = ptr[u]; c < ptr[u + 1]; ++c) p.user_exp[(size_t)u] += fdlibm_exp(val[c]);
    for (int32_t u = 0; u < n_users; ++u)
        for (int32_t c = ptr[u]; c < ptr[u + 1]; ++c) {
            p.A[(size_t)c] = fdlibm_exp(val[c]) / p.user_exp[(size_t)u]; // :89, :95, :96
            p.nz[(size_t)c] = val[c] != 0.0;                             // getColumns(u) leaves a stored zero out
        }
    p.n_levels = build_unit_levels(n_users, n_items, ptr, idx, p.order, p.level_ptr, nullptr, &p.max_chain);
    p.launches.clear();
    p.alone = p.runs = p.widest = p.global_units = 0;
    auto cells_of = [&](int32_t x) { return ptr[p.order[(size_t)x] + 1] - ptr[p.order[(size_t)x]]; };
    auto rows_of = [&](int32_t x0, int32_t x1) {
        int32_t rows = 0;
        for (int32_t x = x0; x < x1; ++x)
            if (cells_of(x) <= lds_rows) rows = std::max(rows, cells_of(x));
        return rows;
    };
    for (size_t x = 0; x < p.order.size(); ++x) p.global_units += cells_of((int32_t)x) > lds_rows;
    for (int32_t l = 0; l < (int32_t)p.n_levels;) {
        const int32_t x0 = p.level_ptr[(size_t)l], w = p.level_ptr[(size_t)l + 1] - x0;
        p.widest = std::max<int64_t>(p.widest, w);
        if (w > 1) { // a level of several units: one launch
            p.launches.push_back({x0, x0 + w, rows_of(x0, x0 + w), false});
            ++p.alone, ++l;
            continue;
        }
        int32_t e = l + 1; // consecutive levels of one unit each: one workgroup walks them
        while (e < (int32_t)p.n_levels && p.level_ptr[(size_t)e + 1] - p.level_ptr[(size_t)e] == 1) ++e;
        p.widest = std::max<int64_t>(p.widest, 1);
        p.launches.push_back({x0, p.level_ptr[(size_t)e], rows_of(x0, p.level_ptr[(size_t)e]), true});
        ++p.runs, l = e;
    }
}

} // namespace cmi
