// lrmf_kernels.hpp -- device side of LRMF (lrmf_kernels.hip), launched by lrmf_api.cpp, and the LDS budget both sides compute with.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "lrmf_host.hpp"

namespace cmi {

struct LrmfEpoch {
    int k = 0;
    double *P = nullptr, *Q = nullptr;
    const int32_t *ptr = nullptr;   // n_users + 1: the cells of user u are [ptr[u], ptr[u + 1]), the matrix iterator's order
    const int32_t *col = nullptr;   // per cell: its column
    const double *A = nullptr;      // per cell: Math.exp(r) / userExp[u]
    const uint8_t *nz = nullptr;    // per cell: r != 0.0, the column is in getColumns(u)
    const int32_t *order = nullptr; // the users with a cell sorted by level
    double *slots = nullptr;        // n x (k + 1): -A log(B) and the k regularisation terms of every cell
    double lrate = 0.0, regU = 0.0, regI = 0.0;
    int32_t lds_rows = 0;           // a unit of more cells leaves its item rows in memory (0: every unit does)
};
// units order[x0, x1): one level of any width, a workgroup per unit, or (run) single-unit levels walked by one workgroup with a barrier
// between units.  rows: the most cells of a unit among them that keeps its rows in LDS (sizes the launch's LDS)
hipError_t lrmf_launch_level(const LrmfEpoch &a, int32_t x0, int32_t x1, int32_t rows, hipStream_t s);
hipError_t lrmf_launch_run(const LrmfEpoch &a, int32_t x0, int32_t x1, int32_t rows, hipStream_t s);

} // namespace cmi
