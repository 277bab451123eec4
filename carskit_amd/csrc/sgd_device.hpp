// sgd_device.hpp -- helpers shared by the SGD kernel translation units (mf_sgd_kernels.hip, chain_kernels.hip,
// owner_kernels.hip): DPP row reductions, the per-model container traits and the host's model dispatch.  Internal header.
#pragma once
#include <hip/hip_runtime.h>

#include "mf_sgd_kernels.hpp"

#include <type_traits>

namespace cmi {

// ---------------------------------------------------------------------------------------------
// cross-lane helpers
// ---------------------------------------------------------------------------------------------

// DPP row_ror:n -- lane l of each 16-lane row reads lane (l - n) mod 16 of the same row.
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}

// Sum over the 16 lanes of a DPP row; every lane ends with the bit-identical total (the rotation
// tree pairs the same operands in every lane, and fp add is commutative).
__device__ __forceinline__ float row_sum16(float x) {
    x += dpp_f32<0x128>(x); // row_ror:8
    x += dpp_f32<0x124>(x); // row_ror:4
    x += dpp_f32<0x122>(x); // row_ror:2
    x += dpp_f32<0x121>(x); // row_ror:1
    return x;
}

template <typename T>
__device__ __forceinline__ T wave_sum64(T x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

template <int MODEL>
struct Traits {
    static constexpr ModelParams p = model_params(MODEL);
    static constexpr bool has_bu = p.has_bu, has_bj = p.has_bj, has_bc = p.has_bc, has_ic = p.has_ic, has_uc = p.has_uc;
    static constexpr bool has_ctx = p.has_ctx;
};

// Host side: call f(std::integral_constant<int, MODEL>) for the runtime model id; `invalid` for a model outside the set.
// PARALLEL = the models with fast / small / narrow-run / chain / owner kernels; ALL adds CAMF_C (generic level and serial kernels).
enum class ModelSet { PARALLEL, ALL };
template <ModelSet SET, typename R, typename F>
R dispatch_model(int model, R invalid, F &&f) {
    switch (model) {
    case BIASEDMF: return f(std::integral_constant<int, BIASEDMF>{});
    case PMF: return f(std::integral_constant<int, PMF>{});
    case CAMF_C:
        if constexpr (SET == ModelSet::ALL) return f(std::integral_constant<int, CAMF_C>{});
        break;
    case CAMF_CI: return f(std::integral_constant<int, CAMF_CI>{});
    case CAMF_CU: return f(std::integral_constant<int, CAMF_CU>{});
    case CAMF_CUCI: return f(std::integral_constant<int, CAMF_CUCI>{});
    }
    return invalid;
}

// Sum over the LPT (4, 8 or 16) lanes of a group that shares one tuple in the small-k kernels: quad permutes, then row
// (half-)mirrors; every lane of the group ends with the same total.
template <int LPT>
__device__ __forceinline__ float group_sum(float x) {
    x += dpp_f32<0xB1>(x); // quad_perm [1,0,3,2]
    x += dpp_f32<0x4E>(x); // quad_perm [2,3,0,1]
    if (LPT >= 8) x += dpp_f32<0x141>(x);  // row_half_mirror: lane i <- lane 7-i of its half row (the other quad's total)
    if (LPT >= 16) x += dpp_f32<0x140>(x); // row_mirror: lane i <- lane 15-i (the other half's total)
    return x;
}

// fp64 flavour of the 16-lane DPP row sum (both dwords rotated with the same control)
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double row_sum16(double x) {
    x += dpp_f64<0x128>(x);
    x += dpp_f64<0x124>(x);
    x += dpp_f64<0x122>(x);
    x += dpp_f64<0x121>(x);
    return x;
}

} // namespace cmi
