// pair_tree.hpp -- the cross-lane half of the fixed tree of adjacent pairs the row accumulators share (k_env_rows, env.hip; k_lag_rows,
// lag.hip): the value of the partner lane at each level.  One definition of the order, not one per kernel.
#pragma once
#include <hip/hip_runtime.h>

namespace iqgpu {

// the value of the lane M away in the pair tree.  After the levels below M every lane of a group of M holds the group's sum, so any
// lane of the partner group serves: quad permutes for 1 and 2, the mirrors of 8 and 16 lanes for 4 and 8 (lane i <- 7 - i, 15 - i)
template <int M> __device__ __forceinline__ int pair_i32(int v)
{
    if constexpr (M == 1) return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, true);             // quad_perm [1, 0, 3, 2]
    else if constexpr (M == 2) return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xf, 0xf, true);        // quad_perm [2, 3, 0, 1]
    else if constexpr (M == 4) return __builtin_amdgcn_update_dpp(0, v, 0x141, 0xf, 0xf, true);       // row_half_mirror
    else if constexpr (M == 8) return __builtin_amdgcn_update_dpp(0, v, 0x140, 0xf, 0xf, true);       // row_mirror
    else return __shfl_xor(v, M);
}
template <int M> __device__ __forceinline__ double pair_f64(double v)
{
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)pair_i32<M>((int)(uint32_t)u), hi = (uint32_t)pair_i32<M>((int)(uint32_t)(u >> 32));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
template <int M> __device__ __forceinline__ float pair_f32(float v) { return __builtin_bit_cast(float, pair_i32<M>(__builtin_bit_cast(int, v))); }

} // namespace iqgpu
