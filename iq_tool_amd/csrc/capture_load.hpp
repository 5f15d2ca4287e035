// capture_load.hpp -- what the accumulators over the BYTES of a capture share on the device (k_stats_pages, stats.hip; k_env_rows,
// env.hip; k_lag_rows, lag.hip): the integer codes of a frame beside its unpacked value, the bin and the rails of a code
// (include/iqgpu.h "capture statistics": the table), the loads -- four adjacent frames of a thread in one piece, one frame alone --
// through the word unpacks of dsp_device.hpp, the non-finite total of the two fold kernels, and the one ladder over formats that
// the three page launchers go through.  One definition of a format's rails, not one per accumulator.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "dsp_device.hpp"

namespace iqgpu {

// bin and rails of one integer code (include/iqgpu.h: the table).  c: the code, sign- or zero-extended; cu32 as its bit pattern
__device__ __forceinline__ void classify_code(int fmt, int c, int &bin, bool &lo, bool &hi)
{
    switch (fmt) {
    case IQGPU_FMT_CU8: bin = c; lo = c == 0; hi = c == 255; break;
    case IQGPU_FMT_CS8: bin = c + 128; lo = c == -128; hi = c == 127; break;
    case IQGPU_FMT_CU16: bin = c >> 8; lo = c == 0; hi = c == 65535; break;
    case IQGPU_FMT_CS16: bin = (c >> 8) + 128; lo = c == -32768; hi = c == 32767; break;
    case IQGPU_FMT_SC16Q11: {
        const int b = (c >> 4) + 128;
        bin = b < 0 ? 0 : b > 255 ? 255 : b; lo = c <= -2048; hi = c >= 2047;
        break; }
    case IQGPU_FMT_CS24: bin = (c >> 16) + 128; lo = c == -8388608; hi = c == 8388607; break;
    case IQGPU_FMT_CU32: bin = (int)((unsigned)c >> 24); lo = c == 0; hi = (unsigned)c == 0xffffffffu; break;
    default: /* IQGPU_FMT_CS32 */ bin = (c >> 24) + 128; lo = c == (int)0x80000000u; hi = c == 0x7fffffff; break;
    }
}

// ... of one finite cf32 component: v * 128 is exact, the clamp comes before the conversion
__device__ __forceinline__ void classify_float(float v, int &bin, bool &lo, bool &hi)
{
    float f = floorf(__fmul_rn(v, 128.0f));
    f = f < -128.0f ? -128.0f : f > 127.0f ? 127.0f : f;
    bin = (int)f + 128; lo = v <= -1.0f; hi = v >= 1.0f;
}

// the components of one frame on a rail, 0 .. 2: the rules above, for an accumulator that keeps no histogram (k_env_rows)
__device__ __forceinline__ uint32_t rails_of_codes(int fmt, int ci, int cq)
{
    int bin; bool li, hi, lq, hq;
    classify_code(fmt, ci, bin, li, hi); classify_code(fmt, cq, bin, lq, hq);
    return (uint32_t)li + (uint32_t)hi + (uint32_t)lq + (uint32_t)hq;
}
__device__ __forceinline__ uint32_t rails_of_floats(float re, float im)
{
    int bin; bool li, hi, lq, hq;
    classify_float(re, bin, li, hi); classify_float(im, bin, lq, hq);
    return (uint32_t)li + (uint32_t)hi + (uint32_t)lq + (uint32_t)hq;
}

// the two codes of frame j of a format decoded at run time (the value comes from unpack_one: the loads are the same)
__device__ __forceinline__ void codes_one(const void *raw, int64_t j, int fmt, int &ci, int &cq)
{
    switch (fmt) {
    case IQGPU_FMT_CU16: { const unsigned short *p = (const unsigned short *)raw + 2 * j; ci = p[0]; cq = p[1]; break; }
    case IQGPU_FMT_SC16Q11: { const short *p = (const short *)raw + 2 * j; ci = p[0]; cq = p[1]; break; }
    case IQGPU_FMT_CS24: {
        const unsigned char *p = (const unsigned char *)raw + 6 * j;
        ci = (int)(((unsigned)p[0] << 8) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 24)) >> 8;
        cq = (int)(((unsigned)p[3] << 8) | ((unsigned)p[4] << 16) | ((unsigned)p[5] << 24)) >> 8;
        break; }
    default: { /* IQGPU_FMT_CS32, IQGPU_FMT_CU32: the bit pattern */ const int *p = (const int *)raw + 2 * j; ci = p[0]; cq = p[1]; break; }
    }
}

__device__ __forceinline__ void codes_b16(uint32_t w, int &ci, int &cq) { ci = (short)(w & 0xffffu); cq = (short)(w >> 16); }
template <int FMT> __device__ __forceinline__ void codes_b8(uint32_t h, int &ci, int &cq)
{
    if constexpr (FMT == IQGPU_FMT_CU8) { ci = (int)(h & 0xffu); cq = (int)((h >> 8) & 0xffu); }
    else { ci = (signed char)(h & 0xffu); cq = (signed char)((h >> 8) & 0xffu); }
}

// frame j of raw, alone (row ends, unaligned launches, run-time formats)
template <int FMT>
__device__ __forceinline__ void load_one(const void *raw, int64_t j, int fmt, int &ci, int &cq, cf2 &x)
{
    ci = cq = 0;
    if constexpr (FMT == IQGPU_FMT_CS16) {
        const uint32_t w = ((const uint32_t *)raw)[j];
        codes_b16(w, ci, cq); x = unpack_b16(w, FMT, 1.0f);
    } else if constexpr (FMT == IQGPU_FMT_CU8 || FMT == IQGPU_FMT_CS8) {
        const uint32_t h = ((const uint16_t *)raw)[j];
        codes_b8<FMT>(h, ci, cq); x = unpack_b8(h, FMT, 1.0f);
    } else if constexpr (FMT == IQGPU_FMT_CF32) {
        const float2 v = ((const float2 *)raw)[j];
        x = cf2{__fmul_rn(v.x, 1.0f), __fmul_rn(v.y, 1.0f)};
    } else {
        codes_one(raw, j, fmt, ci, cq); x = unpack_one(raw, j, fmt, 1.0f);
    }
}

// bytes a thread's four frames are fetched as in one piece, 0: never
template <int FMT> constexpr int vec_bytes()
{
    return FMT == IQGPU_FMT_CS16 ? 16 : (FMT == IQGPU_FMT_CU8 || FMT == IQGPU_FMT_CS8) ? 8 : FMT == IQGPU_FMT_CF32 ? 16 : 0;
}

// frames j .. j + 3 of raw, all inside the launch, at an address aligned to vec_bytes<FMT>()
template <int FMT>
__device__ __forceinline__ void load_four(const void *raw, int64_t j, int (&ci)[4], int (&cq)[4], cf2 (&x)[4])
{
    if constexpr (FMT == IQGPU_FMT_CS16) {
        const uint4 v = *(const uint4 *)((const char *)raw + 4 * j);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) { codes_b16(w[k], ci[k], cq[k]); x[k] = unpack_b16(w[k], FMT, 1.0f); }
    } else if constexpr (FMT == IQGPU_FMT_CU8 || FMT == IQGPU_FMT_CS8) {
        const uint2 v = *(const uint2 *)((const char *)raw + 2 * j);
        const uint32_t w[2] = {v.x, v.y};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t h = (w[k >> 1] >> ((k & 1) * 16)) & 0xffffu;
            codes_b8<FMT>(h, ci[k], cq[k]); x[k] = unpack_b8(h, FMT, 1.0f);
        }
    } else if constexpr (FMT == IQGPU_FMT_CF32) {
        const float4 v0 = *(const float4 *)((const char *)raw + 8 * j);
        const float4 v1 = *(const float4 *)((const char *)raw + 8 * j + 16);
        x[0] = cf2{__fmul_rn(v0.x, 1.0f), __fmul_rn(v0.y, 1.0f)}; x[1] = cf2{__fmul_rn(v0.z, 1.0f), __fmul_rn(v0.w, 1.0f)};
        x[2] = cf2{__fmul_rn(v1.x, 1.0f), __fmul_rn(v1.y, 1.0f)}; x[3] = cf2{__fmul_rn(v1.z, 1.0f), __fmul_rn(v1.w, 1.0f)};
#pragma unroll
        for (int k = 0; k < 4; ++k) ci[k] = cq[k] = 0;
    }
}

// a fold kernel's first half, one workgroup of THREADS: *total += the groups' counts (n_groups > 0: a cf32 launch)
template <int THREADS>
__device__ __forceinline__ void fold_nonfinite(const uint32_t *nonfinite, int n_groups, uint64_t *total, uint64_t (&W)[THREADS])
{
    const int tid = threadIdx.x;
    if (n_groups > 0) {
        uint64_t n = 0;
        for (int g = tid; g < n_groups; g += THREADS) n += nonfinite[g];
        W[tid] = n;
        __syncthreads();
        for (int m = THREADS / 2; m >= 1; m >>= 1) {
            if (tid < m) W[tid] += W[tid + m];
            __syncthreads();
        }
        if (tid == 0) *total += W[0];
    }
}

// the format instantiation of a page launch: launch(F) with std::integral_constant<int, format>, -1 for every format that is decoded
// at run time (psd_stream.hpp's psd_dispatch, without the sizes)
template <class Launch>
static hipError_t page_dispatch(int fmt, Launch launch)
{
    switch (fmt) {
    case IQGPU_FMT_CS16: launch(std::integral_constant<int, IQGPU_FMT_CS16>{}); break;
    case IQGPU_FMT_CU8:  launch(std::integral_constant<int, IQGPU_FMT_CU8>{}); break;
    case IQGPU_FMT_CS8:  launch(std::integral_constant<int, IQGPU_FMT_CS8>{}); break;
    case IQGPU_FMT_CF32: launch(std::integral_constant<int, IQGPU_FMT_CF32>{}); break;
    default:             launch(std::integral_constant<int, -1>{}); break;
    }
    return hipGetLastError();
}

} // namespace iqgpu
