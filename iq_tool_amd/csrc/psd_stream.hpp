// psd_stream.hpp -- device code that the accumulators over a stream's segment grid share: k_psd_pages (psd.hip) and k_sgram_cells
// (sgram.hip) read their frames through the one psd_unpack below, so the two see the same x for the same bytes.  (The other shared piece,
// the carry of trailing frames, is k_psd_carry behind launch_psd_carry of psd.hpp: one kernel, defined once in psd.hip, launched by both
// host sides.)  psd_dispatch is the one ladder over sizes and formats both launchers go through.  Included by .hip sources only.
#pragma once
#include "dsp_device.hpp"

namespace iqgpu {

// one frame of a format known at compile time, fetched as one word where its alignment allows (unpack_b16 / unpack_b8, dsp_device.hpp)
template <int FMT>
__device__ __forceinline__ cf2 psd_unpack(const void *raw, int64_t j, int fmt, float gain)
{
    if constexpr (FMT == IQGPU_FMT_CS16) {
        return unpack_b16(((const uint32_t *)raw)[j], FMT, gain);
    } else if constexpr (FMT == IQGPU_FMT_CU8 || FMT == IQGPU_FMT_CS8) {
        return unpack_b8(((const uint16_t *)raw)[j], FMT, gain);
    } else if constexpr (FMT == IQGPU_FMT_CF32) {
        const float2 v = ((const float2 *)raw)[j];
        return cf2{__fmul_rn(v.x, gain), __fmul_rn(v.y, gain)};
    } else {
        return unpack_one(raw, j, fmt, gain);
    }
}

// the (log2 nfft, format) instantiation of a launch of either kernel: launch(L, F) with std::integral_constant<int, log2 nfft> and
// <int, format>, the format -1 for every one that is decoded at run time
template <class Launch>
static hipError_t psd_dispatch(int log2n, int fmt, Launch launch)
{
    auto of_size = [&](auto L) {
        switch (fmt) {
        case IQGPU_FMT_CS16: launch(L, std::integral_constant<int, IQGPU_FMT_CS16>{}); break;
        case IQGPU_FMT_CU8:  launch(L, std::integral_constant<int, IQGPU_FMT_CU8>{}); break;
        case IQGPU_FMT_CS8:  launch(L, std::integral_constant<int, IQGPU_FMT_CS8>{}); break;
        case IQGPU_FMT_CF32: launch(L, std::integral_constant<int, IQGPU_FMT_CF32>{}); break;
        default:             launch(L, std::integral_constant<int, -1>{}); break;
        }
        return hipGetLastError();
    };
    switch (log2n) {
    case 10: return of_size(std::integral_constant<int, 10>{});
    case 11: return of_size(std::integral_constant<int, 11>{});
    case 12: return of_size(std::integral_constant<int, 12>{});
    default: return hipErrorInvalidValue;
    }
}

} // namespace iqgpu
