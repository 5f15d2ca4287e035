// iq_calib.hpp -- I/Q calibration on the device (include/iqgpu.h: iqgpu_iq_metric_batch, iqgpu_chain_calibrate_iq): the argument
// blocks and launchers of k_iq_blocks / k_iq_metric (iq_calib.hip; host side iq_calib.cpp) and -- for device code only -- the
// per-sample expressions of a probe block, which k_iq_probe (kernels.hip) shares with k_iq_blocks.
#pragma once
#include "iq_search.hpp"
#include "kernels.hpp"

namespace iqgpu {

// k_iq_blocks: block b = the 1024 frames from frame b * stride of raw, through unpack / gain / [dc block from a zero state]
struct IqBlocksArgs {
    const void *raw; int32_t in_fmt; float gain;
    int32_t dc_enable; float dc_c;
    int64_t stride;           // frames between the starts of two blocks
    int32_t n_blocks;
    cf2 *out;                 // [n_blocks][1024]
};
hipError_t launch_iq_blocks(const IqBlocksArgs &a, hipStream_t s);

// k_iq_metric: the utility of every (block, candidate) and the power statistics of every block
struct IqMetricArgs {
    const cf2 *blocks; int64_t stride;    // block b at blocks + b * stride
    int32_t n_blocks, n_cand;             // n_cand <= kIqCandsPerLaunch
    const iqgpu_iq_cand *cands;
    const float *window;                  // [1024], the optimiser's Hamming window
    const cf2 *twiddle;                   // [1024], exp(-2 pi i k / 1024)
    float *metric; int64_t metric_pitch;  // metric[b * metric_pitch + c]
    float *power;                         // [n_blocks][2]: average_power_db, power_range_db; NULL: not wanted
};
hipError_t launch_iq_metric(const IqMetricArgs &a, hipStream_t s);

} // namespace iqgpu

#if defined(__HIPCC__)
#include "dsp_device.hpp"

namespace iqgpu {

// The head of a probe block, one wave: x[0 .. 1024) (LDS) = frames first .. first + 1023 of raw through unpack and gain, then --
// dc_enable -- through the DC blocker from the state (vr, vi): the 1024-step recurrence on lane 0.  The one definition behind
// k_iq_probe (the state the stream is in) and k_iq_blocks (zero: a fresh pre-processor).  Ends behind a barrier.
__device__ __forceinline__ void iq_block_head(cf2 *x, const void *raw, int64_t first, int in_fmt, float gain,
                                              bool dc_enable, float dc_c, float vr, float vi, int lane)
{
    for (int i = lane; i < kIqN; i += 64) x[i] = unpack_one(raw, first + i, in_fmt, gain);
    __syncthreads();
    if (dc_enable && lane == 0) {
        const float aa = 1.0f - dc_c;
        for (int i = 0; i < kIqN; ++i) {
            const cf2 v = x[i];
            x[i] = cf2{fmaf(-aa, vr, v.x), fmaf(-aa, vi, v.y)};
            vr = fmaf(dc_c, vr, v.x); vi = fmaf(dc_c, vi, v.y);
        }
    }
    __syncthreads();
}

} // namespace iqgpu
#endif
