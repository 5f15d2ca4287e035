// iq_calib.hip -- the kernels of the I/Q calibration (include/iqgpu.h "I/Q calibration"; host side iq_calib.cpp).
//   k_iq_blocks   block b of a raw buffer, taken where iq_correct_apply acts: k_iq_probe's head (iq_calib.hpp, one definition) from a
//                 zero DC state, no I/Q correction, no NCO.  One wave per block.
//   k_iq_metric   the optimiser's utility (iq_optimizer.cpp: metric, estimate_power) of every (block, candidate).  One wave per
//                 (block, tile of kIqCandTile candidates): window, ONE forward 1024-point transform in LDS (fft16_lds<10>), then
//                 the candidates from the two real spectra.  With X = FFT(w (re + j im)):
//                     R[k] = (X[k] + conj X[N-k]) / 2 = FFT(w re),   I[k] = (X[k] - conj X[N-k]) / (2j) = FFT(w im)
//                     Y_c[k] = (1 + mag) R[k] + j (I[k] + phase R[k])                  -- the correction is linear, the window real
//                 Every tile runs the transform again rather than sharing it through memory: the transform is ~1 000 vector
//                 instructions a lane, a tile's 16 candidates x 16 bins x (hypotf + log10f) ~20 000, and small tiles are what
//                 spreads 64 blocks x 81 candidates over the machine (384 waves instead of 64); DESIGN 3.8.
//                 Bins: lane l owns i = 25 + l + 64 q, q = 0 .. 7 (i < 486), p_neg = S[i] = bin 512 + i, p_pos = S[1023 - i] = bin
//                 511 - i of the transform -- the reference's pair, one bin off the mirror, kept as it is.  A lane sums its bins in
//                 ascending order, then a butterfly of six fixed exchanges (32 .. 1) sums the 64 lanes: the same bits on every call.
#include <hip/hip_runtime.h>

#include "fft16.hpp"
#include "iq_calib.hpp"

namespace iqgpu {

__global__ __launch_bounds__(64) void k_iq_blocks(const IqBlocksArgs a)
{
    __shared__ cf2 x[kIqN];
    const int lane = threadIdx.x;
    const int64_t b = blockIdx.x;
    iq_block_head(x, a.raw, b * a.stride, a.in_fmt, a.gain, a.dc_enable != 0, a.dc_c, 0.0f, 0.0f, lane);
    cf2 *out = a.out + b * kIqN;
    for (int i = lane; i < kIqN; i += 64) out[i] = x[i];
}

hipError_t launch_iq_blocks(const IqBlocksArgs &a, hipStream_t s)
{
    if (a.n_blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_iq_blocks, dim3((unsigned)a.n_blocks), dim3(64), 0, s, a);
    return hipGetLastError();
}

// 20 log10f(|v| / 1024 + 1e-12f): iq_optimizer.cpp power_spectrum, the same float expressions
__device__ __forceinline__ float iq_db(float re, float im)
{
    float m = hypotf(re, im);
    m /= (float)kIqN;
    return 20.0f * log10f(m + 1e-12f);
}

constexpr int kIqBinsPerLane = (kIqBinHi - kIqBinLo + 63) / 64;      // 8

__global__ __launch_bounds__(64) void k_iq_metric(const IqMetricArgs a)
{
    __shared__ cf2 X[kIqN + (kIqN >> 5) + 2];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int c0 = (int)blockIdx.y * kIqCandTile;
    const int nc = a.n_cand - c0 < kIqCandTile ? a.n_cand - c0 : kIqCandTile;
    const cf2 *blk = a.blocks + b * a.stride;
    cf2 io[16];                                                      // point tid + 64 r of the windowed block, then of its transform
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = tid + 64 * r;
        const cf2 v = blk[i];
        const float w = a.window[i];
        io[r] = cf2{v.x * w, v.y * w};
    }
    fft16_lds<10, false>(X, a.twiddle, tid, io);
    __syncthreads();                                                 // (the last pass's reads of X)
#pragma unroll
    for (int r = 0; r < 16; ++r) X[tid + 64 * r] = io[r];            // natural order, unpadded: a lane's bins are its neighbours'
    __syncthreads();

    // this lane's bins: the two real spectra at bin 512 + i (p_neg) and bin 511 - i (p_pos)
    float nRr[kIqBinsPerLane], nRi[kIqBinsPerLane], nIr[kIqBinsPerLane], nIi[kIqBinsPerLane];
    float pRr[kIqBinsPerLane], pRi[kIqBinsPerLane], pIr[kIqBinsPerLane], pIi[kIqBinsPerLane];
    float max_power = -1000.0f;
    double sum_power = 0.0;
#pragma unroll
    for (int q = 0; q < kIqBinsPerLane; ++q) {
        const int i = kIqBinLo + tid + 64 * q;
        const bool in = i < kIqBinHi;
        const int ii = in ? i : kIqBinLo;                            // (a lane past the last bin reads a valid one and drops it)
        const cf2 A = X[512 + ii], B = X[512 - ii];                  // X[k], X[N - k] at k = 512 + i
        const cf2 C = X[511 - ii], D = X[513 + ii];                  // X[k], X[N - k] at k = 511 - i
        nRr[q] = 0.5f * (A.x + B.x); nRi[q] = 0.5f * (A.y - B.y); nIr[q] = 0.5f * (A.y + B.y); nIi[q] = -0.5f * (A.x - B.x);
        pRr[q] = 0.5f * (C.x + D.x); pRi[q] = 0.5f * (C.y - D.y); pIr[q] = 0.5f * (C.y + D.y); pIi[q] = -0.5f * (C.x - D.x);
        if (in) {                                                    // estimate_power: candidate (0, 0) is the transform itself
            const float p_neg = iq_db(A.x, A.y), p_pos = iq_db(C.x, C.y);
            max_power = fmaxf(max_power, fmaxf(p_pos, p_neg));
            sum_power += (double)(p_pos + p_neg);
        }
    }
    if (a.power && blockIdx.y == 0) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { max_power = fmaxf(max_power, __shfl_xor(max_power, o)); sum_power += __shfl_xor(sum_power, o); }
        if (tid == 0) {
            const float average = (float)(sum_power / (double)(2 * (kIqBinHi - kIqBinLo)));
            a.power[2 * b] = average; a.power[2 * b + 1] = max_power - average;
        }
    }

    for (int c = 0; c < nc; ++c) {
        const iqgpu_iq_cand cd = a.cands[c0 + c];
        const float magp1 = 1.0f + cd.mag, ph = cd.phase;
        float part = 0.0f;
#pragma unroll
        for (int q = 0; q < kIqBinsPerLane; ++q) {
            const float p_neg = iq_db(magp1 * nRr[q] - (nIi[q] + ph * nRi[q]), magp1 * nRi[q] + (nIr[q] + ph * nRr[q]));
            const float p_pos = iq_db(magp1 * pRr[q] - (pIi[q] + ph * pRi[q]), magp1 * pRi[q] + (pIr[q] + ph * pRr[q]));
            const bool in = kIqBinLo + tid + 64 * q < kIqBinHi;
            if (in && (p_pos > -80.0f || p_neg > -80.0f)) { const float d = p_pos - p_neg; part += d * d; }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o);
        if (tid == 0) a.metric[b * a.metric_pitch + c0 + c] = part;
    }
}

hipError_t launch_iq_metric(const IqMetricArgs &a, hipStream_t s)
{
    if (a.n_blocks <= 0 || a.n_cand <= 0) return hipSuccess;
    if (a.n_cand > kIqCandsPerLaunch) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_iq_metric, dim3((unsigned)a.n_blocks, (unsigned)((a.n_cand + kIqCandTile - 1) / kIqCandTile)), dim3(64), 0, s, a);
    return hipGetLastError();
}

} // namespace iqgpu
