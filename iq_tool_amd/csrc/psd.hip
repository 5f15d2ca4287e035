// psd.hip -- the kernels of the power-spectrum accumulator (include/iqgpu.h "power spectrum"; host side psd.cpp).
//   k_psd_pages   one workgroup of nfft / 16 threads per PAGE of kPsdPageSegments consecutive segments of the stream's grid.  Per
//                 segment, in stream order: 16 points a thread from the logical stream (the carry, then the pushed buffer: two bases
//                 and a split index), unpack / gain / window, fft16_lds<log2 nfft>; the thread then holds bins tid + r nfft / 16 and
//                 adds their powers to double acc[16], float pk[16] in registers.  A page that ends inside the launch goes to the page
//                 buffer, the stream's open page starts from and returns to the handle's open arrays.  No atomics.
//                 Ordering: the workgroups of a launch run in no defined order, and one launch may hold both the workgroup that
//                 STARTS from the open page (the first) and the one that LEAVES an open page (the last).  The open arrays are
//                 therefore two buffers: a launch reads open[cur] and writes open[cur ^ 1], and the host flips cur behind a launch
//                 that left an open page.  Within a launch every address is then either read only (input, carry, tables, open[cur])
//                 or written by exactly one workgroup (its page slot, or open[cur ^ 1] by the last); launches on one stream are ordered.
//   k_psd_fold    one thread per bin: total += page[p] for the launch's closed pages in page order, peak = max.
//   k_psd_carry   the trailing bytes a later segment still needs, into the other carry buffer.
// The sum of a bin is therefore (((0 + s0) + s1) + ...) over a page's segments and ((total + page0) + page1) + ... over the pages: an
// order that belongs to the stream, whatever the calls were.
#include <hip/hip_runtime.h>

#include "fft16.hpp"
#include "psd.hpp"
#include "psd_stream.hpp"

namespace iqgpu {

template <int LOG2N, int FMT>
__global__ __launch_bounds__((1 << LOG2N) / 16) void k_psd_pages(const PsdPagesArgs a)
{
    constexpr int N = 1 << LOG2N, T = N / 16, G = kPsdPageSegments;
    __shared__ cf2 X[N + (N >> 5) + 2];
    const int tid = threadIdx.x;
    const int64_t page = a.seg0 / G + (int64_t)blockIdx.x;
    const int64_t seg_end = a.seg0 + a.n_seg;
    const int64_t sbeg = page * G > a.seg0 ? page * G : a.seg0;
    const int64_t send = (page + 1) * G < seg_end ? (page + 1) * G : seg_end;
    const bool from_open = page * G < a.seg0, closed = (page + 1) * G <= seg_end;

    double acc[16];
    float pk[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        acc[r] = from_open ? a.open_sum_in[tid + r * T] : 0.0;
        pk[r] = from_open ? a.open_pk_in[tid + r * T] : 0.0f;
    }
    float w[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) w[r] = a.window[tid + r * T];

    for (int64_t s = sbeg; s < send; ++s) {
        const int64_t i0 = a.first + (s - a.seg0) * (int64_t)a.hop + tid;
        cf2 io[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t i = i0 + r * T;
            const bool old = i < a.split;
            const cf2 v = psd_unpack<FMT>(old ? a.carry : a.raw, old ? i : i - a.split, a.fmt, a.gain);
            io[r] = cf2{v.x * w[r], v.y * w[r]};
        }
        fft16_lds<LOG2N, true>(X, a.twiddle, tid, io);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __fadd_rn(__fmul_rn(io[r].x, io[r].x), __fmul_rn(io[r].y, io[r].y));
            acc[r] += (double)p;
            pk[r] = fmaxf(pk[r], p);
        }
    }

    double *dsum = closed ? a.page_sum + (int64_t)blockIdx.x * N : a.open_sum_out;
    float *dpk = closed ? a.page_pk + (int64_t)blockIdx.x * N : a.open_pk_out;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dsum[tid + r * T] = acc[r]; dpk[tid + r * T] = pk[r]; }
}

hipError_t launch_psd_pages(const PsdPagesArgs &a, hipStream_t s)
{
    if (a.n_seg <= 0) return hipSuccess;
    const int64_t G = kPsdPageSegments;
    const int64_t pages = (a.seg0 + a.n_seg - 1) / G - a.seg0 / G + 1;
    if (pages * ((int64_t)1 << a.log2n) > kPsdPageBufBins) return hipErrorInvalidValue;      // (the page buffer's bound: psd.cpp cuts longer pushes)
    return psd_dispatch(a.log2n, a.fmt, [&](auto L, auto F) {
        hipLaunchKernelGGL((k_psd_pages<decltype(L)::value, decltype(F)::value>), dim3((unsigned)pages), dim3((1u << decltype(L)::value) / 16), 0, s, a);
    });
}

__global__ __launch_bounds__(64) void k_psd_fold(const PsdFoldArgs a)
{
    const int k = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (k >= a.nfft) return;
    double t = a.total_sum[k];
    float m = a.total_pk[k];
    const double *ps = a.page_sum + k;
    const float *pp = a.page_pk + k;
#pragma unroll 16
    for (int p = 0; p < a.n_pages; ++p) {
        t += ps[(int64_t)p * a.nfft];
        m = fmaxf(m, pp[(int64_t)p * a.nfft]);
    }
    a.total_sum[k] = t;
    a.total_pk[k] = m;
}

hipError_t launch_psd_fold(const PsdFoldArgs &a, hipStream_t s)
{
    if (a.n_pages <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_psd_fold, dim3((unsigned)((a.nfft + 63) / 64)), dim3(64), 0, s, a);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_psd_carry(const PsdCarryArgs a)
{
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= a.bytes) return;
    const int64_t j = a.first + i;
    a.dst[i] = j < a.split_bytes ? a.carry[j] : a.raw[j - a.split_bytes];
}

hipError_t launch_psd_carry(const PsdCarryArgs &a, hipStream_t s)
{
    if (a.bytes <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_psd_carry, dim3((unsigned)((a.bytes + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace iqgpu
