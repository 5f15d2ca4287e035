// sgram.hip -- the kernels of the row accumulator (include/iqgpu.h "spectrogram"; host side sgram.cpp).
//   k_sgram_cells  one workgroup of nfft / 16 threads per CELL (sgram.hpp): k_psd_pages' segment loop over the cell's segments that lie
//                  in the launch -- 16 points a thread from the logical stream, psd_unpack / gain / window, fft16_lds, the powers of bins
//                  tid + r nfft / 16 into double acc[16], float pk[16] in registers.  A cell that is a whole row (R <= 32) and ends in
//                  the launch is rounded once and stored straight into the caller's planes -- also when it began in an earlier push:
//                  its registers then start from the open cell and hold the whole row all the same.  Each of a thread's 16 stores
//                  per plane is one run of consecutive floats across the wave's lanes.  Any other cell that ends in
//                  the launch goes to its slot of the cell buffer, the one that does not to the OTHER open-cell buffer.  No atomics.
//   k_sgram_fold   R > 32: one thread per (row, bin) adds a row's cells in cell order, behind the open row's total where the row began
//                  before the launch; finished rows are rounded once into the caller's planes, the open row's total goes to the other
//                  total buffer.
// Ordering: the argument of psd.hip, for the open cell and the open total alike -- two buffers each, and the host flips cur behind
// every launch.  Within a launch every address is read only or written by exactly one workgroup (cells) or thread (fold).
#include <hip/hip_runtime.h>

#include "fft16.hpp"
#include "psd_stream.hpp"
#include "sgram.hpp"

namespace iqgpu {

template <int LOG2N, int FMT>
__global__ __launch_bounds__((1 << LOG2N) / 16) void k_sgram_cells(const SgramCellsArgs a)
{
    constexpr int N = 1 << LOG2N, T = N / 16, G = kPsdPageSegments;
    __shared__ cf2 X[N + (N >> 5) + 2];
    const int tid = threadIdx.x;
    const int64_t g = a.g0 + (int64_t)blockIdx.x;
    const int64_t row = g / a.C, c = g - row * a.C;
    const int64_t cell_beg = row * a.R + c * G;
    const int64_t cell_end = (c + 1) * G < a.R ? cell_beg + G : (row + 1) * a.R;
    const int64_t seg_end = a.seg0 + a.n_seg;
    const int64_t sbeg = cell_beg > a.seg0 ? cell_beg : a.seg0;
    const int64_t send = cell_end < seg_end ? cell_end : seg_end;
    const bool from_open = cell_beg < a.seg0, closed = cell_end <= seg_end;

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

    if (closed && a.C == 1) {                       // the cell is the row
        const int64_t at = (row - a.r0) * N + tid;
        if (a.row_sum) {
#pragma unroll
            for (int r = 0; r < 16; ++r) a.row_sum[at + r * T] = (float)acc[r];
        }
        if (a.row_pk) {
#pragma unroll
            for (int r = 0; r < 16; ++r) a.row_pk[at + r * T] = pk[r];
        }
        return;
    }
    double *dsum = closed ? a.cell_sum + (int64_t)blockIdx.x * N : a.open_sum_out;
    float *dpk = closed ? a.cell_pk + (int64_t)blockIdx.x * N : a.open_pk_out;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dsum[tid + r * T] = acc[r]; dpk[tid + r * T] = pk[r]; }
}

hipError_t launch_sgram_cells(const SgramCellsArgs &a, hipStream_t s)
{
    if (a.n_seg <= 0) return hipSuccess;
    if (a.R < 1 || a.C != sgram_cells_per_row(a.R) || a.g0 != sgram_cell_of(a.seg0, a.R) || a.r0 != a.seg0 / a.R) return hipErrorInvalidValue;
    const int64_t cells = sgram_cell_of(a.seg0 + a.n_seg - 1, a.R) - a.g0 + 1;
    // (the bounds of the cell buffer and of the grid: sgram.cpp cuts longer pushes)
    if (a.C == 1 ? cells > kSgramDirectCells : cells * ((int64_t)1 << a.log2n) > kSgramCellBufBins) return hipErrorInvalidValue;
    return psd_dispatch(a.log2n, a.fmt, [&](auto L, auto F) {
        hipLaunchKernelGGL((k_sgram_cells<decltype(L)::value, decltype(F)::value>), dim3((unsigned)cells), dim3((1u << decltype(L)::value) / 16), 0, s, a);
    });
}

__global__ __launch_bounds__(256) void k_sgram_fold(const SgramFoldArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    const int64_t j = i / a.nfft;
    const int k = (int)(i - j * a.nfft);
    if (j >= a.n_rows) return;
    const int64_t row = a.r0 + j;
    const bool from_open = j == 0 && a.has_tot_in;
    double t = from_open ? a.tot_sum_in[k] : 0.0;
    float m = from_open ? a.tot_pk_in[k] : 0.0f;
    const int64_t lo = row * a.C > a.g0 ? row * a.C : a.g0;
    const int64_t hi = (row + 1) * a.C < a.g0 + a.n_closed ? (row + 1) * a.C : a.g0 + a.n_closed;
    const double *cs = a.cell_sum + k;
    const float *cp = a.cell_pk + k;
#pragma unroll 8
    for (int64_t g = lo; g < hi; ++g) {
        t += cs[(g - a.g0) * a.nfft];
        m = fmaxf(m, cp[(g - a.g0) * a.nfft]);
    }
    if ((row + 1) * a.R <= a.seg_end) {
        if (a.row_sum) a.row_sum[j * a.nfft + k] = (float)t;
        if (a.row_pk) a.row_pk[j * a.nfft + k] = m;
    } else {
        a.tot_sum_out[k] = t;
        a.tot_pk_out[k] = m;
    }
}

hipError_t launch_sgram_fold(const SgramFoldArgs &a, hipStream_t s)
{
    if (a.n_rows <= 0) return hipSuccess;
    const int64_t threads = (int64_t)a.n_rows * a.nfft;
    hipLaunchKernelGGL(k_sgram_fold, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace iqgpu
