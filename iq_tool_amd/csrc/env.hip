// env.hip -- the kernels of the envelope accumulator (include/iqgpu.h "envelope"; host side env.cpp).
//   k_env_rows  one workgroup of 256 threads per run of consecutive PAGES (env.hpp).  A step of a page is 1024 frames: thread t takes
//               frames 4 t .. 4 t + 3 of every step with k_stats_pages' loads (capture_load.hpp) and so owns columns 4 t .. 4 t + 3,
//               each with its sum and peak in double and its rail count.  What leaves a page depends on B alone:
//                 B < 1024            the page is one step and holds 1024 / B rows, a column holds one term.  The row is the tree of
//                                     adjacent pairs over its B terms: two levels in the thread, then pair adds across B / 4 lanes --
//                                     DPP for the partners 1, 2, 4 and 8 lanes away, xor-shuffles for 16 and 32, the two waves of a
//                                     B = 512 row through LDS -- and the row's first lane stores it.
//                 1024 <= B <= 65536  the page is the row: the ten-level tree over the 1024 columns, thread 0 stores the row.
//                 B > 65536           the page is a cell of the row: the same tree, thread 0 stores an EnvCell for k_env_fold.
//               The stream's open page starts from and returns to the handle's open columns, in TWO buffers flipped behind the launch
//               (psd.hip's reason).  Everything leaves as plain stores into slots of its own; no atomics.
//   k_env_fold  one workgroup: the non-finite count of a cf32 launch, and for B > 65536 a thread per row adding its cells in order.
#include <hip/hip_runtime.h>

#include "capture_load.hpp"
#include "env.hpp"
#include "pair_tree.hpp"

namespace iqgpu {

namespace {

// one level of the tree for the three values of a row: the sum's pair add, and the two order-free ones
template <int M> __device__ __forceinline__ void level(double &s, float &pk, uint32_t &rl)
{
    s = __dadd_rn(s, pair_f64<M>(s));             // (both lanes of a pair hold the pair's sum: a + b == b + a)
    pk = fmaxf(pk, pair_f32<M>(pk));
    rl += (uint32_t)pair_i32<M>((int)rl);
}

// one frame into its column
template <int FMT>
__device__ __forceinline__ void take(int fmt, int ci, int cq, cf2 x, double &s, double &pk, uint32_t &rl, uint32_t &nonfinite)
{
    uint32_t rails;
    if constexpr (FMT == IQGPU_FMT_CF32) {
        if (!(fabsf(x.x) < __builtin_inff() && fabsf(x.y) < __builtin_inff())) { ++nonfinite; return; }
        rails = rails_of_floats(x.x, x.y);
    } else {
        rails = rails_of_codes(FMT >= 0 ? FMT : fmt, ci, cq);
    }
    const double re = (double)x.x, im = (double)x.y;
    const double p = __dadd_rn(__dmul_rn(re, re), __dmul_rn(im, im));       // iqgpu_stats' peak_power term
    s = __dadd_rn(s, p);
    pk = p > pk ? p : pk;
    rl += rails;
}

} // namespace

template <int FMT>
__global__ __launch_bounds__(kEnvThreads) void k_env_rows(const EnvRowsArgs a)
{
    constexpr int C = kStatsColumns;
    __shared__ double Ws[4], Wp[4];
    __shared__ uint32_t Wr[4], Wn[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lb = a.log2_b, lp = lb < kEnvLog2Columns ? kEnvLog2Columns : lb > kEnvLog2CellFrames ? kEnvLog2CellFrames : lb;      // (env_log2_page)
    const int64_t P = (int64_t)1 << lp;
    const int64_t end = a.first + a.n, page_first = a.first >> lp, page_last = (end - 1) >> lp;
    const int64_t pg0 = page_first + (int64_t)blockIdx.x * a.pages_per_group;
    const int64_t pg1 = pg0 + a.pages_per_group - 1 < page_last ? pg0 + a.pages_per_group - 1 : page_last;
    const int64_t rows_before = a.first >> lb;
    const int bps = frame_bytes(FMT >= 0 ? FMT : a.fmt);

    uint32_t nonfinite = 0;
    for (int64_t pg = pg0; pg <= pg1; ++pg) {
        const int64_t base = pg << lp;
        const int64_t fbeg = base > a.first ? base : a.first, fend = base + P < end ? base + P : end;
        const bool from_open = base < a.first, closed = base + P <= end;
        double s[4], pk[4]; uint32_t rl[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            s[j] = from_open ? a.open_in->col_sum[4 * tid + j] : 0.0;
            pk[j] = from_open ? a.open_in->col_peak[4 * tid + j] : 0.0;
            rl[j] = from_open ? a.open_in->col_rail[4 * tid + j] : 0u;
        }

        const int r0 = (int)((fbeg - base) / C), r1 = (int)((fend - base + C - 1) / C);
        for (int r = r0; r < r1; ++r) {
            const int64_t i0 = base + (int64_t)r * C + 4 * tid;      // stream index of the thread's first frame of the step
            const int64_t j0 = i0 - a.first;                          // ... its index in raw
            int ci[4], cq[4]; cf2 x[4]; bool ok[4];
            bool four = false;
            if constexpr (vec_bytes<FMT>() != 0)
                four = i0 >= fbeg && i0 + 4 <= fend && (((uintptr_t)a.raw + (uintptr_t)(j0 * bps)) & (uintptr_t)(vec_bytes<FMT>() - 1)) == 0;
            if (four) {
                load_four<FMT>(a.raw, j0, ci, cq, x);
#pragma unroll
                for (int k = 0; k < 4; ++k) ok[k] = true;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    ok[k] = i0 + k >= fbeg && i0 + k < fend;
                    ci[k] = cq[k] = 0; x[k] = cf2{0.0f, 0.0f};
                    if (ok[k]) load_one<FMT>(a.raw, j0 + k, a.fmt, ci[k], cq[k], x[k]);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (ok[k]) take<FMT>(a.fmt, ci[k], cq[k], x[k], s[k], pk[k], rl[k], nonfinite);
        }

        if (!closed) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a.open_out->col_sum[4 * tid + j] = s[j]; a.open_out->col_peak[4 * tid + j] = pk[j]; a.open_out->col_rail[4 * tid + j] = rl[j];
            }
        }
        if (lb >= kEnvLog2Columns && !closed) continue;               // (uniform: the page is the workgroup's)

        // the tree of adjacent pairs: two levels in the thread, up to six across the wave, up to two across the waves.  The peak goes
        // on in float where it leaves as one: rounding is monotone, so the max of the rounded terms is the rounded max
        double v = __dadd_rn(__dadd_rn(s[0], s[1]), __dadd_rn(s[2], s[3]));
        const double pkd = fmax(fmax(pk[0], pk[1]), fmax(pk[2], pk[3]));
        float pf = __double2float_rn(pkd);
        uint32_t n = rl[0] + rl[1] + rl[2] + rl[3];
        level<1>(v, pf, n); level<2>(v, pf, n); level<4>(v, pf, n); level<8>(v, pf, n);               // B >= 64: 16 lanes at least
        if (lb >= 7) level<16>(v, pf, n);
        if (lb >= 8) level<32>(v, pf, n);
        if (lb <= 8) {
            // rows inside a wave: the first lane of each stores the rows that end in this launch
            const int lanes = 1 << (lb - 2);
            const int64_t row = (base + 4 * tid) >> lb, row_end = (row + 1) << lb;
            if ((lane & (lanes - 1)) == 0 && row_end > a.first && row_end <= end) {
                if (a.row_sum) a.row_sum[row - rows_before] = __double2float_rn(v);
                if (a.row_peak) a.row_peak[row - rows_before] = pf;
                if (a.row_rail) a.row_rail[row - rows_before] = n;
            }
            continue;
        }
        // (the double peak of a cell: the float above is the row's only)
        double pd = pkd;
        if (lb > kEnvLog2CellFrames) {
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) pd = fmax(pd, __shfl_xor(pd, m));
        }
        if (lane == 0) { Ws[wave] = v; Wp[wave] = lb > kEnvLog2CellFrames ? pd : (double)pf; Wr[wave] = n; }
        __syncthreads();
        if (lb == 9) {
            if (tid == 0 || tid == 128) {
                const int64_t row = (base + 4 * tid) >> lb, row_end = (row + 1) << lb;
                if (row_end > a.first && row_end <= end) {
                    if (a.row_sum) a.row_sum[row - rows_before] = __double2float_rn(__dadd_rn(Ws[wave], Ws[wave + 1]));
                    if (a.row_peak) a.row_peak[row - rows_before] = (float)fmax(Wp[wave], Wp[wave + 1]);
                    if (a.row_rail) a.row_rail[row - rows_before] = Wr[wave] + Wr[wave + 1];
                }
            }
        } else if (tid == 0) {
            const double sum = __dadd_rn(__dadd_rn(Ws[0], Ws[1]), __dadd_rn(Ws[2], Ws[3]));
            const double peak = fmax(fmax(Wp[0], Wp[1]), fmax(Wp[2], Wp[3]));
            const uint32_t rail = Wr[0] + Wr[1] + Wr[2] + Wr[3];
            if (lb <= kEnvLog2CellFrames) {                           // the page is row pg
                if (a.row_sum) a.row_sum[pg - rows_before] = __double2float_rn(sum);
                if (a.row_peak) a.row_peak[pg - rows_before] = (float)peak;
                if (a.row_rail) a.row_rail[pg - rows_before] = rail;
            } else {
                a.cells[pg - page_first] = EnvCell{sum, peak, rail, 0u};
            }
        }
        __syncthreads();
    }

    if constexpr (FMT == IQGPU_FMT_CF32) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) nonfinite += (uint32_t)__shfl_xor((int)nonfinite, m);
        if (lane == 0) Wn[wave] = nonfinite;
        __syncthreads();
        if (tid == 0) a.nonfinite[blockIdx.x] = Wn[0] + Wn[1] + Wn[2] + Wn[3];
    }
}

hipError_t launch_env_rows(const EnvRowsArgs &a, hipStream_t s)
{
    if (a.n <= 0) return hipSuccess;
    int groups = 0;
    if (!env_rows_launch_ok(a.first, a.n, a.log2_b, a.fmt, a.pages_per_group, a.cells, a.nonfinite, &groups)) return hipErrorInvalidValue;
    return page_dispatch(a.fmt, [&](auto F) { hipLaunchKernelGGL(k_env_rows<decltype(F)::value>, dim3((unsigned)groups), dim3(kEnvThreads), 0, s, a); });
}

__global__ __launch_bounds__(kEnvThreads) void k_env_fold(const EnvFoldArgs a)
{
    __shared__ uint64_t W[kEnvThreads];
    const int tid = threadIdx.x;
    fold_nonfinite<kEnvThreads>(a.nonfinite, a.n_groups, a.nonfinite_total, W);
    if (!a.cells) return;
    const int lc = a.log2_cells_per_row;
    const int64_t r_first = a.c0 >> lc, r_last = (a.c0 + a.n_touched - 1) >> lc, c_end = a.c0 + a.n_closed;
    for (int64_t r = r_first + tid; r <= r_last; r += kEnvThreads) {
        const int64_t row_c0 = r << lc, row_c1 = (r + 1) << lc;
        const bool carried = row_c0 < a.c0;                           // cells of the row lie in front of the launch
        double sum = carried ? a.open_in->tot_sum : 0.0, peak = carried ? a.open_in->tot_peak : 0.0;
        uint32_t rail = carried ? a.open_in->tot_rail : 0u;
        const int64_t c_lo = carried ? a.c0 : row_c0, c_hi = row_c1 < c_end ? row_c1 : c_end;
        for (int64_t c = c_lo; c < c_hi; ++c) {
            const EnvCell e = a.cells[c - a.c0];
            sum = __dadd_rn(sum, e.sum); peak = fmax(peak, e.peak); rail += e.rail;
        }
        if (row_c1 <= c_end) {
            if (a.row_sum) a.row_sum[r - a.rows_before] = __double2float_rn(sum);
            if (a.row_peak) a.row_peak[r - a.rows_before] = __double2float_rn(peak);
            if (a.row_rail) a.row_rail[r - a.rows_before] = rail;
        } else {
            a.open_out->tot_sum = sum; a.open_out->tot_peak = peak; a.open_out->tot_rail = rail;
        }
    }
}

hipError_t launch_env_fold(const EnvFoldArgs &a, hipStream_t s)
{
    if (a.n_groups < 0 || a.n_groups > kEnvMaxGroups || (a.cells && (a.n_touched < 1 || a.n_touched > kEnvMaxCells || a.n_closed > a.n_touched)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_env_fold, dim3(1), dim3(kEnvThreads), 0, s, a);
    return hipGetLastError();
}

} // namespace iqgpu
