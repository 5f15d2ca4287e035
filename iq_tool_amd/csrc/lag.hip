// lag.hip -- the kernels of the lag-product accumulator (include/iqgpu.h "lag products"; host side lag.cpp).
//   k_lag_rows  k_env_rows' sibling (env.hip): the same pages dealt in runs to workgroups of 256 threads, the same steps of 1024
//               frames with thread t on frames / columns 4 t .. 4 t + 3 through capture_load.hpp, the same trees (pair_tree.hpp) and
//               the same three ways out of a page (rows inside a wave, the page as the row, the page as a cell).  A column holds
//               2 n_lags + 1 double sums: the power (iqgpu_env's row_sum term) and re / im of every lag.  New is the partner
//               x[n - d] of a frame:
//                 d <= 1024  out of LDS.  The workgroup keeps the unpacked frames of three steps (3 x 8 KiB; the step being filled,
//                            the one in front of it, and the one slow waves may still read: one barrier per step instead of two),
//                            frame o of a step at word (o & 3) * 256 + (o >> 2), so that the 64 lanes of a wave write and read
//                            consecutive words.  The step in front of a workgroup's first is loaded once more: from raw, or, in
//                            front of the launch, from the handle's history.
//                 d > 1024   a second load of raw at n - d, of the history in front of the launch.
//               All arithmetic in plain C++ with __dmul_rn / __dadd_rn / __dsub_rn; plain stores into slots of their own; no atomics.
//               Instantiated for 1 lag and for up to 4, so that one lag does not pay for the columns of four.  The build reports
//               (-Rpass-analysis=kernel-resource-usage, cs16; the other formats within 20 VGPRs): 1 lag 91 VGPRs, 5 waves per SIMD;
//               4 lags 192 VGPRs, 2 waves per SIMD; no scratch, 24.7 KB of LDS.  Two waves hide little: four near lags cost 5.2
//               times k_env_rows on the same bytes where one costs 1.55 times (profiles/lag.md).
//   k_lag_fold  k_env_fold's shape: the non-finite count of a cf32 launch, and for B > 65536 a thread per row adding its cells in order.
#include <hip/hip_runtime.h>

#include "capture_load.hpp"
#include "lag.hpp"
#include "pair_tree.hpp"

namespace iqgpu {

namespace {

__device__ __forceinline__ bool finite2(cf2 x) { return fabsf(x.x) < __builtin_inff() && fabsf(x.y) < __builtin_inff(); }

// where frame o of a step lies in its LDS slot
__device__ __forceinline__ int ring_at(int o) { return ((o & 3) << 8) | (o >> 2); }

// stream frame m, unpacked: from raw at or behind the launch's first frame, from the history in front of it.  The caller has
// checked first - max_lag <= m < first + n and m >= 0
template <int FMT> __device__ __forceinline__ cf2 fetch(const LagRowsArgs &a, int64_t m)
{
    int ci, cq; cf2 x;
    if (m >= a.first) load_one<FMT>(a.raw, m - a.first, a.fmt, ci, cq, x);
    else load_one<FMT>(a.hist, m - a.first + a.max_lag, a.fmt, ci, cq, x);
    return x;
}
template <int FMT> __device__ __forceinline__ cf2 fetch_or_zero(const LagRowsArgs &a, int64_t m)
{
    if (m < 0 || m < a.first - a.max_lag || m >= a.first + a.n) return cf2{0.0f, 0.0f};     // (never read as a partner)
    return fetch<FMT>(a, m);
}

template <int M> __device__ __forceinline__ void level(double &v) { v = __dadd_rn(v, pair_f64<M>(v)); }

} // namespace

template <int FMT, int NL>
__global__ __launch_bounds__(kEnvThreads) void k_lag_rows(const LagRowsArgs a)
{
    constexpr int C = kStatsColumns, NC = 2 * NL + 1;              // component 0: the power; 1 + 2 l, 2 + 2 l: re, im of lag l
    __shared__ cf2 ring[3 * C];
    __shared__ double W[4][NC];
    __shared__ uint32_t Wn[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lb = a.log2_b, lp = lb < kEnvLog2Columns ? kEnvLog2Columns : lb > kEnvLog2CellFrames ? kEnvLog2CellFrames : lb;      // (env_log2_page)
    const int64_t P = (int64_t)1 << lp;
    const int64_t end = a.first + a.n, page_first = a.first >> lp, page_last = (end - 1) >> lp;
    const int64_t pg0 = page_first + (int64_t)blockIdx.x * a.pages_per_group;
    const int64_t pg1 = pg0 + a.pages_per_group - 1 < page_last ? pg0 + a.pages_per_group - 1 : page_last;
    const int64_t rows_before = a.first >> lb;
    const int bps = frame_bytes(FMT >= 0 ? FMT : a.fmt);
    const int nl = a.n_lags < NL ? a.n_lags : NL, nc = 2 * nl + 1;
    const bool near = a.lags[0] <= kLagNear;                       // (uniform) some partner comes out of LDS

    uint32_t nonfinite = 0;
    int slot = 1, prev = 0;                                        // the LDS slots of this step and of the one in front
    bool primed = false;
    for (int64_t pg = pg0; pg <= pg1; ++pg) {
        const int64_t base = pg << lp;
        const int64_t fbeg = base > a.first ? base : a.first, fend = base + P < end ? base + P : end;
        const bool from_open = base < a.first, closed = base + P <= end;
        double s[NC][4];
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j) s[c][j] = from_open && c < nc ? a.open_in->col[c][4 * tid + j] : 0.0;

        const int r0 = (int)((fbeg - base) / C), r1 = (int)((fend - base + C - 1) / C);
        for (int r = r0; r < r1; ++r) {
            const int64_t S = base + (int64_t)r * C;                 // stream index of the step's first frame
            const int64_t i0 = S + 4 * tid;                          // ... of the thread's first frame of the step
            const int64_t j0 = i0 - a.first;                         // ... its index in raw
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

            if (near) {
                if (!primed) {
                    // the step in front of the workgroup's first: once more from raw, or from the history
#pragma unroll
                    for (int k = 0; k < 4; ++k) ring[prev * C + ring_at(4 * tid + k)] = fetch_or_zero<FMT>(a, i0 - C + k);
                    primed = true;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)                          // (a frame of the step in front of the launch: the history's)
                    ring[slot * C + ring_at(4 * tid + k)] = ok[k] ? x[k] : i0 + k < a.first ? fetch_or_zero<FMT>(a, i0 + k) : cf2{0.0f, 0.0f};
                __syncthreads();
            }

#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!ok[k]) continue;
                const cf2 u = x[k];
                if constexpr (FMT == IQGPU_FMT_CF32) {
                    if (!finite2(u)) { ++nonfinite; continue; }
                }
                const double ure = (double)u.x, uim = (double)u.y;
                s[0][k] = __dadd_rn(s[0][k], __dadd_rn(__dmul_rn(ure, ure), __dmul_rn(uim, uim)));      // iqgpu_env's term
#pragma unroll
                for (int l = 0; l < NL; ++l) {
                    if (l >= nl) continue;
                    const int d = a.lags[l];
                    const int64_t i = i0 + k;
                    if (i < d) continue;                             // no partner: no term
                    cf2 b;
                    if (d <= kLagNear) {
                        const int po = 4 * tid + k - d;
                        b = po >= 0 ? ring[slot * C + ring_at(po)] : ring[prev * C + ring_at(po + C)];
                    } else {
                        b = fetch<FMT>(a, i - d);
                    }
                    if constexpr (FMT == IQGPU_FMT_CF32) {
                        if (!finite2(b)) continue;
                    }
                    const double bre = (double)b.x, bim = (double)b.y;
                    s[1 + 2 * l][k] = __dadd_rn(s[1 + 2 * l][k], __dadd_rn(__dmul_rn(ure, bre), __dmul_rn(uim, bim)));
                    s[2 + 2 * l][k] = __dadd_rn(s[2 + 2 * l][k], __dsub_rn(__dmul_rn(uim, bre), __dmul_rn(ure, bim)));
                }
            }
            prev = slot; slot = slot == 2 ? 0 : slot + 1;
        }

        if (!closed) {
#pragma unroll
            for (int c = 0; c < NC; ++c)
                if (c < nc) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) a.open_out->col[c][4 * tid + j] = s[c][j];
                }
        }
        if (lb >= kEnvLog2Columns && !closed) continue;               // (uniform: the page is the workgroup's)

        // the tree of adjacent pairs per component: two levels in the thread, up to six across the wave, up to two across the waves
        double v[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            v[c] = __dadd_rn(__dadd_rn(s[c][0], s[c][1]), __dadd_rn(s[c][2], s[c][3]));
            level<1>(v[c]); level<2>(v[c]); level<4>(v[c]); level<8>(v[c]);                           // B >= 64: 16 lanes at least
            if (lb >= 7) level<16>(v[c]);
            if (lb >= 8) level<32>(v[c]);
        }
        if (lb <= 8) {
            // rows inside a wave: the first lane of each stores the rows that end in this launch
            const int lanes = 1 << (lb - 2);
            const int64_t row = (base + 4 * tid) >> lb, row_end = (row + 1) << lb;
            if ((lane & (lanes - 1)) == 0 && row_end > a.first && row_end <= end) {
                if (a.row_sum) a.row_sum[row - rows_before] = __double2float_rn(v[0]);
                if (a.row_lag) {
#pragma unroll
                    for (int c = 1; c < NC; ++c)
                        if (c < nc) a.row_lag[(row - rows_before) * (nc - 1) + (c - 1)] = __double2float_rn(v[c]);
                }
            }
            continue;
        }
        if (lane == 0) {
#pragma unroll
            for (int c = 0; c < NC; ++c) W[wave][c] = v[c];
        }
        __syncthreads();
        if (lb == 9) {
            if (tid == 0 || tid == 128) {
                const int64_t row = (base + 4 * tid) >> lb, row_end = (row + 1) << lb;
                if (row_end > a.first && row_end <= end) {
                    for (int c = 0; c < nc; ++c) {
                        const float f = __double2float_rn(__dadd_rn(W[wave][c], W[wave + 1][c]));
                        if (c == 0) { if (a.row_sum) a.row_sum[row - rows_before] = f; }
                        else if (a.row_lag) a.row_lag[(row - rows_before) * (nc - 1) + (c - 1)] = f;
                    }
                }
            }
        } else if (tid == 0) {
            for (int c = 0; c < nc; ++c) {
                const double sum = __dadd_rn(__dadd_rn(W[0][c], W[1][c]), __dadd_rn(W[2][c], W[3][c]));
                if (lb <= kEnvLog2CellFrames) {                       // the page is row pg
                    if (c == 0) { if (a.row_sum) a.row_sum[pg - rows_before] = __double2float_rn(sum); }
                    else if (a.row_lag) a.row_lag[(pg - rows_before) * (nc - 1) + (c - 1)] = __double2float_rn(sum);
                } else {
                    a.cells[pg - page_first].v[c] = sum;
                }
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

hipError_t launch_lag_rows(const LagRowsArgs &a, hipStream_t s)
{
    if (a.n <= 0) return hipSuccess;
    int groups = 0;
    // (env's bounds, and the history's: lag.cpp keeps max_lag frames)
    if (!env_rows_launch_ok(a.first, a.n, a.log2_b, a.fmt, a.pages_per_group, a.cells, a.nonfinite, &groups) || !a.hist ||
        a.n_lags < 1 || a.n_lags > kLagMaxLags || a.max_lag != a.lags[a.n_lags - 1])
        return hipErrorInvalidValue;
    for (int l = 0; l < a.n_lags; ++l)
        if (a.lags[l] < 1 || a.lags[l] > kLagMaxLag || (l && a.lags[l] <= a.lags[l - 1])) return hipErrorInvalidValue;
    const dim3 g((unsigned)groups), b(kEnvThreads);
    if (a.n_lags == 1) return page_dispatch(a.fmt, [&](auto F) { hipLaunchKernelGGL((k_lag_rows<decltype(F)::value, 1>), g, b, 0, s, a); });
    return page_dispatch(a.fmt, [&](auto F) { hipLaunchKernelGGL((k_lag_rows<decltype(F)::value, kLagMaxLags>), g, b, 0, s, a); });
}

__global__ __launch_bounds__(kEnvThreads) void k_lag_fold(const LagFoldArgs a)
{
    __shared__ uint64_t W[kEnvThreads];
    const int tid = threadIdx.x;
    fold_nonfinite<kEnvThreads>(a.nonfinite, a.n_groups, a.nonfinite_total, W);
    if (!a.cells) return;
    const int lc = a.log2_cells_per_row, nc = 2 * a.n_lags + 1;
    const int64_t r_first = a.c0 >> lc, r_last = (a.c0 + a.n_touched - 1) >> lc, c_end = a.c0 + a.n_closed;
    for (int64_t r = r_first + tid; r <= r_last; r += kEnvThreads) {
        const int64_t row_c0 = r << lc, row_c1 = (r + 1) << lc;
        const bool carried = row_c0 < a.c0;                           // cells of the row lie in front of the launch
        const int64_t c_lo = carried ? a.c0 : row_c0, c_hi = row_c1 < c_end ? row_c1 : c_end;
        for (int c = 0; c < nc; ++c) {
            double sum = carried ? a.open_in->tot[c] : 0.0;
            for (int64_t k = c_lo; k < c_hi; ++k) sum = __dadd_rn(sum, a.cells[k - a.c0].v[c]);
            if (row_c1 <= c_end) {
                if (c == 0) { if (a.row_sum) a.row_sum[r - a.rows_before] = __double2float_rn(sum); }
                else if (a.row_lag) a.row_lag[(r - a.rows_before) * (nc - 1) + (c - 1)] = __double2float_rn(sum);
            } else {
                a.open_out->tot[c] = sum;
            }
        }
    }
}

hipError_t launch_lag_fold(const LagFoldArgs &a, hipStream_t s)
{
    if (a.n_groups < 0 || a.n_groups > kEnvMaxGroups || a.n_lags < 1 || a.n_lags > kLagMaxLags ||
        (a.cells && (a.n_touched < 1 || a.n_touched > kEnvMaxCells || a.n_closed > a.n_touched)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_lag_fold, dim3(1), dim3(kEnvThreads), 0, s, a);
    return hipGetLastError();
}

} // namespace iqgpu
