// lag.hpp -- the lag products R_d = sum x[n] conj(x[n - d]) per block of B frames of a stream on the device (include/iqgpu.h "lag
// products"): the device-side records and the argument blocks and launchers of k_lag_rows / k_lag_fold (lag.hip; host
// side lag.cpp).  Pages, columns, cells, the launch bound and the grid are iqgpu_env's (env.hpp) and are used here, not restated.
#pragma once
#include "chain.hpp"
#include "env.hpp"

namespace iqgpu {

constexpr int kLagMaxLags = 4, kLagMaxLag = 65536;
constexpr int kLagNear = kStatsColumns;                   // a partner at most this far back comes out of LDS, a farther one from memory
constexpr int kLagComps = 2 * kLagMaxLags + 1;            // component 0: the power (iqgpu_env's row_sum); 1 + 2 l, 2 + 2 l: re, im of lag l

// The open row on the device, per component: the columns of its open page and, for B > 65536, the total of its closed cells.  Two
// of these, read [cur] and written [cur ^ 1] by a launch (psd.hip's reason).
struct LagOpen {
    double col[kLagComps][kStatsColumns];
    double tot[kLagComps];
};
// a closed cell of a row of more than one (B > 65536)
struct LagCell { double v[kLagComps]; };

// k_lag_rows<format, lags compiled for>: the launch covers stream frames [first, first + n), raw[0] being frame `first`, dealt in pages
// exactly as k_env_rows'.  hist holds the max_lag frames in front of `first` as raw bytes, hist[k] being stream frame first - max_lag
// + k (those of a negative index are never read).  B <= 65536: the rows that END in (first, first + n] are stored at
// row - (first >> log2_b): row_lag[row][n_lags][2], row_sum[row] (device memory; either may be NULL).  B > 65536: closed pages leave a
// LagCell at cells[page - (first >> 16)].
struct LagRowsArgs {
    const void *raw, *hist;
    int64_t first, n;
    int32_t fmt, log2_b, pages_per_group, n_lags;
    int32_t lags[kLagMaxLags], max_lag;
    const LagOpen *open_in; LagOpen *open_out;
    LagCell *cells;
    float *row_lag, *row_sum;
    uint32_t *nonfinite;          // [groups], cf32 only
};
hipError_t launch_lag_rows(const LagRowsArgs &a, hipStream_t s);

// k_lag_fold: k_env_fold for the 2 n_lags + 1 components.
struct LagFoldArgs {
    const uint32_t *nonfinite; int32_t n_groups; uint64_t *nonfinite_total;
    const LagCell *cells; int32_t log2_cells_per_row, n_lags;       // cells == NULL: no rows to fold
    int64_t c0, n_closed, n_touched, rows_before;
    const LagOpen *open_in; LagOpen *open_out;
    float *row_lag, *row_sum;
};
hipError_t launch_lag_fold(const LagFoldArgs &a, hipStream_t s);

} // namespace iqgpu
