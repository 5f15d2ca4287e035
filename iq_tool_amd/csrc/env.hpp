// env.hpp -- power, peak and rail count per block of B frames of a stream on the device (include/iqgpu.h "envelope"):
// the geometry, the device-side records and the argument blocks and launchers of k_env_rows / k_env_fold (env.hip; host side env.cpp).
// The summation order is iqgpu_stats' applied per row: its constants and its host tree (stats.hpp) are used here, not restated.
#pragma once
#include "chain.hpp"
#include "stats.hpp"

namespace iqgpu {

constexpr int kEnvLog2BlockMin = 6, kEnvLog2BlockMax = 24, kEnvLog2BlockDefault = 12;
constexpr int kEnvLog2Columns = 10, kEnvLog2CellFrames = 16;
static_assert((1 << kEnvLog2Columns) == kStatsColumns && (1 << kEnvLog2CellFrames) == kStatsPageFrames, "one order: iqgpu_stats'");
constexpr int kEnvThreads = 256;
// A PAGE is what one workgroup walks in steps of kStatsColumns frames, thread t on columns 4 t .. 4 t + 3: the row's cell for
// B >= 1024 (B frames up to 65536, then 65536), and for B < 1024 one step of 1024 frames that holds 1024 / B whole rows.
inline int env_log2_page(int log2_b)
{
    return log2_b < kEnvLog2Columns ? kEnvLog2Columns : log2_b > kEnvLog2CellFrames ? kEnvLog2CellFrames : log2_b;
}
// A launch: at most 2^28 frames of whole pages (env.cpp cuts longer pushes: a workgroup's 32-bit counters cannot wrap, the cell
// buffer holds kEnvMaxCells), dealt in runs of consecutive pages to at most kEnvMaxGroups workgroups.
constexpr int kEnvLog2LaunchFrames = 28;
constexpr int kEnvMaxGroups = 2048;
constexpr int kEnvMaxCells = 1 << (kEnvLog2LaunchFrames - kEnvLog2CellFrames);

// The open row on the device: the columns of its open page (B < 1024: of the open step, whose finished rows have left), and for
// B > 65536 the total of its closed cells.  Two of these, read [cur] and written [cur ^ 1] by a launch (psd.hip's reason).
struct EnvOpen {
    double col_sum[kStatsColumns], col_peak[kStatsColumns];
    uint32_t col_rail[kStatsColumns];
    double tot_sum, tot_peak;
    uint32_t tot_rail, pad;
};
// a closed cell of a row of more than one (B > 65536)
struct EnvCell { double sum, peak; uint32_t rail, pad; };

// k_env_rows<format>: the launch covers stream frames [first, first + n), raw[0] being frame `first`.  Workgroup b takes pages
// (first >> lp) + b * pages_per_group ...; the page that begins in front of `first` starts from open_in, the one that does not end
// with the launch goes to open_out.  B <= 65536: the rows that END in (first, first + n] are stored at row - (first >> log2_b) of the
// planes given (device memory; any may be NULL).  B > 65536: closed pages leave an EnvCell at cells[page - (first >> 16)].
struct EnvRowsArgs {
    const void *raw;
    int64_t first, n;
    int32_t fmt, log2_b, pages_per_group;
    const EnvOpen *open_in; EnvOpen *open_out;
    EnvCell *cells;
    float *row_sum, *row_peak; uint32_t *row_rail;
    uint32_t *nonfinite;          // [groups], cf32 only
};
hipError_t launch_env_rows(const EnvRowsArgs &a, hipStream_t s);

// k_env_fold: *nonfinite_total += the groups' counts (n_groups > 0: cf32), and for B > 65536 the rows of the launch: row r of the
// stream is ((0.0 + cell 0) + cell 1) + ... over its cells, the cells in front of the launch in open_in's total; a row whose last
// cell closed in the launch goes to the planes at r - rows_before, the row left open to open_out's total.
struct EnvFoldArgs {
    const uint32_t *nonfinite; int32_t n_groups; uint64_t *nonfinite_total;
    const EnvCell *cells; int32_t log2_cells_per_row;      // cells == NULL: no rows to fold
    int64_t c0, n_closed, n_touched, rows_before;         // first cell the launch touched; how many it closed / touched
    const EnvOpen *open_in; EnvOpen *open_out;
    float *row_sum, *row_peak; uint32_t *row_rail;
};
hipError_t launch_env_fold(const EnvFoldArgs &a, hipStream_t s);

// the groups a launch over [first, first + n) is dealt to, and the pages of each
inline void env_grid(int64_t first, int64_t n, int log2_b, int *groups, int *pages_per_group)
{
    const int lp = env_log2_page(log2_b);
    const int64_t pages = ((first + n - 1) >> lp) - (first >> lp) + 1;
    const int64_t ppg = (pages + kEnvMaxGroups - 1) / kEnvMaxGroups;
    *pages_per_group = (int)ppg; *groups = (int)((pages + ppg - 1) / ppg);
}

// the bounds a launch of k_env_rows or k_lag_rows keeps (the cell buffer's, the counters': the host cuts longer pushes); *groups: its workgroups
inline bool env_rows_launch_ok(int64_t first, int64_t n, int log2_b, int fmt, int pages_per_group, const void *cells, const void *nonfinite,
                               int *groups)
{
    int ppg = 0;
    env_grid(first, n, log2_b, groups, &ppg);
    const int lp = env_log2_page(log2_b);
    const int64_t pages = ((first + n - 1) >> lp) - (first >> lp) + 1;
    return !(first < 0 || log2_b < kEnvLog2BlockMin || log2_b > kEnvLog2BlockMax || pages > ((int64_t)1 << (kEnvLog2LaunchFrames - lp)) ||
             ppg != pages_per_group || (log2_b > kEnvLog2CellFrames && !cells) || (fmt == IQGPU_FMT_CF32 && !nonfinite));
}

} // namespace iqgpu
