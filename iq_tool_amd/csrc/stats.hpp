// stats.hpp -- capture statistics of a stream on the device (include/iqgpu.h "capture statistics"): the geometry, the
// device-side records and the argument blocks and launchers of k_stats_pages / k_stats_fold (stats.hip; host side stats.cpp).
#pragma once
#include "chain.hpp"

namespace iqgpu {

// Frames of one page, and the columns a page's five double sums are kept in (column = index in the page mod kStatsColumns).  The columns
// are what lets a page continue at ANY frame: a thread of k_stats_pages owns four adjacent columns for the whole page, so a page cut
// between two pushes is the same per-column sequence of additions as an uncut one.  1024 = 256 threads x 4 frames: one row of a page is
// one 16-byte load a lane at cs16.  A closed page costs 40 bytes (five doubles) against 65536 frames read.
constexpr int kStatsPageFrames = 1 << 16;
constexpr int kStatsColumns = 1024;
constexpr int kStatsThreads = 256;
// A launch: at most kStatsMaxPages pages (2^28 frames; stats.cpp cuts longer pushes), dealt in runs of consecutive pages to at most
// kStatsMaxGroups workgroups.  A workgroup's share is then at most 4 pages = 2^18 frames: its 32-bit LDS and register counters
// (2 components a frame) cannot wrap.
constexpr int kStatsMaxPages = 4096;
constexpr int kStatsMaxGroups = 1024;
// The LDS histogram of a workgroup: [2][256] bins in kStatsSlices copies, lane l adds to copy l mod 16, the copy index in the low
// address bits (word = (c * 256 + bin) * 16 + slice).  A wave's 64 adds to ONE bin (digital silence, a clipped capture) then fall on 16
// banks, 4 lanes an address, instead of 64 lanes on one; adds to different bins meet two-way at most.  32 KiB a workgroup.
constexpr int kStatsSlices = 16;

// what one workgroup leaves, order-free: everything of its frames that merges exactly (hist apart, [groups][512] uint32)
struct StatsPartial {
    uint32_t rail_lo[2], rail_hi[2], nonfinite, finite;
    float mn[2], mx[2];           // +inf / -inf without a finite frame
    double pk; uint64_t pkf;      // pk < 0 without a finite frame
};

// the handle's totals on the device; finite: frames that entered the sums
struct StatsTotals {
    uint64_t hist[512];
    uint64_t rail_lo[2], rail_hi[2], nonfinite, finite;
    double pk; uint64_t pkf;
    double sum[5];                // sum I, sum Q, sum_sq I, sum_sq Q, sum_iq: the closed pages in page order
    float mn[2], mx[2];
};

// k_stats_pages<format>: the launch covers stream frames [first, first + n), raw[0] being frame `first`.  Workgroup b takes pages
// first / P + b * pages_per_group ... ; the page that begins in front of `first` starts from open_in, the one that does not end with
// the launch goes to open_out ([5][kStatsColumns] doubles each; never the same memory: psd.hip's reason).  Closed pages leave their
// five sums at page_sum[page - first / P].
struct StatsPagesArgs {
    const void *raw;
    int64_t first, n;
    int32_t fmt, pages_per_group;
    const double *open_in; double *open_out;
    uint32_t *hist;               // [groups][512]
    StatsPartial *part;           // [groups]
    double *page_sum;             // [pages of the launch][5]
};
hipError_t launch_stats_pages(const StatsPagesArgs &a, hipStream_t s);

// k_stats_fold: totals += the partials of a launch (integer adds, min / max, the earlier of equal peaks), sum[k] += page_sum[p][k]
// for the launch's closed pages p = 0 .. n_pages - 1 in that order
struct StatsFoldArgs {
    const uint32_t *hist; const StatsPartial *part; const double *page_sum;
    int32_t groups, n_pages;
    StatsTotals *tot;
};
hipError_t launch_stats_fold(const StatsFoldArgs &a, hipStream_t s);

// the groups a launch over [first, first + n) is dealt to, and the pages of each
inline void stats_grid(int64_t first, int64_t n, int *groups, int *pages_per_group)
{
    const int64_t P = kStatsPageFrames, pages = (first + n - 1) / P - first / P + 1;
    const int64_t ppg = (pages + kStatsMaxGroups - 1) / kStatsMaxGroups;
    *pages_per_group = (int)ppg; *groups = (int)((pages + ppg - 1) / ppg);
}

// the fixed tree over a page's column sums, on the host: iqgpu_stats_read folds the open page with it (the device's: stats.hip)
inline double stats_tree(const double *col)
{
    double t[kStatsColumns];
    for (int i = 0; i < kStatsColumns; ++i) t[i] = col[i];
    for (int n = kStatsColumns / 2; n >= 1; n /= 2)
        for (int i = 0; i < n; ++i) t[i] = t[2 * i] + t[2 * i + 1];
    return t[0];
}

} // namespace iqgpu
