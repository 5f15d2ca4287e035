// sgram.hpp -- time-resolved spectrum of a stream on the device (include/iqgpu.h "spectrogram"): the argument blocks and launchers of
// k_sgram_cells / k_sgram_fold (sgram.hip; host side sgram.cpp).  The segment grid, the unpack, the tables, the transform
// and the carry are the power spectrum's (psd.hpp, psd_stream.hpp).
#pragma once
#include "psd.hpp"

namespace iqgpu {

// Rows and cells.  Row r is segments [r R, (r + 1) R) of the stream's grid, R = row_segments.  A row is cut into C = ceil(R / G) cells
// of G = kPsdPageSegments consecutive segments counted from the row's first (the last may be short); cell c of row r has the stream-wide
// index g = r C + c.  A workgroup sums one cell in registers, exactly as k_psd_pages sums a page, so a row equals the power spectrum of
// its frames bit for bit: a fresh iqgpu_psd's pages are the row's cells.
inline int64_t sgram_cells_per_row(int64_t R) { return (R + kPsdPageSegments - 1) / kPsdPageSegments; }
inline int64_t sgram_cell_of(int64_t seg, int64_t R) { return seg / R * sgram_cells_per_row(R) + seg % R / kPsdPageSegments; }
// one past the last segment of cell g
inline int64_t sgram_cell_end(int64_t g, int64_t R)
{
    const int64_t C = sgram_cells_per_row(R), c = g % C, e = (c + 1) * kPsdPageSegments;
    return g / C * R + (e < R ? e : R);
}
// bins of the cell buffer (as kPsdPageBufBins bounds the page buffer: 48 MiB of doubles and floats); sgram.cpp cuts longer pushes into
// several launches.  Rows of one cell (R <= G) never touch it and are bounded by kSgramDirectCells workgroups a launch instead
constexpr int64_t kSgramCellBufBins = (int64_t)1 << 22;
constexpr int64_t kSgramDirectCells = (int64_t)1 << 24;

// k_sgram_cells<log2 nfft, format>: workgroup b sums the segments of cell g0 + b that lie in [seg0, seg0 + n_seg).  The logical stream
// of a launch is carry[0 .. split) followed by raw[0 ..), as for k_psd_pages: segment seg0 + j starts at logical frame first + j * hop.
struct SgramCellsArgs {
    const void *carry, *raw;
    int64_t split, first;
    int32_t fmt, log2n, hop;
    float gain;
    int64_t seg0, n_seg;          // stream index of the launch's first segment, segments of the launch (>= 1)
    int64_t R, C, g0, r0;         // row_segments, cells per row, the cell and the row seg0 lies in
    const float *window;
    const cf2 *twiddle;
    // the open cell, [nfft] each, in two buffers (the rule of PsdPagesArgs): the cell that begins in front of seg0 starts from *_in,
    // the one that does not end with the launch goes to *_out
    const double *open_sum_in; const float *open_pk_in;
    double *open_sum_out; float *open_pk_out;
    double *cell_sum; float *cell_pk;     // C > 1: [cells of the launch][nfft], slot b for a cell that ends in the launch
    // C == 1, a cell is a row: the caller's planes at row r0, [rows][nfft] floats, either may be NULL
    float *row_sum; float *row_pk;
};
hipError_t launch_sgram_cells(const SgramCellsArgs &a, hipStream_t s);

// k_sgram_fold (C > 1 only): one thread per (row the launch touches, bin).  t = the open row's total if the row began in front of the
// launch and has closed cells there (has_tot_in), else 0.0; t += the row's cells that ended in the launch, in cell order; peak = max.
// A row that ends in the launch is rounded once to float into the caller's planes at row r - r0; the row the launch leaves open goes
// to tot_*_out -- the other buffer, never tot_*_in.
struct SgramFoldArgs {
    const double *cell_sum; const float *cell_pk;
    int32_t nfft, n_rows, has_tot_in;     // n_rows: rows r0 .. r0 + n_rows - 1 hold a segment of the launch
    int64_t R, C, g0, r0, n_closed;       // n_closed: cells g0 .. g0 + n_closed - 1 ended in the launch
    int64_t seg_end;                      // one past the launch's last segment
    const double *tot_sum_in; const float *tot_pk_in;
    double *tot_sum_out; float *tot_pk_out;
    float *row_sum; float *row_pk;
};
hipError_t launch_sgram_fold(const SgramFoldArgs &a, hipStream_t s);

} // namespace iqgpu
