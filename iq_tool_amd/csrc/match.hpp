// match.hpp -- template correlation of a stream on the device (include/iqgpu.h "template correlation"): the argument blocks and
// launchers of k_match_segs / k_match_fold (match.hip; host side match.cpp).  The segment grid at hop = nfft / 2, the
// unpack, the twiddles, the transform and the carry are the power spectrum's (psd.hpp, psd_stream.hpp, fft16.hpp).
#pragma once
#include "psd.hpp"

namespace iqgpu {

constexpr int kMatchMaxTemplates = 8;
// segments of one launch: the slab holds one record per (segment, template) of it, 4 MiB at eight templates; match.cpp cuts longer
// pushes into several launches
constexpr int64_t kMatchSlabSegments = (int64_t)1 << 15;

// what a workgroup leaves of one segment and one template, and what the fold carries of an open row: the double sum of the V powers,
// the largest of them and the lowest position that attains it (a segment's: 0 .. V - 1; an open row's: from the row's first position)
struct MatchRec { double sum; float peak; uint32_t at; };
static_assert(sizeof(MatchRec) == 16, "one 16-byte store a record");

// k_match_segs<log2 nfft, format>: workgroup b serves segment seg0 + b.  The logical stream of a launch is carry[0 .. split) followed
// by raw[0 ..), as for k_psd_pages: segment seg0 + j starts at logical frame first + j * hop.  The fields up to `twiddle` are the ones
// PsdStream::fill sets (window is not read: no window is applied)
struct MatchSegsArgs {
    const void *carry, *raw;
    int64_t split, first;
    int32_t fmt, log2n, hop;
    float gain;
    int64_t seg0, n_seg;
    const float *window;
    const cf2 *twiddle;
    const cf2 *g;                 // [n_templates][nfft]: conj(FFT(h_t zero-padded)) / nfft
    int32_t n_templates;
    MatchRec *slab;               // [n_seg][n_templates]
};
hipError_t launch_match_segs(const MatchSegsArgs &a, hipStream_t s);

// k_match_fold: one thread per (row the launch touches, template).  It starts from open_in[t] if the row began in front of the launch
// (has_open_in; row r0 only), else from {0.0, 0.0f, 0}; walks the row's records of the launch in segment order -- sum += in double,
// a peak replaces the held one only where it is GREATER, so the lowest position wins a tie -- and writes a row that ends in the launch
// rounded once into the caller's planes at row r - r0, [rows][n_templates] each, any may be NULL; the row the launch leaves open goes
// to open_out -- the other buffer, never open_in.
struct MatchFoldArgs {
    const MatchRec *slab;
    int32_t n_templates, n_rows, has_open_in, V;      // n_rows: rows r0 .. r0 + n_rows - 1 hold a segment of the launch
    int64_t R, r0, seg0, seg_end;                     // segments a row; the launch's segments [seg0, seg_end)
    const MatchRec *open_in; MatchRec *open_out;      // [n_templates]
    float *row_peak; uint32_t *row_at; float *row_sum;
};
hipError_t launch_match_fold(const MatchFoldArgs &a, hipStream_t s);

} // namespace iqgpu
