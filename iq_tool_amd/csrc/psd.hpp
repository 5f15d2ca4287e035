// psd.hpp -- power spectrum of a stream on the device (include/iqgpu.h "power spectrum"): the argument blocks and launchers of
// k_psd_pages / k_psd_fold / k_psd_carry (psd.hip; host side psd.cpp), and the host's stream core PsdStream, which the
// row accumulator (sgram.hpp) holds too.
#pragma once
#include "accum_core.hpp"
#include "chain.hpp"

namespace iqgpu {

// Segments of one page: consecutive segments, by stream index, whose powers one workgroup sums in registers.  A closed page costs
// 12 bytes a bin in the page buffer, written once and read once by the fold, against G * hop frames of input read: at cs16 and
// hop = nfft / 2 that is 12 / (2 G) of the input bytes each way -- 19 % at G = 32, and it halves with every doubling.  The fold is a
// serial chain per bin over the pages of a launch, so its length falls with G as well.  Against that, a push of n frames yields
// n / (G hop) workgroups: at G = 32 a 2^22-frame push at nfft = 1024 still gives one workgroup to each of the 256 CUs, at 64 it does not.
constexpr int kPsdPageSegments = 32;
// bins of the page buffer: 4096 closed pages a launch at nfft = 1024, 1024 at nfft = 4096 (48 MiB of doubles and floats)
constexpr int64_t kPsdPageBufBins = (int64_t)1 << 22;

// k_psd_pages<log2 nfft, format>: workgroup b sums page `page0 + b` of the stream's segment grid.  The logical stream of a launch is
// carry[0 .. split) followed by raw[0 ..): segment seg0 + j starts at logical frame first + j * hop.
struct PsdPagesArgs {
    const void *carry, *raw;      // frames in the accumulator's format; raw needs frame alignment only
    int64_t split;                // frames of the carry in front of raw[0]
    int64_t first;                // logical frame segment seg0 starts at
    int32_t fmt, log2n, hop;
    float gain;
    int64_t seg0, n_seg;          // stream index of the launch's first segment, segments of the launch (>= 1)
    const float *window;          // [nfft]
    const cf2 *twiddle;           // [nfft], exp(-2 pi i k / nfft)
    // the open page, [nfft] each, in TWO buffers: a page that begins in front of seg0 starts from open_*_in, one that does not end with
    // the launch goes to open_*_out -- never the same memory, so no workgroup of a launch reads what another one writes
    const double *open_sum_in; const float *open_pk_in;
    double *open_sum_out; float *open_pk_out;
    double *page_sum; float *page_pk;     // [closed pages of the launch][nfft], in page order
};
hipError_t launch_psd_pages(const PsdPagesArgs &a, hipStream_t s);

// k_psd_fold: total[k] += page[p][k] for p = 0 .. n_pages - 1 in that order, peak[k] = max
struct PsdFoldArgs {
    const double *page_sum; const float *page_pk; int32_t n_pages, nfft;
    double *total_sum; float *total_pk;
};
hipError_t launch_psd_fold(const PsdFoldArgs &a, hipStream_t s);

// k_psd_carry: dst[0 .. bytes) = bytes first .. first + bytes - 1 of the logical stream carry[0 .. split_bytes) ++ raw
struct PsdCarryArgs { const unsigned char *carry, *raw; int64_t split_bytes, first; int32_t bytes; unsigned char *dst; };
hipError_t launch_psd_carry(const PsdCarryArgs &a, hipStream_t s);

// host side, no device (psd.cpp), shared with the row accumulator (sgram.cpp): the option checks (`who` names the caller in the error
// text) and the whole segments of `frames` frames
int psd_check_opts(const iqgpu_psd_opts *o, const char *who);
uint64_t psd_segments_of(const iqgpu_psd_opts &o, uint64_t frames);

// One push: n frames of device memory at raw on stream s; the stream's frames and whole segments with them, m of the segments new
struct PsdPush { const void *raw; size_t n; hipStream_t s; uint64_t frames, segs; int64_t m; };

// The stream core both handles hold (psd.cpp): the handle core (accum_core.hpp: identity, position in frames, streams, guard / settle
// / close) and what belongs to the segment grid -- the carry of trailing frames in two buffers (the launches of a push read
// carry[cur], its last launch writes carry[cur ^ 1]) and the device tables.  What a handle accumulates, and its open state, are the handle's.
struct IQGPU_LOCAL PsdStream : AccumCore {
    int log2n = 0;
    iqgpu_psd_opts q{};
    double window_sum = 0.0, window_sum_sq = 0.0;
    uint64_t segments = 0;                // whole segments of the frames pushed since the last reset (all accumulated)
    size_t carry_n = 0;                   // frames in carry[cur]: stream frames segments * hop .. frames - 1
    int cur = 0;
    DevBuf tables, carry[2], stage;       // tables: [nfft] window, then [nfft] twiddles as (cos, sin) pairs
    const float *window() const { return (const float *)tables.p; }
    const cf2 *twiddle() const { return (const cf2 *)((const float *)tables.p + q.nfft); }

    // The checks of a create in their order -- options, then AccumCore::open's (st NULL: no handle could be allocated) -- then buffers
    // and the tables' upload, queued on `own` from `tab`: the caller queues the zero fill of its open state behind it and synchronises
    // once, with `tab` alive until then.  `who` leads the error texts.
    static int open(PsdStream *st, int device, int format, const iqgpu_psd_opts *o, const char *who, std::vector<float> &tab);
    ~PsdStream() = default;               // frees the stream and the buffers; the waits in front of that are close()
    void rewind() { AccumCore::rewind(); segments = 0; carry_n = 0; cur = 0; }           // ... as created
    int enter(const void *d_raw, size_t n, hipStream_t s, PsdPush *u);   // the previous push's stream waited for if it is another; s remembered
    // what PsdPagesArgs and SgramCellsArgs have in common, for the launch over segments [j, j + cnt) of the push, but for open_*: the handle's
    template <class Args> void fill(const PsdPush &u, int64_t j, int64_t cnt, Args *a) const
    {
        a->carry = carry[cur].p; a->raw = u.raw; a->split = (int64_t)carry_n; a->first = j * (int64_t)q.hop;
        a->fmt = format; a->log2n = log2n; a->hop = (int32_t)q.hop; a->gain = q.gain;
        a->seg0 = (int64_t)segments + j; a->n_seg = cnt; a->window = window(); a->twiddle = twiddle();
    }
    int finish(const PsdPush &u);         // the trailing frames into the other carry buffer, the position behind the push, poisoned cleared
};

} // namespace iqgpu
