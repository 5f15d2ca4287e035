/*
 * iqgpu_run -- minimal raw-file harness around libiqgpu: reader -> GPU chain -> writer.
 *
 * It plays the role that iq_tool's raw-file reader (src/input_rawfile.c:168-252), stage threads and
 * raw-file writer (src/output_raw_file.c:146-184) play around the sample path, with the reference's
 * option names where they exist, so that BASELINE.json's configs can be run from a shell:
 *
 *   iqgpu_run -i in.cs16 --raw-file-input-rate 2.4e6 --raw-file-input-sample-format cs16 \
 *             -o out.cs16 --output-rate 744187.5 --output-sample-format cs16 --freq-shift 200e3
 *
 * Copies are double-buffered: pinned host buffers, hipMemcpyAsync on separate streams, events
 * between them (all through the C ABI, no HIP header here), so H2D of chunk i+1 and D2H of chunk
 * i-1 overlap the kernels of chunk i.  Nothing is flushed at end of stream (as in the reference).
 *
 * --shards N splits the input file into N equal frame ranges, one worker thread (and one GPU,
 * round-robin over --devices) per range, each with fresh state, and stitches the outputs in shard
 * order with pwrite at offsets known up front (the output count of a shard is a closed form):
 * exactly what N iq_tool runs + cat would produce (BASELINE configs[4]).  No collective.  Every shard thread binds itself to
 * the NUMA node of its GPU before its first GPU call and before it allocates its pinned buffers (iqgpu_bind_thread_to_device),
 * and fails when the frames its chain produced differ from the count its output offset was planned with.
 *
 * --shards N --seamless cuts ONE stream instead: shard starts are s * (frames / N) rounded down to a multiple of 4096 frames (every
 * 2^S decimation group the ratio range allows and 16 bytes of every input format divide it, so each shard starts on a group and on
 * an aligned word), every shard thread reads the iqgpu_design_preroll_frames frames in front of its start, puts its chain there with
 * iqgpu_chain_seek and runs its usual chunk loop; output offsets come from iqgpu_design_out_frames_range.  The stitched file is the
 * file --shards 1 writes (iqgpu.h: byte for byte without --dc-block, to 1e-6 of full scale with it; refused with an AGC option).
 *
 * --shards N --seamless-agc is --seamless for chains with the digital output AGC (every shipped preset), in the two passes of
 * iqgpu.h's v8 block.  Shard starts are s * (frames / N) rounded down to a multiple of lcm(4096, AGC chunk, --chunk-frames): the
 * digital AGC works on the chunks of each call, so every call of every shard has to lie on the single stream's call and chunk grid.
 * Pass 1: shards 0 .. N-2 put their chain at their start (iqgpu_chain_seek_agc, no entry state) and measure their range batch by
 * batch (iqgpu_chain_measure; the last shard's range is in front of nobody).  One walk over the tables in order
 * (iqgpu_chain_agc_advance) then gives the AGC state at the start of shards 1 .. N-1.  Pass 2: every shard seeks again, now with
 * its entry state, and runs the usual chunk loop.  Preroll and output placement come from the description with the AGC off.
 *
 * --shards N --seamless-dc is the EXACT --seamless for chains with the DC blocker (--dc-block, no AGC option), in the three passes of
 * iqgpu.h's DC block.  Shard starts are s * (frames / N) rounded down to a multiple of lcm(4096, --chunk-frames): every call of every
 * shard is a call of the single stream.  Pass 1: shards 0 .. N-2 measure the map of every call of their range, a batch of whole calls
 * per library call (iqgpu_chain_dc_measure_range: one read of the input, no front kernel, no output).  One walk over all rows (iqgpu_chain_dc_advance) then
 * gives the blocker's state in front of every call.  Pass 2: every shard puts its chain at its start with iqgpu_chain_seek_dc -- the
 * preroll is the filters' memory rounded up to whole chunks, with NO warm-up of the blocker, entered with the walked state -- and runs
 * the usual chunk loop.  The stitched file is the file --shards 1 writes, byte for byte.
 *
 * --shards N --seamless-rms is --seamless for chains with the dx / local output AGC (--output-agc, --agc-profile dx|local), whose
 * loop state the library rebuilds from a bounded window (iqgpu.h): cuts at multiples of 4096 frames, every shard thread reads the
 * iqgpu_design_preroll_frames_rms frames in front of its start, seeks with iqgpu_chain_seek_rms, processes its range and records its
 * AGC state right after the seek and behind the range, and a checkpoint behind the range.  After the join the seams are checked in
 * order: the state a shard started from against the state the shard in front ended in (gain, peak_memory, samples_seen, bit for
 * bit).  A range behind a seam that does not certify -- a cut in or behind digital silence -- is processed again from the checkpoint
 * of the range in front, and the next seam is checked against its new end state.  The file is the one --shards 1 writes; the report
 * says how many seams certified and how many ranges were redone.
 * --shards N --seamless-dc-agc is the exact --seamless for chains with the DC blocker AND the digital output AGC (--dc-block
 * --agc-profile digital), in the five steps of iqgpu.h's block on such chains.  Shard starts lie on lcm(4096, --chunk-frames), and
 * --chunk-frames is a multiple of the AGC chunk.  Step 1: shards 0 .. N-2 measure the DC maps of every call of their range
 * (iqgpu_chain_dcagc_dc_measure_range: one row per piece, two for the call the stream cuts at the AGC's lock).  Step 2: one walk over all
 * rows; the state in front of a call is the one in front of its first row.  Step 3: the same shards put their chain at their start
 * with the walked DC state and no AGC entry (iqgpu_chain_dcagc_seek) and measure the AGC rows of their range in shadow calls
 * (iqgpu_chain_dcagc_measure, synchronous).  Step 4: the AGC walk.  Step 5: every shard seeks with both states and runs the usual
 * chunk loop.  The stitched file is the file --shards 1 writes, byte for byte.
 *
 * --shards N --seamless-dc-rms is the exact --seamless for chains with the DC blocker AND the dx / local output AGC (--dc-block
 * --agc-profile dx|local): --seamless-dc's measure pass and walk (iqgpu_chain_dcrms_dc_measure_range, one row per call; one
 * iqgpu_chain_dcrms_dc_advance), then --seamless-rms's pass: every shard seeks with iqgpu_chain_dcrms_seek -- a preroll of
 * iqgpu_design_preroll_frames_dcrms frames rounded up to whole calls, entered with the walked state -- processes its range on the call
 * grid, and the seams are certified in order, a range behind a seam that does not certify redone from the checkpoint in front.
 *
 * --synthetic FRAMES [--synthetic-hash SEED]: no input file.  Without a seed one constant pinned buffer is sent again and again
 * (the PCIe-inclusive rate of the path, nothing else); with one, shard s is the stream frame n -> splitmix64((SEED + s) * K + n)
 * of its own (iq_tool_amd/synth.py hash_stream restates it): configs[4] at its real size -- 8 x 2.5 G frames -- without 80 GB of
 * files, every range of every shard reproducible by the checker.  With --seamless the job is ONE stream of seed SEED indexed by the
 * global frame number.
 *
 * --psd PREFIX (plain single-stream runs only: no --shards, no --seamless* mode, no --iq-calibrate): one iqgpu_psd accumulator on the
 * input bytes and one on the output bytes, at the library's defaults (Hann, 1024 bins, hop 512), fed on the chain's stream behind every
 * call; behind the run PREFIX.in.f64 and PREFIX.out.f64 hold sum_power (1024 little-endian doubles, bin 0 = DC) and PREFIX.json both
 * info records and the two rates.
 *
 * --sgram PREFIX [--sgram-row-segments R] (the same runs as --psd, and it may stand beside --psd): one iqgpu_sgram accumulator on the
 * input bytes and one on the output bytes, at the library's defaults with R segments a row (32), fed on the chain's stream behind every
 * call.  PREFIX.in.f32 and PREFIX.out.f32 receive row_sum of every row as it finishes (1024 little-endian floats a row, bin 0 = DC);
 * the partial last row is not written.  PREFIX.json holds both info records -- rows, segments, open_segments among them -- and the rates.
 *
 * --envelope PREFIX [--envelope-block B] (the same runs as --psd, and it may stand beside --psd / --sgram / --stats): one iqgpu_env accumulator
 * on the input bytes and one on the output bytes, B frames a row (the library's default, 4096), fed on the chain's stream behind every
 * call.  PREFIX.in.f32 and PREFIX.out.f32 receive row_sum of every row as it finishes (one little-endian float a row); PREFIX.json holds
 * B, both info records with both open rows, and the bursts of the INPUT (iqgpu_env_bursts) at on = floor(0.1) + 10 dB, off = floor(0.1)
 * + 7 dB, min_rows 2, hang_rows 2, pad_rows 1, floor(0.1) being iqgpu_env_floor of the input's rows.
 *
 * --lag PREFIX [--lag-list d1,d2,..] [--lag-block B] (the same runs as --envelope, and it may stand beside --psd / --sgram / --stats / --envelope):
 * one iqgpu_lag accumulator on the input bytes and one on the output bytes, B frames a row (4096) and up to four lags (1), fed on the
 * chain's stream behind every call.  PREFIX.in.lag.f32 / PREFIX.out.lag.f32 receive row_lag of every row as it finishes (2 n_lags
 * little-endian floats a row), PREFIX.in.sum.f32 / PREFIX.out.sum.f32 its row_sum; PREFIX.json holds the options, both info records and
 * iqgpu_lag_estimate_rows over the whole input and the whole output per lag, at the run's input and output rates.
 * --match PREFIX --match-template FILE.cf32 [--match-block B] [--match-shifts hz1,hz2,..] (the same runs as --lag, and it may stand beside the others):
 * one iqgpu_match accumulator on the input bytes and one on the output bytes, fed on the chain's stream behind every call.  FILE.cf32 holds
 * the template, 2 .. 2049 cf32 frames; with --match-shifts (one to eight offsets in Hz) each side correlates with the
 * iqgpu_match_shift_bank of the template at that side's sample rate.  B start positions a row (4096), nfft the smallest that holds the
 * template.  PREFIX.{in,out}.peak.f32 / .at.u32 / .sum.f32 receive the rows as they finish (n_templates values a row each); PREFIX.json
 * holds the options, both info records and iqgpu_match_peaks over all rows of each side at ratio 100.
 *
 * --stats PREFIX (plain runs and --shards N with independent shards; no --seamless* mode, no --iq-calibrate): one iqgpu_stats accumulator
 * on the input bytes and one on the output bytes of every shard, fed on the chain's stream behind every call.  The shards' results are
 * concatenated in shard order (iqgpu_stats_merge: every count, extremum and the peak are exactly the one stream's) and PREFIX.json
 * holds, for "in" and "out", the complete iqgpu_stats_result -- every field, the histograms as arrays, doubles as %.17g -- and under
 * "derived" the iqgpu_stats_derived record.
 */
#define _GNU_SOURCE
#define _FILE_OFFSET_BITS 64
#include <errno.h>
#include <fcntl.h>
#include <pthread.h>
#include <sched.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include "iqgpu.h"

#define NBUF 2

/* what the shards of a job are to each other: streams of their own, or ranges of ONE stream under one of the six recipes above */
typedef enum { M_INDEPENDENT, M_SEAMLESS, M_AGC, M_DC, M_DC_AGC, M_RMS, M_DC_RMS, M_COUNT } Mode;

/* What a mode asks of the command line and of the chain, each named after what it refuses: no --shards; a chain with / without the
 * output AGC; without the DC blocker; an AGC profile other than digital; the digital profile; an input that cannot be read twice;
 * --chunk-frames 0 / not a multiple of the AGC chunk.  validate() goes through a row's list in the row's order */
enum { C_END, C_SHARDS, C_HAS_AGC, C_NO_AGC, C_NO_DC, C_PROFILE, C_DIGITAL, C_TWICE, C_CHUNK0, C_CHUNK_AGC };
/* the two stages the exact recipes carry a state for.  As bits: dc_block_enable / agc_enable cleared for a design query; rows predicted */
enum { F_DC = 1, F_AGC = 2 };

typedef struct {
    const char *flag, *json_key;
    unsigned char checks[8];          /* C_*, in the order of the refusals */
    const char *sans_agc, *sans_dc;   /* the mode a refusal names for the same chain without its AGC / its blocker */
    int grid_agc, grid_chunk;         /* cuts at multiples of lcm(4096 [, the AGC chunk] [, --chunk-frames]) */
    int preroll_off, place_off;       /* F_*: cleared in the description for the preroll query / for iqgpu_design_out_frames_range */
    int (*preroll_fn)(const iqgpu_chain_desc *, uint64_t *);
    int whole_calls;                  /* the preroll is rounded up to whole calls of --chunk-frames */
    const char *grid_words;           /* an empty shard is refused, with the grid in these words; NULL: it is planned */
    int barriers;                     /* rendezvous of the shard threads: two per walk */
    int dry_rows;                     /* F_*: the row counts --dry-placement predicts */
    int certify;                      /* the seam certificate of the dx / local AGC: states and checkpoints kept, the seams checked after the join */
} ModeRow;

static const ModeRow MODES[M_COUNT] = {
    [M_INDEPENDENT] = {0},
    [M_SEAMLESS] = {.flag = "--seamless", .json_key = "seamless", .preroll_fn = iqgpu_design_preroll_frames},
    [M_AGC] = {.flag = "--seamless-agc", .json_key = "seamless_agc", .checks = {C_NO_AGC, C_TWICE, C_PROFILE}, .sans_agc = "--seamless",
               .grid_agc = 1, .grid_chunk = 1, .preroll_off = F_AGC, .place_off = F_AGC, .preroll_fn = iqgpu_design_preroll_frames,
               .grid_words = " (lcm of 4096, the AGC chunk and --chunk-frames)", .barriers = 2, .dry_rows = F_AGC},
    [M_DC] = {.flag = "--seamless-dc", .json_key = "seamless_dc", .checks = {C_SHARDS, C_HAS_AGC, C_NO_DC, C_TWICE, C_CHUNK0}, .sans_dc = "--seamless",
              .grid_chunk = 1, .preroll_off = F_DC, .place_off = 0, .preroll_fn = iqgpu_design_preroll_frames, .whole_calls = 1,
              .grid_words = " (lcm of 4096 and --chunk-frames)", .barriers = 2, .dry_rows = F_DC},
    [M_DC_AGC] = {.flag = "--seamless-dc-agc", .json_key = "seamless_dc_agc", .checks = {C_SHARDS, C_NO_DC, C_NO_AGC, C_PROFILE, C_TWICE, C_CHUNK_AGC},
                  .sans_agc = "--seamless-dc", .sans_dc = "--seamless-agc", .grid_chunk = 1, .preroll_off = F_DC | F_AGC, .place_off = F_DC | F_AGC,
                  .preroll_fn = iqgpu_design_preroll_frames, .whole_calls = 1, .grid_words = " (lcm of 4096 and --chunk-frames)", .barriers = 4,
                  .dry_rows = F_DC | F_AGC},
    [M_RMS] = {.flag = "--seamless-rms", .json_key = "seamless_rms", .checks = {C_SHARDS, C_TWICE, C_CHUNK0}, .place_off = F_AGC,
               .preroll_fn = iqgpu_design_preroll_frames_rms, .grid_words = "", .certify = 1},
    [M_DC_RMS] = {.flag = "--seamless-dc-rms", .json_key = "seamless_dc_rms", .checks = {C_SHARDS, C_NO_DC, C_NO_AGC, C_DIGITAL, C_TWICE, C_CHUNK0},
                  .sans_agc = "--seamless-dc", .sans_dc = "--seamless-rms", .grid_chunk = 1, .place_off = F_AGC,
                  .preroll_fn = iqgpu_design_preroll_frames_dcrms, .whole_calls = 1, .grid_words = " (lcm of 4096 and --chunk-frames)", .barriers = 2,
                  .dry_rows = F_DC, .certify = 1},
};

typedef struct {
    const char *in_path, *out_path;
    iqgpu_chain_desc desc;
    size_t chunk_frames;
    int shards, devices, device0;
    long long synthetic_frames;       /* > 0: no input file, reuse one pinned buffer (PCIe-inclusive rate) */
    int have_hash; unsigned long long hash_seed;   /* ... or generate shard s as the counter-hash stream of seed hash_seed + s */
    int no_bind;                      /* --no-numa-bind */
    Mode mode, clash;                 /* the --seamless* option given (none: M_INDEPENDENT); a second, different one (validate() refuses it) */
    int have_shards;                  /* --shards was given */
    int dry;                          /* --dry-placement: plan, bind, size the buffers, report -- no GPU call */
    int quiet;
    int iq_calibrate, have_iq_factors;   /* --iq-calibrate: the I/Q factors come from the head of the input (calibrate_head); --iq-factors was given */
    const char *psd_prefix;           /* --psd PREFIX: the power spectra of the input and of the output, written behind the run (write_psd) */
    const char *sgram_prefix;         /* --sgram PREFIX: the rows of the input and of the output, appended as they finish (write_sgram_rows) */
    unsigned sgram_row_segments;      /* --sgram-row-segments R (0: the library's default) */
    const char *env_prefix;           /* --envelope PREFIX: row_sum of the input and of the output, appended as the rows finish; the bursts of the input (write_env) */
    unsigned env_block;               /* --envelope-block B (0: the library's default) */
    const char *lag_prefix;           /* --lag PREFIX: row_lag and row_sum of the input and of the output, appended as the rows finish; the estimates (write_lag) */
    const char *lag_list;             /* --lag-list d1,d2,.. (NULL: the library's default); lag_opts_of reads both */
    unsigned lag_block;               /* --lag-block B (0: the library's default) */
    const char *match_prefix;         /* --match PREFIX: row_peak, row_at and row_sum of the input and of the output, appended as the rows finish; the detections (write_match) */
    const char *match_template;       /* --match-template FILE.cf32 */
    const char *match_shifts;         /* --match-shifts hz1,hz2,.. (NULL: the template alone); match_shifts_of reads it */
    unsigned match_block;             /* --match-block B (0: the library's default) */
    const char *stats_prefix;         /* --stats PREFIX: the statistics of the input and of the output bytes, merged over the shards (write_stats) */
} Options;

typedef struct {
    const Options *opt;
    int shard;
    long long first_frame, frames;    /* input range */
    long long out_offset_bytes;       /* where this shard's output starts in the output file */
    long long frames_out;             /* result */
    long long planned_out;            /* iqgpu_design_out_frames(frames): what out_offset_bytes of the NEXT shard was computed from */
    long long preroll_frames;         /* every seamless mode: input frames in front of first_frame the chain is warmed up on */
    int device, numa_node;            /* where it ran; -1 = the host does not say / not bound */
    char bus_id[64]; int cpus_allowed; long long pinned_bytes, hbm_bytes;   /* --dry-placement's report */
    double seconds, stream_seconds;   /* whole shard incl. set-up / copy-process-copy loop only */
    /* --seamless-agc */
    iqgpu_agc_chunk *rows; long long agc_rows;   /* pass 1: this shard's table (planned count with --dry-placement) */
    iqgpu_agc_state entry; int have_entry;       /* the AGC state at first_frame, from the walk */
    /* --seamless-dc */
    iqgpu_dc_row *dc_rows; long long n_dc_rows;  /* pass 1: the rows of the calls of this shard's range (planned count with --dry-placement) */
    iqgpu_dc_state dc_entry;                     /* the blocker's state in front of this shard's preroll, from the walk */
    unsigned char *dc_call_rows; long long n_dc_calls;   /* how many rows every call of the range gave (--seamless-dc-agc: 1 or 2) */
    double measure_seconds;
    /* --seamless-rms, --seamless-dc-rms: the AGC state right after the seek and behind the range, the checkpoint behind the range; redo_blob: this
     * range again from the checkpoint of the range in front (its seam did not certify) */
    iqgpu_agc_state rms_seek_state, rms_end_state;
    void *blob; size_t blob_bytes;
    const void *redo_blob; size_t redo_bytes;
    int certified, redone;
    int barriers;                     /* how many of its mode's barriers this thread has been through */
    iqgpu_stats_result stats[2];      /* --stats: this shard's input and output bytes (read_stats) */
    int rc;
    char err[256];
} Shard;

/* what one shard thread holds while it runs: ctx_open() fills it, ctx_close() releases whatever of it is there */
typedef struct {
    Shard *sh;
    const Options *o;
    iqgpu_chain_desc d;
    size_t ibps, obps, chunk, out_cap;
    iqgpu_chain *chain;
    void *s_in, *s_k, *s_out;
    void *h_in[NBUF], *h_out[NBUF], *d_in[NBUF], *d_out[NBUF];
    void *e_in[NBUF], *e_k[NBUF], *e_out[NBUF];
    int in_fd, out_fd;
    void *pre; size_t np;             /* the preroll in front of first_frame (load_preroll) */
    size_t agc_cap;                   /* rows sh->rows has room for (alloc_agc_table) */
    iqgpu_psd *psd_in, *psd_out;      /* --psd: one accumulator on the input bytes, one on the output bytes (the library's defaults) */
    iqgpu_psd_opts psd_opts;          /* ... the options both were created with */
    iqgpu_stats *st[2];               /* --stats: side 0 = input bytes, 1 = output bytes */
    /* --sgram, side 0 = input, 1 = output: the accumulator, its file, per pipeline buffer the device and pinned host planes of the rows a
     * call finishes (sg_cap rows each) and how many the call in flight there did finish */
    iqgpu_sgram *sg[2]; iqgpu_sgram_opts sg_opts; FILE *sg_f[2];
    void *sg_d[2][NBUF], *sg_h[2][NBUF]; size_t sg_cap[2], sg_rows[2][NBUF];
    /* --envelope, the same shape: one float a row; ev_all keeps the input's rows for the burst finder behind the run */
    iqgpu_env *ev[2]; iqgpu_env_opts ev_opts; FILE *ev_f[2];
    void *ev_d[2][NBUF], *ev_h[2][NBUF]; size_t ev_cap[2], ev_rows[2][NBUF];
    float *ev_all; size_t ev_all_n, ev_all_cap;
    /* --lag, the same shape: plane 0 = row_lag (2 n_lags floats a row), plane 1 = row_sum; lg_all keeps both for the estimates behind the run */
    iqgpu_lag *lg[2]; iqgpu_lag_opts lg_opts; FILE *lg_f[2][2];
    void *lg_d[2][2][NBUF], *lg_h[2][2][NBUF]; size_t lg_cap[2], lg_rows[2][NBUF];
    float *lg_all[2][2]; size_t lg_all_n[2], lg_all_cap[2];
    /* --match, the same shape: planes 0 .. 2 = row_peak, row_at, row_sum (n_templates 4-byte values a row each); mt_all keeps them for the
     * detections behind the run */
    iqgpu_match *mt[2]; iqgpu_match_opts mt_opts; FILE *mt_f[2][3];
    void *mt_d[2][3][NBUF], *mt_h[2][3][NBUF]; size_t mt_cap[2], mt_rows[2][NBUF];
    uint32_t *mt_all[2][3]; size_t mt_all_n[2], mt_all_cap[2];
    double mt_hz[8]; uint32_t mt_nhz;
} Ctx;

/* the modes with passes: all shard threads meet behind a measure pass and again behind the walk, which shard 0's thread does in between */
static pthread_barrier_t g_pass;
static Shard *g_shards;
static volatile int g_walk_ok;

static double now_s(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
static size_t agc_chunk_of(const iqgpu_chain_desc *d) { return d->agc_chunk_frames ? d->agc_chunk_frames : 16384; }
static long long lcm(long long a, long long b) { long long x = a, y = b; while (y) { const long long t = x % y; x = y; y = t; } return a / x * b; }

/* frame n of the stream with this seed: splitmix64 of a counter (any range of it can be regenerated, iq_tool_amd/synth.py) */
static inline uint64_t mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
/* cs16: I, Q = the two low 16-bit words as signed values, arithmetic >> 2 (quarter scale: nothing on the path clips); every other
 * integer format: the low bytes of the hash as they are (full-scale noise) */
static void hash_fill(void *dst, int fmt, size_t bps, uint64_t seed, long long first, size_t n)
{
    const uint64_t base = seed * 0xD1342543DE82EF95ull;
    if (fmt == IQGPU_FMT_CS16) {
        int16_t *d = (int16_t *)dst;
        for (size_t i = 0; i < n; i++) {
            const uint64_t x = mix64(base + (uint64_t)(first + (long long)i));
            d[2 * i] = (int16_t)((int16_t)(x & 0xffffu) >> 2);
            d[2 * i + 1] = (int16_t)((int16_t)((x >> 16) & 0xffffu) >> 2);
        }
    } else {
        unsigned char *d = (unsigned char *)dst;
        for (size_t i = 0; i < n; i++) {
            const uint64_t x = mix64(base + (uint64_t)(first + (long long)i));
            memcpy(d + i * bps, &x, bps);              /* (little-endian hosts only, like the raw formats themselves) */
        }
    }
}

static int fmt_from_name(const char *s)
{
    static const struct { const char *n; int v; } t[] = {
        {"cu8", IQGPU_FMT_CU8}, {"cs8", IQGPU_FMT_CS8}, {"cu16", IQGPU_FMT_CU16}, {"cs16", IQGPU_FMT_CS16},
        {"cs24", IQGPU_FMT_CS24}, {"cu32", IQGPU_FMT_CU32}, {"cs32", IQGPU_FMT_CS32}, {"cf32", IQGPU_FMT_CF32},
        {"sc16q11", IQGPU_FMT_SC16Q11}};
    for (size_t i = 0; i < sizeof(t) / sizeof(t[0]); i++) if (!strcmp(s, t[i].n)) return t[i].v;
    return -1;
}

/* n frames of the job's input from stream frame `first` into dst: the file, the counter-hash stream, or the constant filling */
/* the options of --lag: the library's defaults, --lag-block and --lag-list d1,d2,.. (one to four decimal numbers) on top; the library
 * checks their values (iqgpu_lag_rows).  0: fine */
static int lag_opts_of(const Options *o, iqgpu_lag_opts *lo)
{
    uint64_t rows = 0;
    iqgpu_lag_opts_init(lo);
    if (o->lag_block) lo->block_frames = o->lag_block;
    if (o->lag_list) {
        const char *p = o->lag_list;
        uint32_t n = 0;
        if (!*p) return 1;
        while (*p) {
            char *end = NULL;
            const unsigned long long v = strtoull(p, &end, 10);
            if (*p < '0' || *p > '9' || end == p || v > 65536 || n >= 4 || (*end != ',' && *end != 0) || (*end == ',' && !end[1])) return 1;
            lo->lags[n++] = (uint32_t)v;
            p = *end ? end + 1 : end;
        }
        lo->n_lags = n;
    }
    return iqgpu_lag_rows(lo, 0, &rows) != IQGPU_OK;
}

static int read_frames(const Options *o, int in_fd, int fmt, size_t ibps, long long first, size_t n, void *dst, char *err, size_t errcap)
{
    const size_t nb = n * ibps;
    if (in_fd >= 0) {
        size_t got = 0;
        while (got < nb) {
            ssize_t r = pread(in_fd, (char *)dst + got, nb - got, first * (long long)ibps + (long long)got);
            if (r <= 0) { snprintf(err, errcap, "pread: %s", r < 0 ? strerror(errno) : "short file"); return -1; }
            got += (size_t)r;
        }
    } else if (o->have_hash) hash_fill(dst, fmt, ibps, o->hash_seed, first, n);
    else memset(dst, 0x11, nb);
    return 0;
}

/* the steps of a shard thread: 0, or -1 with sh->rc and sh->err set */
#define CK(call) do { int rc_ = (call); if (rc_ != IQGPU_OK) { snprintf(sh->err, sizeof(sh->err), "%s: %s", #call, iqgpu_last_error()); sh->rc = rc_; return -1; } } while (0)
#define FAIL(...) do { snprintf(sh->err, sizeof(sh->err), __VA_ARGS__); sh->rc = -1; return -1; } while (0)
/* main() and its helpers: a message and the exit status */
#define REFUSE(status, ...) do { fprintf(stderr, __VA_ARGS__); return (status); } while (0)

/* n frames of this shard's range from frame `at` of the range.  Independent shards are streams of their own: seed SEED + shard,
 * counted from their own start; the ranges of a seamless job are read at their place in the ONE stream */
static int read_range(Ctx *x, long long at, size_t n, void *dst)
{
    Shard *sh = x->sh;
    if (x->o->mode == M_INDEPENDENT && x->in_fd < 0 && x->o->have_hash) { hash_fill(dst, x->d.in_format, x->ibps, x->o->hash_seed + (uint64_t)sh->shard, at, n); return 0; }
    if (read_frames(x->o, x->in_fd, x->d.in_format, x->ibps, sh->first_frame + at, n, dst, sh->err, sizeof(sh->err))) { sh->rc = -1; return -1; }
    return 0;
}

/* the frames in front of this shard's start, read like any other range of the stream (none: x->pre stays NULL) */
static int load_preroll(Ctx *x)
{
    Shard *sh = x->sh;
    x->np = (size_t)sh->preroll_frames;
    if (!x->np) return 0;
    x->pre = malloc(x->np * x->ibps);
    if (!x->pre) FAIL("out of memory for a preroll of %zu frames", x->np);
    return read_range(x, -sh->preroll_frames, x->np, x->pre);
}

/* every call the ordinary pass will make of this range, in order: its frames into h_in[0], then fn(x, first frame in the range, frames) */
static int for_each_call(Ctx *x, int (*fn)(Ctx *, long long, size_t))
{
    const Shard *sh = x->sh;
    for (long long at = 0; at < sh->frames; at += (long long)x->chunk) {
        size_t n = x->chunk;
        if ((long long)n > sh->frames - at) n = (size_t)(sh->frames - at);
        if (read_range(x, at, n, x->h_in[0]) || fn(x, at, n)) return -1;
    }
    return 0;
}

static size_t range_calls(const Ctx *x) { return (size_t)((x->sh->frames + (long long)x->chunk - 1) / (long long)x->chunk); }

/* room for one AGC row per chunk of every call of the range (pinned: the pipelined pass copies the rows of a batch out asynchronously,
 * behind the kernels of the next one) */
static int alloc_agc_table(Ctx *x)
{
    Shard *sh = x->sh;
    const size_t agc_chunk = agc_chunk_of(&x->d);
    void *table = NULL;
    x->agc_cap = range_calls(x) * ((x->chunk + agc_chunk - 1) / agc_chunk) + 1;
    if (iqgpu_host_malloc_pinned(x->agc_cap * sizeof(iqgpu_agc_chunk), &table) != IQGPU_OK) FAIL("out of memory for a table of %zu rows", x->agc_cap);
    sh->rows = (iqgpu_agc_chunk *)table;
    return 0;
}

/* --seamless-agc, pass 1: the chain at the start of the range with the AGC out of the way, then the range measured in the calls pass 2
 * will make: the batch grid and the two pinned input buffers of the ordinary pass, through the chain's own pipeline: batch i is read
 * while the copy of batch i-1 and the kernels of batch i-2 run; buffer i % 2 is free once batch i-2 is collected */
static int measure_agc_pipelined(Ctx *x)
{
    Shard *sh = x->sh;
    uint64_t tk[NBUF] = {0};
    long long i = 0;
    if (alloc_agc_table(x)) return -1;
    CK(iqgpu_chain_seek_agc(x->chain, (uint64_t)sh->first_frame, x->pre, x->np, NULL));
    for (long long at = 0; at < sh->frames; at += (long long)x->chunk, i++) {
        const int b = (int)(i % NBUF);
        size_t n = x->chunk, got = 0;
        if ((long long)n > sh->frames - at) n = (size_t)(sh->frames - at);
        if (tk[b]) { CK(iqgpu_chain_collect(x->chain, tk[b])); tk[b] = 0; }
        if (read_range(x, at, n, x->h_in[b])) return -1;
        CK(iqgpu_chain_measure_submit(x->chain, x->h_in[b], n, sh->rows + sh->agc_rows, x->agc_cap - (size_t)sh->agc_rows, &got, &tk[b]));
        sh->agc_rows += (long long)got;
    }
    for (int b = 0; b < NBUF; b++) if (tk[b]) CK(iqgpu_chain_collect(x->chain, tk[b]));
    return 0;
}

/* --seamless-dc-agc, step 3: the AGC rows of one call, as a shadow call (synchronous: the pipelined measure makes no shadow calls) */
static int measure_agc_call(Ctx *x, long long at, size_t n)
{
    Shard *sh = x->sh;
    size_t got = 0;
    (void)at;
    CK(iqgpu_chain_dcagc_measure(x->chain, x->h_in[0], n, sh->rows + sh->agc_rows, x->agc_cap - (size_t)sh->agc_rows, &got));
    sh->agc_rows += (long long)got;
    return 0;
}

/* pass 1 of the three DC modes reads its range in batches of whole calls -- one pinned buffer of up to this many bytes, at least one
 * call -- and hands every batch to the range form of its family's DC measure in ONE call.  (The range form wants calls of a multiple
 * of 4096 frames; a grid of other calls -- only the cuts have to be such multiples -- is measured call by call, as before it existed) */
#define DC_BATCH_BYTES ((size_t)256 << 20)

/* the DC maps of every call the ordinary pass will make of this range: one row per call (iqgpu_chain_dc_measure_range,
 * _dcrms_dc_measure_range: no front kernel, no output), with the digital AGC one row per piece (_dcagc_dc_measure_range) */
static int measure_dc(Ctx *x)
{
    Shard *sh = x->sh;
    const Mode mode = x->o->mode;
    int (*const range)(iqgpu_chain *, uint64_t, const void *, size_t, size_t, iqgpu_dc_row *, size_t, size_t *, uint32_t *) =
        mode == M_DC ? iqgpu_chain_dc_measure_range : mode == M_DC_RMS ? iqgpu_chain_dcrms_dc_measure_range : iqgpu_chain_dcagc_dc_measure_range;
    const char *who = mode == M_DC ? "iqgpu_chain_dc_measure_range" : mode == M_DC_RMS ? "iqgpu_chain_dcrms_dc_measure_range" : "iqgpu_chain_dcagc_dc_measure_range";
    const size_t calls = range_calls(x), most = 2 * calls;
    const int by_range = x->chunk % 4096 == 0;
    size_t per = by_range ? DC_BATCH_BYTES / (x->chunk * x->ibps) : 1;
    if (per < 1) per = 1;
    if (per > calls) per = calls;
    sh->dc_rows = (iqgpu_dc_row *)malloc((most + 1) * sizeof(iqgpu_dc_row));
    sh->dc_call_rows = (unsigned char *)malloc(calls + 1);
    uint32_t *first = (uint32_t *)malloc((per + 1) * sizeof(uint32_t));
    void *batch = NULL;
    int rc = -1;
    if (!sh->dc_rows || !sh->dc_call_rows || !first) { snprintf(sh->err, sizeof(sh->err), "out of memory for a table of %zu rows", most); sh->rc = -1; goto out; }
    if (per > 1 && iqgpu_host_malloc_pinned(per * x->chunk * x->ibps, &batch) != IQGPU_OK) {
        snprintf(sh->err, sizeof(sh->err), "out of pinned memory for a batch of %zu calls: %s", per, iqgpu_last_error()); sh->rc = -1; goto out;
    }
    for (long long at = 0; at < sh->frames; at += (long long)(per * x->chunk)) {
        size_t n = per * x->chunk, got = 0;
        if ((long long)n > sh->frames - at) n = (size_t)(sh->frames - at);
        const size_t nc = (n + x->chunk - 1) / x->chunk;
        void *buf = batch ? batch : x->h_in[0];                /* (a batch of one call: the pinned buffer of the ordinary pass) */
        if (read_range(x, at, n, buf)) goto out;
        iqgpu_dc_row *rows = sh->dc_rows + sh->n_dc_rows;
        const uint64_t pos = (uint64_t)(sh->first_frame + at);
        int r;
        if (by_range) r = range(x->chain, pos, buf, n, x->chunk, rows, most - (size_t)sh->n_dc_rows, &got, first);
        else {
            first[0] = 0; got = 1;
            r = mode == M_DC ? iqgpu_chain_dc_measure(x->chain, pos, buf, n, rows) : mode == M_DC_RMS ? iqgpu_chain_dcrms_dc_measure(x->chain, pos, buf, n, rows)
                : iqgpu_chain_dcagc_dc_measure(x->chain, pos, buf, n, rows, 2, &got);
        }
        if (r != IQGPU_OK) { snprintf(sh->err, sizeof(sh->err), "%s: %s", by_range ? who : "the DC measure of one call", iqgpu_last_error()); sh->rc = r; goto out; }
        for (size_t k = 0; k < nc; k++) sh->dc_call_rows[sh->n_dc_calls++] = (unsigned char)((k + 1 < nc ? first[k + 1] : (uint32_t)got) - first[k]);
        sh->n_dc_rows += (long long)got;
    }
    rc = 0;
out:
    if (batch) iqgpu_host_free_pinned(batch);
    free(first);
    return rc;
}

/* the AGC walk: the tables in shard order, the state in front of every shard kept.  (The walks run in shard 0's thread, on its chain,
 * and return whether they went through) */
static int walk_agc(Ctx *x)
{
    Shard *sh = x->sh;
    const int shards = x->o->shards;
    iqgpu_agc_state st;
    if (iqgpu_chain_agc_initial_state(x->chain, &st) != IQGPU_OK) return 0;
    for (int q = 0; q < shards; q++) {
        g_shards[q].entry = st; g_shards[q].have_entry = 1;
        if (q < shards - 1 && iqgpu_chain_agc_advance(x->chain, &st, g_shards[q].rows, (size_t)g_shards[q].agc_rows, NULL) != IQGPU_OK) {
            snprintf(sh->err, sizeof(sh->err), "iqgpu_chain_agc_advance: %s", iqgpu_last_error()); sh->rc = -1; return 0;
        }
    }
    return 1;
}

/* the DC walk: ONE table of all rows in stream order, the state in front of every row; call k of the single stream starts at row
 * first_row[k], and every shard enters its preroll with the state in front of the preroll's first call */
static int walk_dc(Ctx *x)
{
    Shard *sh = x->sh;
    const int shards = x->o->shards;
    const Mode mode = x->o->mode;
    const char *who = mode == M_DC ? "iqgpu_chain_dc_advance" : mode == M_DC_RMS ? "iqgpu_chain_dcrms_dc_advance" : "iqgpu_chain_dcagc_dc_advance";
    int (*const advance)(iqgpu_chain *, iqgpu_dc_state *, const iqgpu_dc_row *, size_t, iqgpu_dc_state *) =
        mode == M_DC ? iqgpu_chain_dc_advance : mode == M_DC_RMS ? iqgpu_chain_dcrms_dc_advance : iqgpu_chain_dcagc_dc_advance;
    int ok = 1;
    long long total = 0, total_calls = 0, k = 0, call = 0;
    for (int q = 0; q < shards; q++) { total += g_shards[q].n_dc_rows; total_calls += g_shards[q].n_dc_calls; }
    iqgpu_dc_row *all = (iqgpu_dc_row *)malloc((size_t)(total ? total : 1) * sizeof(iqgpu_dc_row));
    iqgpu_dc_state *before = (iqgpu_dc_state *)malloc((size_t)(total ? total : 1) * sizeof(iqgpu_dc_state));
    long long *first_row = (long long *)malloc((size_t)(total_calls + 1) * sizeof(long long));
    iqgpu_dc_state st = {0.0, 0.0};
    if (!all || !before || !first_row) { snprintf(sh->err, sizeof(sh->err), "out of memory for the walk over %lld rows", total); sh->rc = -1; ok = 0; }
    for (int q = 0; q < shards && ok; q++) {
        if (g_shards[q].n_dc_rows) memcpy(all + k, g_shards[q].dc_rows, (size_t)g_shards[q].n_dc_rows * sizeof(iqgpu_dc_row));
        long long r = k;
        for (long long j = 0; j < g_shards[q].n_dc_calls; j++) { first_row[call++] = r; r += g_shards[q].dc_call_rows[j]; }
        k += g_shards[q].n_dc_rows;
    }
    if (ok) first_row[call] = k;
    if (ok && advance(x->chain, &st, all, (size_t)total, before) != IQGPU_OK) {
        snprintf(sh->err, sizeof(sh->err), "%s: %s", who, iqgpu_last_error()); sh->rc = -1; ok = 0;
    }
    for (int q = 1; q < shards && ok; q++) {
        const long long c = (g_shards[q].first_frame - g_shards[q].preroll_frames) / (long long)x->chunk;
        /* (c == total_calls: a preroll of no frames in front of the last shard -- a chain without filter memory; the state behind the last row) */
        if (c < 0 || c > total_calls) { snprintf(sh->err, sizeof(sh->err), "the walk holds no state in front of call %lld", c); sh->rc = -1; ok = 0; break; }
        g_shards[q].dc_entry = first_row[c] < total ? before[first_row[c]] : st;
    }
    free(all); free(before); free(first_row);
    return ok;
}

/* All shard threads meet, shard 0's thread walks (if every shard came through the pass in front), all meet again and learn how it went.
 * A thread that failed earlier keeps the appointment without a walk of its own (walk NULL): the others wait there */
static int rendezvous(Ctx *x, int (*walk)(Ctx *), const char *what)
{
    Shard *sh = x->sh;
    pthread_barrier_wait(&g_pass); sh->barriers++;
    if (sh->shard == 0) {
        int ok = walk != NULL;
        for (int q = 0; q < x->o->shards; q++) if (g_shards[q].rc) ok = 0;
        g_walk_ok = ok && walk(x);
    }
    pthread_barrier_wait(&g_pass); sh->barriers++;
    if (!g_walk_ok) { if (!sh->rc) { snprintf(sh->err, sizeof(sh->err), "%s", what ? what : ""); sh->rc = -1; } return -1; }
    return 0;
}

/* chain, streams, events, the NBUF buffer sets, the files */
#define MATCH_RATIO 100.0             /* of --match's detections: the peak against the mean of the row's other positions */

/* --match-shifts hz1,hz2,..: one to eight finite numbers.  0: fine (*n = 0 without the option) */
static int match_shifts_of(const Options *o, double *hz, uint32_t *n)
{
    *n = 0;
    if (!o->match_shifts) return 0;
    const char *p = o->match_shifts;
    for (;;) {
        char *end;
        const double v = strtod(p, &end);
        if (end == p || !(v == v) || v - v != 0.0 || *n >= 8) return -1;
        hz[(*n)++] = v;
        if (*end == '\0') return 0;
        if (*end != ',') return -1;
        p = end + 1;
    }
}

/* the template file of --match: *frames cf32 frames (2 .. 2049) in malloc'd memory, NULL with a reason in `why` */
static float *match_template_of(const char *path, uint32_t *frames, char *why, size_t cap)
{
    FILE *f = fopen(path, "rb");
    if (!f) { snprintf(why, cap, "--match-template %.160s: %s", path, strerror(errno)); return NULL; }
    float *t = (float *)malloc(2050 * 2 * sizeof(float));
    const size_t got = t ? fread(t, 1, 2050 * 2 * sizeof(float), f) : 0;
    fclose(f);
    if (!t || got % (2 * sizeof(float)) != 0 || got < 2 * 2 * sizeof(float) || got > 2049 * 2 * sizeof(float)) {
        snprintf(why, cap, "--match-template %.160s: not 2 .. 2049 cf32 frames", path);
        free(t);
        return NULL;
    }
    *frames = (uint32_t)(got / (2 * sizeof(float)));
    return t;
}

static int ctx_open(Ctx *x)
{
    Shard *sh = x->sh;
    const Options *o = x->o;
    const int dev = x->d.device_ordinal;
    CK(iqgpu_chain_create(&x->d, &x->chain));
    x->chunk = o->chunk_frames;
    x->out_cap = iqgpu_chain_max_out_frames(x->chain, x->chunk) * x->obps;
    CK(iqgpu_stream_create(dev, &x->s_in));
    CK(iqgpu_stream_create(dev, &x->s_k));
    CK(iqgpu_stream_create(dev, &x->s_out));
    CK(iqgpu_chain_set_stream(x->chain, x->s_k));
    for (int b = 0; b < NBUF; b++) {
        CK(iqgpu_host_malloc_pinned(x->chunk * x->ibps, &x->h_in[b]));
        CK(iqgpu_host_malloc_pinned(x->out_cap, &x->h_out[b]));
        CK(iqgpu_device_malloc(dev, x->chunk * x->ibps, &x->d_in[b]));
        CK(iqgpu_device_malloc(dev, x->out_cap, &x->d_out[b]));
        CK(iqgpu_event_create(&x->e_in[b])); CK(iqgpu_event_create(&x->e_k[b])); CK(iqgpu_event_create(&x->e_out[b]));
    }
    if (o->psd_prefix) {
        iqgpu_psd_opts_init(&x->psd_opts);
        CK(iqgpu_psd_create(dev, x->d.in_format, &x->psd_opts, &x->psd_in));
        CK(iqgpu_psd_create(dev, x->d.out_format, &x->psd_opts, &x->psd_out));
    }
    if (o->stats_prefix) {
        CK(iqgpu_stats_create(dev, x->d.in_format, &x->st[0]));
        CK(iqgpu_stats_create(dev, x->d.out_format, &x->st[1]));
    }
    if (o->sgram_prefix) {
        static const char *const side[2] = {"in", "out"};
        const int fmt[2] = {x->d.in_format, x->d.out_format};
        const size_t most[2] = {x->chunk, x->out_cap / x->obps};      /* frames of one call */
        char path[4096];
        iqgpu_sgram_opts_init(&x->sg_opts);
        if (o->sgram_row_segments) x->sg_opts.row_segments = o->sgram_row_segments;
        for (int k = 0; k < 2; k++) {
            CK(iqgpu_sgram_create(dev, fmt[k], &x->sg_opts, &x->sg[k]));
            /* rows one call can finish: the segments that start in it and the one its first frames complete, behind an open row */
            x->sg_cap[k] = (most[k] / x->sg_opts.hop + 1) / x->sg_opts.row_segments + 1;
            for (int b = 0; b < NBUF; b++) {
                CK(iqgpu_device_malloc(dev, x->sg_cap[k] * x->sg_opts.nfft * sizeof(float), &x->sg_d[k][b]));
                CK(iqgpu_host_malloc_pinned(x->sg_cap[k] * x->sg_opts.nfft * sizeof(float), &x->sg_h[k][b]));
            }
            snprintf(path, sizeof(path), "%s.%s.f32", o->sgram_prefix, side[k]);
            x->sg_f[k] = fopen(path, "wb");
            if (!x->sg_f[k]) FAIL("writing %.160s: %s", path, strerror(errno));
        }
    }
    if (o->env_prefix) {
        static const char *const side[2] = {"in", "out"};
        const int fmt[2] = {x->d.in_format, x->d.out_format};
        const size_t most[2] = {x->chunk, x->out_cap / x->obps};      /* frames of one call */
        char path[4096];
        iqgpu_env_opts_init(&x->ev_opts);
        if (o->env_block) x->ev_opts.block_frames = o->env_block;
        for (int k = 0; k < 2; k++) {
            CK(iqgpu_env_create(dev, fmt[k], &x->ev_opts, &x->ev[k]));
            x->ev_cap[k] = most[k] / x->ev_opts.block_frames + 1;     /* rows one call can finish, behind an open row */
            for (int b = 0; b < NBUF; b++) {
                CK(iqgpu_device_malloc(dev, x->ev_cap[k] * sizeof(float), &x->ev_d[k][b]));
                CK(iqgpu_host_malloc_pinned(x->ev_cap[k] * sizeof(float), &x->ev_h[k][b]));
            }
            snprintf(path, sizeof(path), "%s.%s.f32", o->env_prefix, side[k]);
            x->ev_f[k] = fopen(path, "wb");
            if (!x->ev_f[k]) FAIL("writing %.160s: %s", path, strerror(errno));
        }
    }
    if (o->lag_prefix) {
        static const char *const side[2] = {"in", "out"}, *const plane[2] = {"lag", "sum"};
        const int fmt[2] = {x->d.in_format, x->d.out_format};
        const size_t most[2] = {x->chunk, x->out_cap / x->obps};      /* frames of one call */
        char path[4096];
        if (lag_opts_of(o, &x->lg_opts)) FAIL("--lag-list: %s", o->lag_list);
        for (int k = 0; k < 2; k++) {
            const size_t per_row[2] = {2 * (size_t)x->lg_opts.n_lags, 1};
            CK(iqgpu_lag_create(dev, fmt[k], &x->lg_opts, &x->lg[k]));
            x->lg_cap[k] = most[k] / x->lg_opts.block_frames + 1;     /* rows one call can finish, behind an open row */
            for (int q = 0; q < 2; q++) {
                for (int b = 0; b < NBUF; b++) {
                    CK(iqgpu_device_malloc(dev, x->lg_cap[k] * per_row[q] * sizeof(float), &x->lg_d[k][q][b]));
                    CK(iqgpu_host_malloc_pinned(x->lg_cap[k] * per_row[q] * sizeof(float), &x->lg_h[k][q][b]));
                }
                snprintf(path, sizeof(path), "%s.%s.%s.f32", o->lag_prefix, side[k], plane[q]);
                x->lg_f[k][q] = fopen(path, "wb");
                if (!x->lg_f[k][q]) FAIL("writing %.160s: %s", path, strerror(errno));
            }
        }
    }
    if (o->match_prefix) {
        static const char *const side[2] = {"in", "out"}, *const plane[3] = {"peak.f32", "at.u32", "sum.f32"};
        const int fmt[2] = {x->d.in_format, x->d.out_format};
        const double rate[2] = {x->d.input_rate_hz, x->d.target_rate_hz};
        const size_t most[2] = {x->chunk, x->out_cap / x->obps};      /* frames of one call */
        char path[4096], why[512];
        uint32_t L = 0;
        float *tmpl = match_template_of(o->match_template, &L, why, sizeof(why));
        if (!tmpl) FAIL("%.250s", why);
        if (match_shifts_of(o, x->mt_hz, &x->mt_nhz)) { free(tmpl); FAIL("--match-shifts: %s", o->match_shifts); }
        iqgpu_match_opts_init(&x->mt_opts);
        if (o->match_block) x->mt_opts.block_frames = o->match_block;
        x->mt_opts.template_frames = L;
        x->mt_opts.n_templates = x->mt_nhz ? x->mt_nhz : 1;
        float *bank = (float *)malloc((size_t)x->mt_opts.n_templates * L * 2 * sizeof(float));
        if (!bank) { free(tmpl); FAIL("--match: out of memory for the templates"); }
        for (int k = 0; k < 2; k++) {
            int rc = IQGPU_OK;
            if (x->mt_nhz) rc = iqgpu_match_shift_bank(tmpl, L, x->mt_hz, x->mt_nhz, rate[k], bank);
            else memcpy(bank, tmpl, (size_t)L * 2 * sizeof(float));
            if (rc == IQGPU_OK) rc = iqgpu_match_create(dev, fmt[k], &x->mt_opts, bank, &x->mt[k]);
            if (rc != IQGPU_OK) { free(bank); free(tmpl); FAIL("--match: %s", iqgpu_last_error()); }
        }
        free(bank); free(tmpl);
        {
            iqgpu_match_info info;
            CK(iqgpu_match_read_open(x->mt[0], NULL, NULL, NULL, &info));
            x->mt_opts.nfft = info.nfft;                               /* as the handles run it */
        }
        for (int k = 0; k < 2; k++) {
            const size_t row_bytes = (size_t)x->mt_opts.n_templates * 4;
            x->mt_cap[k] = most[k] / x->mt_opts.block_frames + 1;     /* rows one call can finish, behind an open row */
            for (int q = 0; q < 3; q++) {
                for (int b = 0; b < NBUF; b++) {
                    CK(iqgpu_device_malloc(dev, x->mt_cap[k] * row_bytes, &x->mt_d[k][q][b]));
                    CK(iqgpu_host_malloc_pinned(x->mt_cap[k] * row_bytes, &x->mt_h[k][q][b]));
                }
                snprintf(path, sizeof(path), "%s.%s.%s", o->match_prefix, side[k], plane[q]);
                x->mt_f[k][q] = fopen(path, "wb");
                if (!x->mt_f[k][q]) FAIL("writing %.160s: %s", path, strerror(errno));
            }
        }
    }
    if (o->synthetic_frames <= 0) {
        x->in_fd = open(o->in_path, O_RDONLY);
        if (x->in_fd < 0) FAIL("open %s: %s", o->in_path, strerror(errno));
    } else if (!o->have_hash) {
        /* bare --synthetic: filled once, sent again and again */
        for (int b = 0; b < NBUF; b++) memset(x->h_in[b], 0x11 * (b + 1), x->chunk * x->ibps);
    }
    if (o->out_path) {
        x->out_fd = open(o->out_path, O_WRONLY | O_CREAT, 0644);
        if (x->out_fd < 0) FAIL("open %s: %s", o->out_path, strerror(errno));
    }
    return 0;
}

static void ctx_close(Ctx *x)
{
    const int dev = x->d.device_ordinal;
    free(x->pre);
    if (x->chain) iqgpu_chain_synchronize(x->chain);
    iqgpu_psd_destroy(x->psd_in); iqgpu_psd_destroy(x->psd_out);     /* (in front of the stream they last worked on) */
    iqgpu_stats_destroy(x->st[0]); iqgpu_stats_destroy(x->st[1]);
    for (int k = 0; k < 2; k++) {
        iqgpu_sgram_destroy(x->sg[k]);
        if (x->sg_f[k]) fclose(x->sg_f[k]);
        for (int b = 0; b < NBUF; b++) {
            if (x->sg_d[k][b]) iqgpu_device_free(dev, x->sg_d[k][b]);
            if (x->sg_h[k][b]) iqgpu_host_free_pinned(x->sg_h[k][b]);
        }
    }
    for (int k = 0; k < 2; k++) {
        iqgpu_lag_destroy(x->lg[k]);
        for (int q = 0; q < 2; q++) {
            if (x->lg_f[k][q]) fclose(x->lg_f[k][q]);
            free(x->lg_all[k][q]);
            for (int b = 0; b < NBUF; b++) {
                if (x->lg_d[k][q][b]) iqgpu_device_free(dev, x->lg_d[k][q][b]);
                if (x->lg_h[k][q][b]) iqgpu_host_free_pinned(x->lg_h[k][q][b]);
            }
        }
    }
    for (int k = 0; k < 2; k++) {
        iqgpu_env_destroy(x->ev[k]);
        if (x->ev_f[k]) fclose(x->ev_f[k]);
        for (int b = 0; b < NBUF; b++) {
            if (x->ev_d[k][b]) iqgpu_device_free(dev, x->ev_d[k][b]);
            if (x->ev_h[k][b]) iqgpu_host_free_pinned(x->ev_h[k][b]);
        }
    }
    for (int k = 0; k < 2; k++) {
        iqgpu_match_destroy(x->mt[k]);
        for (int q = 0; q < 3; q++) {
            if (x->mt_f[k][q]) fclose(x->mt_f[k][q]);
            free(x->mt_all[k][q]);
            for (int b = 0; b < NBUF; b++) {
                if (x->mt_d[k][q][b]) iqgpu_device_free(dev, x->mt_d[k][q][b]);
                if (x->mt_h[k][q][b]) iqgpu_host_free_pinned(x->mt_h[k][q][b]);
            }
        }
    }
    free(x->ev_all);
    for (int b = 0; b < NBUF; b++) {
        if (x->e_in[b]) iqgpu_event_destroy(x->e_in[b]);
        if (x->e_k[b]) iqgpu_event_destroy(x->e_k[b]);
        if (x->e_out[b]) iqgpu_event_destroy(x->e_out[b]);
        if (x->h_in[b]) iqgpu_host_free_pinned(x->h_in[b]);
        if (x->h_out[b]) iqgpu_host_free_pinned(x->h_out[b]);
        if (x->d_in[b]) iqgpu_device_free(dev, x->d_in[b]);
        if (x->d_out[b]) iqgpu_device_free(dev, x->d_out[b]);
    }
    if (x->s_in) iqgpu_stream_destroy(x->s_in);
    if (x->s_k) { if (x->chain) iqgpu_chain_set_stream(x->chain, NULL); iqgpu_stream_destroy(x->s_k); }
    if (x->s_out) iqgpu_stream_destroy(x->s_out);
    if (x->chain) iqgpu_chain_destroy(x->chain);
    if (x->in_fd >= 0) close(x->in_fd);
    if (x->out_fd >= 0) close(x->out_fd);
}

/* --dry-placement: everything the first multi-GPU run does BEFORE its first GPU call -- the device of this shard,
 * its PCI address and NUMA node from sysfs, the binding, the sizes of the buffers it would pin and allocate -- and nothing after it.
 * The capacity rule without a handle: src/pipeline.c:246-258 on the designed ratio */
static int dry_shard(Ctx *x)
{
    Shard *sh = x->sh;
    const Options *o = x->o;
    int node = -1;
    sh->bus_id[0] = 0;
    (void)iqgpu_device_numa_node(x->d.device_ordinal, &node, sh->bus_id, sizeof(sh->bus_id));
    if (sh->numa_node < 0 && o->no_bind) sh->numa_node = node;
    { cpu_set_t m; CPU_ZERO(&m); sh->cpus_allowed = pthread_getaffinity_np(pthread_self(), sizeof(m), &m) == 0 ? CPU_COUNT(&m) : -1; }
    size_t cap_frames = 0;
    CK(iqgpu_design_out_frames(&x->d, o->chunk_frames, &cap_frames));
    cap_frames += 64;
    sh->pinned_bytes = (long long)NBUF * (long long)(o->chunk_frames * x->ibps + cap_frames * x->obps);
    sh->hbm_bytes = sh->pinned_bytes;
    sh->frames_out = sh->planned_out;
    return 0;
}

/* the chain at first_frame of the job's stream, by the recipe of the job's mode (the head of this file); independent shards start fresh.
 * The last shard of a job with passes measures nothing -- nobody starts behind it -- but meets the others at every rendezvous */
static int enter_stream(Ctx *x)
{
    Shard *sh = x->sh;
    const int measures = sh->shard < x->o->shards - 1;
    const uint64_t first = (uint64_t)sh->first_frame;
    const double t_m = now_s();
    switch (x->o->mode) {
    case M_INDEPENDENT: case M_COUNT: break;
    case M_SEAMLESS:
        if (sh->first_frame > 0) {
            if (load_preroll(x)) return -1;
            CK(iqgpu_chain_seek(x->chain, first, x->pre, x->np));
        }
        break;
    case M_RMS:
        if (sh->redo_blob) {
            /* the seam in front of this range did not certify: the range again, from where the range in front really ended */
            CK(iqgpu_chain_load_state(x->chain, sh->redo_blob, sh->redo_bytes));
        } else if (sh->first_frame > 0) {
            if (load_preroll(x)) return -1;
            CK(iqgpu_chain_seek_rms(x->chain, first, x->pre, x->np));
            CK(iqgpu_chain_get_agc_state(x->chain, &sh->rms_seek_state));
        }
        break;
    case M_AGC:
        if (load_preroll(x) || (measures && measure_agc_pipelined(x))) return -1;
        sh->measure_seconds = now_s() - t_m;
        if (rendezvous(x, walk_agc, "the measure pass or the walk of another shard failed")) return -1;
        /* pass 2: the same position again, now carrying the stream's AGC state there */
        CK(iqgpu_chain_seek_agc(x->chain, first, x->pre, x->np, &sh->entry));
        break;
    case M_DC:
        if (measures && measure_dc(x)) return -1;
        sh->measure_seconds = now_s() - t_m;
        if (rendezvous(x, walk_dc, "the measure pass or the walk of another shard failed")) return -1;
        /* pass 2: the chain at the start of the range, behind a preroll of whole calls entered with the walked state */
        if (sh->first_frame > 0) {
            if (load_preroll(x)) return -1;
            CK(iqgpu_chain_seek_dc(x->chain, first, x->pre, x->np, x->chunk, &sh->dc_entry));
        }
        break;
    case M_DC_AGC:
        /* steps 1 and 2: the DC maps of every call step 5 will make of this range, and the walk over all of them */
        if (measures && measure_dc(x)) return -1;
        if (rendezvous(x, walk_dc, "the DC measure pass or the walk of another shard failed")) return -1;
        /* step 3: the chain at the start of the range -- the preroll as shadow calls from the walked DC state, no AGC entry -- and the
         * AGC rows of every call of the range */
        if (load_preroll(x)) return -1;
        if (measures) {
            if (alloc_agc_table(x)) return -1;
            CK(iqgpu_chain_dcagc_seek(x->chain, first, x->pre, x->np, x->chunk, &sh->dc_entry, NULL));
            if (for_each_call(x, measure_agc_call)) return -1;
        }
        sh->measure_seconds = now_s() - t_m;
        /* steps 4 and 5: the AGC walk, then the same position again, now with both states of the stream there */
        if (rendezvous(x, walk_agc, "the AGC measure pass or the walk of another shard failed")) return -1;
        CK(iqgpu_chain_dcagc_seek(x->chain, first, x->pre, x->np, x->chunk, &sh->dc_entry, &sh->entry));
        break;
    case M_DC_RMS:
        if (sh->redo_blob) {
            /* the seam in front of this range did not certify: the range again, from where the range in front really ended (the
             * measure pass, the walk and their rendezvous lie behind this shard: its first run has been through them) */
            CK(iqgpu_chain_load_state(x->chain, sh->redo_blob, sh->redo_bytes));
            break;
        }
        if (measures && measure_dc(x)) return -1;
        sh->measure_seconds = now_s() - t_m;
        if (rendezvous(x, walk_dc, "the measure pass or the walk of another shard failed")) return -1;
        /* the chain at the start of the range, behind a preroll of whole calls entered with the walked state; its AGC state for the seam */
        if (sh->first_frame > 0) {
            if (load_preroll(x)) return -1;
            CK(iqgpu_chain_dcrms_seek(x->chain, first, x->pre, x->np, x->chunk, &sh->dc_entry));
            CK(iqgpu_chain_get_agc_state(x->chain, &sh->rms_seek_state));
        }
        break;
    }
    free(x->pre); x->pre = NULL;
    return 0;
}

/* The range through the chain and into its place in the output file.  Software pipeline: iteration i first issues chunk i (H2D,
 * kernels, D2H, all asynchronous), then retires chunk i-1 (waits for its D2H, writes it): chunk i's copies and kernels overlap the
 * write-out of chunk i-1, and buffer i % 2 is free again because chunk i-2 retired last time */
static int stream_range(Ctx *x)
{
    Shard *sh = x->sh;
    const int reads = x->in_fd >= 0 || x->o->have_hash;      /* (bare --synthetic: the buffers keep what ctx_open put there) */
    size_t out_frames[NBUF] = {0};
    long long done_in = 0, written = 0;
    const double t_loop = now_s();
    const long long n_chunks = (long long)range_calls(x);
    for (long long i = 0; i <= n_chunks; i++) {
        if (i < n_chunks) {
            const int b = (int)(i % NBUF);
            size_t n = x->chunk;
            if ((long long)n > sh->frames - done_in) n = (size_t)(sh->frames - done_in);
            if (reads && read_range(x, done_in, n, x->h_in[b])) return -1;
            CK(iqgpu_memcpy_h2d_async(x->d_in[b], x->h_in[b], n * x->ibps, x->s_in));
            CK(iqgpu_event_record(x->e_in[b], x->s_in));
            CK(iqgpu_stream_wait_event(x->s_k, x->e_in[b]));
            CK(iqgpu_chain_process_device(x->chain, x->d_in[b], n, x->d_out[b], x->out_cap, &out_frames[b]));
            /* --psd: behind the chain on its stream, in front of e_k: both buffers stay as they are until the accumulators have read them */
            if (x->psd_in) CK(iqgpu_psd_push_device(x->psd_in, x->d_in[b], n, x->s_k));
            if (x->psd_out) CK(iqgpu_psd_push_device(x->psd_out, x->d_out[b], out_frames[b], x->s_k));
            /* --stats: the same place */
            if (x->st[0]) CK(iqgpu_stats_push_device(x->st[0], x->d_in[b], n, x->s_k));
            if (x->st[1]) CK(iqgpu_stats_push_device(x->st[1], x->d_out[b], out_frames[b], x->s_k));
            /* --sgram: the same place; the rows a call finishes follow on the same stream into pinned memory, so e_out covers them too */
            for (int k = 0; k < 2 && x->sg[k]; k++) {
                const size_t row_bytes = x->sg_opts.nfft * sizeof(float);
                CK(iqgpu_sgram_push_device(x->sg[k], k ? x->d_out[b] : x->d_in[b], k ? out_frames[b] : n, (float *)x->sg_d[k][b], NULL, x->sg_cap[k],
                                           &x->sg_rows[k][b], x->s_k));
                if (x->sg_rows[k][b]) CK(iqgpu_memcpy_d2h_async(x->sg_h[k][b], x->sg_d[k][b], x->sg_rows[k][b] * row_bytes, x->s_k));
            }
            /* --envelope: the same place and the same way */
            for (int k = 0; k < 2 && x->ev[k]; k++) {
                CK(iqgpu_env_push_device(x->ev[k], k ? x->d_out[b] : x->d_in[b], k ? out_frames[b] : n, (float *)x->ev_d[k][b], NULL, NULL, x->ev_cap[k],
                                         &x->ev_rows[k][b], x->s_k));
                if (x->ev_rows[k][b]) CK(iqgpu_memcpy_d2h_async(x->ev_h[k][b], x->ev_d[k][b], x->ev_rows[k][b] * sizeof(float), x->s_k));
            }
            /* --lag: the same place and the same way, two planes */
            for (int k = 0; k < 2 && x->lg[k]; k++) {
                CK(iqgpu_lag_push_device(x->lg[k], k ? x->d_out[b] : x->d_in[b], k ? out_frames[b] : n, (float *)x->lg_d[k][0][b], (float *)x->lg_d[k][1][b],
                                         x->lg_cap[k], &x->lg_rows[k][b], x->s_k));
                if (x->lg_rows[k][b]) {
                    CK(iqgpu_memcpy_d2h_async(x->lg_h[k][0][b], x->lg_d[k][0][b], x->lg_rows[k][b] * 2 * x->lg_opts.n_lags * sizeof(float), x->s_k));
                    CK(iqgpu_memcpy_d2h_async(x->lg_h[k][1][b], x->lg_d[k][1][b], x->lg_rows[k][b] * sizeof(float), x->s_k));
                }
            }
            /* --match: the same place and the same way, three planes */
            for (int k = 0; k < 2 && x->mt[k]; k++) {
                CK(iqgpu_match_push_device(x->mt[k], k ? x->d_out[b] : x->d_in[b], k ? out_frames[b] : n, (float *)x->mt_d[k][0][b], (uint32_t *)x->mt_d[k][1][b],
                                           (float *)x->mt_d[k][2][b], x->mt_cap[k], &x->mt_rows[k][b], x->s_k));
                for (int q = 0; q < 3 && x->mt_rows[k][b]; q++)
                    CK(iqgpu_memcpy_d2h_async(x->mt_h[k][q][b], x->mt_d[k][q][b], x->mt_rows[k][b] * x->mt_opts.n_templates * 4, x->s_k));
            }
            CK(iqgpu_event_record(x->e_k[b], x->s_k));
            CK(iqgpu_stream_wait_event(x->s_out, x->e_k[b]));
            if (out_frames[b]) CK(iqgpu_memcpy_d2h_async(x->h_out[b], x->d_out[b], out_frames[b] * x->obps, x->s_out));
            CK(iqgpu_event_record(x->e_out[b], x->s_out));
            done_in += (long long)n;
        }
        if (i >= 1) {
            const int b = (int)((i - 1) % NBUF);
            float ms;
            CK(iqgpu_event_elapsed_ms(x->e_k[b], x->e_out[b], &ms));    /* synchronises on e_out */
            if (x->out_fd >= 0 && out_frames[b]) {
                const size_t nb = out_frames[b] * x->obps;
                if (pwrite(x->out_fd, x->h_out[b], nb, sh->out_offset_bytes + written * (long long)x->obps) != (ssize_t)nb) FAIL("pwrite: %s", strerror(errno));
            }
            written += (long long)out_frames[b];
            for (int k = 0; k < 2 && x->sg[k]; k++)
                if (fwrite(x->sg_h[k][b], x->sg_opts.nfft * sizeof(float), x->sg_rows[k][b], x->sg_f[k]) != x->sg_rows[k][b]) FAIL("writing the rows of --sgram: %s", strerror(errno));
            for (int k = 0; k < 2 && x->ev[k]; k++) {
                const size_t nr = x->ev_rows[k][b];
                if (fwrite(x->ev_h[k][b], sizeof(float), nr, x->ev_f[k]) != nr) FAIL("writing the rows of --envelope: %s", strerror(errno));
                if (k == 0 && nr) {
                    if (x->ev_all_n + nr > x->ev_all_cap) {
                        const size_t cap = 2 * (x->ev_all_n + nr);
                        float *g = (float *)realloc(x->ev_all, cap * sizeof(float));
                        if (!g) FAIL("--envelope: out of memory for the input's rows");
                        x->ev_all = g; x->ev_all_cap = cap;
                    }
                    memcpy(x->ev_all + x->ev_all_n, x->ev_h[0][b], nr * sizeof(float));
                    x->ev_all_n += nr;
                }
            }
            for (int k = 0; k < 2 && x->lg[k]; k++) {
                const size_t nr = x->lg_rows[k][b], per_row[2] = {2 * (size_t)x->lg_opts.n_lags, 1};
                if (nr && x->lg_all_n[k] + nr > x->lg_all_cap[k]) {
                    const size_t cap = 2 * (x->lg_all_n[k] + nr);
                    for (int q = 0; q < 2; q++) {
                        float *g = (float *)realloc(x->lg_all[k][q], cap * per_row[q] * sizeof(float));
                        if (!g) FAIL("--lag: out of memory for the rows");
                        x->lg_all[k][q] = g;
                    }
                    x->lg_all_cap[k] = cap;
                }
                for (int q = 0; q < 2 && nr; q++) {
                    if (fwrite(x->lg_h[k][q][b], per_row[q] * sizeof(float), nr, x->lg_f[k][q]) != nr) FAIL("writing the rows of --lag: %s", strerror(errno));
                    memcpy(x->lg_all[k][q] + x->lg_all_n[k] * per_row[q], x->lg_h[k][q][b], nr * per_row[q] * sizeof(float));
                }
                x->lg_all_n[k] += nr;
            }
            for (int k = 0; k < 2 && x->mt[k]; k++) {
                const size_t nr = x->mt_rows[k][b], per_row = x->mt_opts.n_templates;
                if (nr && x->mt_all_n[k] + nr > x->mt_all_cap[k]) {
                    const size_t cap = 2 * (x->mt_all_n[k] + nr);
                    for (int q = 0; q < 3; q++) {
                        uint32_t *g = (uint32_t *)realloc(x->mt_all[k][q], cap * per_row * 4);
                        if (!g) FAIL("--match: out of memory for the rows");
                        x->mt_all[k][q] = g;
                    }
                    x->mt_all_cap[k] = cap;
                }
                for (int q = 0; q < 3 && nr; q++) {
                    if (fwrite(x->mt_h[k][q][b], per_row * 4, nr, x->mt_f[k][q]) != nr) FAIL("writing the rows of --match: %s", strerror(errno));
                    memcpy(x->mt_all[k][q] + x->mt_all_n[k] * per_row, x->mt_h[k][q][b], nr * per_row * 4);
                }
                x->mt_all_n[k] += nr;
            }
        }
    }
    sh->frames_out = written;
    sh->stream_seconds = now_s() - t_loop;
    if (written != sh->planned_out) FAIL("shard %d produced %lld frames, its place in the output was planned for %lld", sh->shard, written, sh->planned_out);
    return 0;
}

/* --psd PREFIX: PREFIX.in.f64 and PREFIX.out.f64 -- sum_power of the input and of the output, nfft little-endian doubles each, natural
 * bin order -- and PREFIX.json with both info records and the two rates */
/* s as the inside of a JSON string: quotes, backslashes and control characters escaped */
static void json_put(FILE *f, const char *s)
{
    for (; *s; s++) {
        const unsigned char c = (unsigned char)*s;
        if (c == '"' || c == '\\') fprintf(f, "\\%c", c);
        else if (c < 0x20) fprintf(f, "\\u%04x", c);
        else fputc(c, f);
    }
}

static int write_psd(Ctx *x)
{
    static const char *const window_name[4] = {"rect", "hann", "hamming", "blackman_harris"};   /* IQGPU_PSD_* */
    Shard *sh = x->sh;
    const Options *o = x->o;
    iqgpu_psd *acc[2] = {x->psd_in, x->psd_out};
    static const char *const side[2] = {"in", "out"};
    const double rate[2] = {x->d.input_rate_hz, x->d.target_rate_hz};
    iqgpu_psd_info info[2];
    char path[4096];
    for (int k = 0; k < 2; k++) {
        double sum[4096];
        CK(iqgpu_psd_read(acc[k], sum, NULL, &info[k]));
        snprintf(path, sizeof(path), "%s.%s.f64", o->psd_prefix, side[k]);
        FILE *f = fopen(path, "wb");
        if (!f) FAIL("writing %.160s: %s", path, strerror(errno));
        const int short_write = fwrite(sum, sizeof(double), info[k].nfft, f) != info[k].nfft;
        if ((fclose(f) != 0) | short_write) FAIL("writing %.160s: %s", path, strerror(errno));
    }
    snprintf(path, sizeof(path), "%s.json", o->psd_prefix);
    FILE *f = fopen(path, "w");
    if (!f) FAIL("writing %.160s: %s", path, strerror(errno));
    fprintf(f, "{");
    for (int k = 0; k < 2; k++) {
        fprintf(f, "%s\"%s\": {\"rate_hz\": %.17g, \"frames\": %llu, \"segments\": %llu, \"nfft\": %u, \"hop\": %u, \"window\": \"%s\", \"window_sum\": %.17g, "
                "\"window_sum_sq\": %.17g, \"file\": \"", k ? ", " : "", side[k], rate[k], (unsigned long long)info[k].frames,
                (unsigned long long)info[k].segments, info[k].nfft, info[k].hop, window_name[x->psd_opts.window & 3], info[k].window_sum, info[k].window_sum_sq);
        json_put(f, o->psd_prefix);
        fprintf(f, ".%s.f64\"}", side[k]);
    }
    fprintf(f, "}\n");
    if (fclose(f) != 0) FAIL("writing %.160s: %s", path, strerror(errno));
    return 0;
}

/* --stats: this shard's two results, for main to merge in shard order */
static int read_stats(Ctx *x)
{
    Shard *sh = x->sh;
    for (int k = 0; k < 2; k++) CK(iqgpu_stats_read(x->st[k], &sh->stats[k]));
    return 0;
}

static void json_u64s(FILE *f, const char *name, const uint64_t *v, int n)
{
    fprintf(f, "\"%s\": [", name);
    for (int i = 0; i < n; i++) fprintf(f, "%s%llu", i ? ", " : "", (unsigned long long)v[i]);
    fprintf(f, "]");
}

/* --stats PREFIX: PREFIX.json -- the shards' results concatenated in shard order, every field of both, and both derived records */
static int write_stats(const Options *o, Shard *sh)
{
    static const char *const side[2] = {"in", "out"};
    char path[4096];
    snprintf(path, sizeof(path), "%s.json", o->stats_prefix);
    FILE *f = fopen(path, "w");
    if (!f) REFUSE(1, "writing %.160s: %s\n", path, strerror(errno));
    fprintf(f, "{\"shards\": %d", o->shards);
    for (int k = 0; k < 2; k++) {
        iqgpu_stats_result *r = &sh[0].stats[k];
        iqgpu_stats_derived d;
        for (int s = 1; s < o->shards; s++) iqgpu_stats_merge(r, &sh[s].stats[k]);
        iqgpu_stats_derive(r, &d);
        fprintf(f, ", \"%s\": {\"frames\": %llu, \"nonfinite_frames\": %llu, ", side[k], (unsigned long long)r->frames, (unsigned long long)r->nonfinite_frames);
        json_u64s(f, "rail_lo", r->rail_lo, 2); fprintf(f, ", ");
        json_u64s(f, "rail_hi", r->rail_hi, 2); fprintf(f, ", \"hist\": [");
        for (int c = 0; c < 2; c++) { fprintf(f, "%s[", c ? ", " : ""); for (int b = 0; b < 256; b++) fprintf(f, "%s%llu", b ? ", " : "", (unsigned long long)r->hist[c][b]); fprintf(f, "]"); }
        fprintf(f, "], \"min\": [%.17g, %.17g], \"max\": [%.17g, %.17g],\"peak_power\": %.17g, \"peak_frame\": %llu, \"sum\": [%.17g, %.17g], "
                "\"sum_sq\": [%.17g, %.17g], \"sum_iq\": %.17g, ", r->min[0], r->min[1], r->max[0], r->max[1], r->peak_power, (unsigned long long)r->peak_frame,
                r->sum[0], r->sum[1], r->sum_sq[0], r->sum_sq[1], r->sum_iq);
        fprintf(f, "\"derived\": {\"n\": %llu, \"mean_i\": %.17g, \"mean_q\": %.17g, \"power\": %.17g, \"rms_dbfs\": %.17g, \"peak_dbfs\": %.17g, \"crest_db\": %.17g, "
                "\"var_i\": %.17g, \"var_q\": %.17g, \"iq_gain_ratio\": %.17g, \"iq_phase_rad\": %.17g, \"clip_fraction\": %.17g, \"bins_used\": [%u, %u]}}",
                (unsigned long long)d.n, d.mean_i, d.mean_q, d.power, d.rms_dbfs, d.peak_dbfs, d.crest_db, d.var_i, d.var_q, d.iq_gain_ratio, d.iq_phase_rad,
                d.clip_fraction, d.bins_used[0], d.bins_used[1]);
    }
    fprintf(f, "}\n");
    if (fclose(f) != 0) REFUSE(1, "writing %.160s: %s\n", path, strerror(errno));
    return 0;
}

/* --sgram PREFIX: the row files are complete (stream_range appended every finished row); PREFIX.json with both info records and the two
 * rates.  The partial last row stays unwritten: open_segments says how many segments it held */
static int write_sgram(Ctx *x)
{
    static const char *const window_name[4] = {"rect", "hann", "hamming", "blackman_harris"};   /* IQGPU_PSD_* */
    static const char *const side[2] = {"in", "out"};
    Shard *sh = x->sh;
    const Options *o = x->o;
    const double rate[2] = {x->d.input_rate_hz, x->d.target_rate_hz};
    char path[4096];
    snprintf(path, sizeof(path), "%s.json", o->sgram_prefix);
    FILE *f = fopen(path, "w");
    if (!f) FAIL("writing %.160s: %s", path, strerror(errno));
    fprintf(f, "{");
    for (int k = 0; k < 2; k++) {
        iqgpu_sgram_info info;
        FILE *rows = x->sg_f[k];
        x->sg_f[k] = NULL;
        if (fclose(rows) != 0) { fclose(f); FAIL("writing %.160s.%s.f32: %s", o->sgram_prefix, side[k], strerror(errno)); }
        if (iqgpu_sgram_read_open(x->sg[k], NULL, NULL, &info) != IQGPU_OK) { fclose(f); FAIL("%s", iqgpu_last_error()); }
        fprintf(f, "%s\"%s\": {\"rate_hz\": %.17g, \"frames\": %llu, \"segments\": %llu, \"rows\": %llu, \"open_segments\": %u, \"nfft\": %u, \"hop\": %u, "
                "\"row_segments\": %u, \"window\": \"%s\", \"window_sum\": %.17g, \"window_sum_sq\": %.17g, \"file\": \"", k ? ", " : "", side[k], rate[k],
                (unsigned long long)info.frames, (unsigned long long)info.segments, (unsigned long long)info.rows, info.open_segments, info.nfft, info.hop,
                info.row_segments, window_name[x->sg_opts.window & 3], info.window_sum, info.window_sum_sq);
        json_put(f, o->sgram_prefix);
        fprintf(f, ".%s.f32\"}", side[k]);
    }
    fprintf(f, "}\n");
    if (fclose(f) != 0) FAIL("writing %.160s: %s", path, strerror(errno));
    return 0;
}

/* --envelope PREFIX: the row files are complete (stream_range appended every finished row); PREFIX.json with B, both info records, both
 * open rows and the bursts of the input */
static int write_env(Ctx *x)
{
    static const char *const side[2] = {"in", "out"};
    Shard *sh = x->sh;
    const Options *o = x->o;
    const double rate[2] = {x->d.input_rate_hz, x->d.target_rate_hz};
    const uint32_t B = x->ev_opts.block_frames;
    char path[4096];
    snprintf(path, sizeof(path), "%s.json", o->env_prefix);
    FILE *f = fopen(path, "w");
    if (!f) FAIL("writing %.160s: %s", path, strerror(errno));
    fprintf(f, "{\"block_frames\": %u", B);
    for (int k = 0; k < 2; k++) {
        iqgpu_env_info info;
        double sum = 0.0, peak = 0.0;
        uint32_t rail = 0;
        FILE *rows = x->ev_f[k];
        x->ev_f[k] = NULL;
        if (fclose(rows) != 0) { fclose(f); FAIL("writing %.160s.%s.f32: %s", o->env_prefix, side[k], strerror(errno)); }
        if (iqgpu_env_read_open(x->ev[k], &sum, &peak, &rail, &info) != IQGPU_OK) { fclose(f); FAIL("%s", iqgpu_last_error()); }
        fprintf(f, ", \"%s\": {\"rate_hz\": %.17g, \"frames\": %llu, \"rows\": %llu, \"nonfinite_frames\": %llu, \"open_frames\": %u, "
                "\"open\": {\"sum\": %.17g, \"peak\": %.17g, \"rail\": %u}, \"file\": \"", side[k], rate[k], (unsigned long long)info.frames,
                (unsigned long long)info.rows, (unsigned long long)info.nonfinite_frames, info.open_frames, sum, peak, rail);
        json_put(f, o->env_prefix);
        fprintf(f, ".%s.f32\"}", side[k]);
    }
    /* the bursts of the input: thresholds 10 dB and 7 dB over the row at the tenth percentile */
    iqgpu_env_burst_opts bo;
    memset(&bo, 0, sizeof(bo));
    bo.block_frames = B; bo.min_rows = 2; bo.hang_rows = 2; bo.pad_rows = 1;
    fprintf(f, ", \"min_rows\": %u, \"hang_rows\": %u, \"pad_rows\": %u", bo.min_rows, bo.hang_rows, bo.pad_rows);
    if (x->ev_all_n == 0) {
        fprintf(f, ", \"floor\": null, \"on\": null, \"off\": null, \"bursts\": []}\n");
    } else {
        double fl = 0.0;
        size_t n = 0;
        if (iqgpu_env_floor(x->ev_all, x->ev_all_n, B, 0.1, &fl) != IQGPU_OK) { fclose(f); FAIL("%s", iqgpu_last_error()); }
        bo.on = fl * 10.0; bo.off = fl * 5.011872336272722;             /* 10^(10 / 10), 10^(7 / 10) */
        (void)iqgpu_env_bursts(x->ev_all, x->ev_all_n, &bo, NULL, 0, &n);   /* (the count: IQGPU_ECAPACITY) */
        iqgpu_env_burst *bu = (iqgpu_env_burst *)calloc(n ? n : 1, sizeof(*bu));
        if (!bu) { fclose(f); FAIL("--envelope: out of memory for %zu bursts", n); }
        if (iqgpu_env_bursts(x->ev_all, x->ev_all_n, &bo, bu, n, &n) != IQGPU_OK) { free(bu); fclose(f); FAIL("%s", iqgpu_last_error()); }
        fprintf(f, ", \"floor\": %.17g, \"on\": %.17g, \"off\": %.17g, \"bursts\": [", fl, bo.on, bo.off);
        for (size_t i = 0; i < n; i++)
            fprintf(f, "%s{\"first_frame\": %llu, \"frames\": %llu, \"peak_row\": %llu, \"peak_mean\": %.17g}", i ? ", " : "",
                    (unsigned long long)bu[i].first_frame, (unsigned long long)bu[i].frames, (unsigned long long)bu[i].peak_row, bu[i].peak_mean);
        fprintf(f, "]}\n");
        free(bu);
    }
    if (fclose(f) != 0) FAIL("writing %.160s: %s", path, strerror(errno));
    return 0;
}

/* --lag PREFIX: the row files are complete (stream_range appended every finished row); PREFIX.json with the options, both info records and
 * the estimate over all rows of each side per lag */
static int write_lag(Ctx *x)
{
    static const char *const side[2] = {"in", "out"}, *const plane[2] = {"lag", "sum"};
    Shard *sh = x->sh;
    const Options *o = x->o;
    const double rate[2] = {x->d.input_rate_hz, x->d.target_rate_hz};
    const iqgpu_lag_opts *lo = &x->lg_opts;
    char path[4096];
    snprintf(path, sizeof(path), "%s.json", o->lag_prefix);
    FILE *f = fopen(path, "w");
    if (!f) FAIL("writing %.160s: %s", path, strerror(errno));
    fprintf(f, "{\"block_frames\": %u, \"lags\": [", lo->block_frames);
    for (uint32_t l = 0; l < lo->n_lags; l++) fprintf(f, "%s%u", l ? ", " : "", lo->lags[l]);
    fprintf(f, "]");
    for (int k = 0; k < 2; k++) {
        iqgpu_lag_info info;
        for (int q = 0; q < 2; q++) {
            FILE *rows = x->lg_f[k][q];
            x->lg_f[k][q] = NULL;
            if (fclose(rows) != 0) { fclose(f); FAIL("writing %.160s.%s.%s.f32: %s", o->lag_prefix, side[k], plane[q], strerror(errno)); }
        }
        if (iqgpu_lag_read_open(x->lg[k], NULL, NULL, &info) != IQGPU_OK) { fclose(f); FAIL("%s", iqgpu_last_error()); }
        fprintf(f, ", \"%s\": {\"sample_rate\": %.17g, \"frames\": %llu, \"rows\": %llu, \"nonfinite_frames\": %llu, \"open_frames\": %u, \"estimates\": [",
                side[k], rate[k], (unsigned long long)info.frames, (unsigned long long)info.rows, (unsigned long long)info.nonfinite_frames, info.open_frames);
        for (uint32_t l = 0; l < lo->n_lags; l++) {
            static const float none[2] = {0.0f, 0.0f};
            iqgpu_lag_estimate e;
            const size_t n = x->lg_all_n[k];
            if (iqgpu_lag_estimate_rows(n ? x->lg_all[k][0] : none, n ? x->lg_all[k][1] : none, n, lo, l, 0, n, rate[k], &e) != IQGPU_OK) {
                fclose(f); FAIL("%s", iqgpu_last_error());
            }
            fprintf(f, "%s{\"lag\": %u, \"re\": %.17g, \"im\": %.17g, \"power\": %.17g, \"hz\": %.17g, \"coherence\": %.17g, \"span_hz\": %.17g}",
                    l ? ", " : "", lo->lags[l], e.re, e.im, e.power, e.hz, e.coherence, e.span_hz);
        }
        fprintf(f, "], \"files\": [\"");
        json_put(f, o->lag_prefix);
        fprintf(f, ".%s.lag.f32\", \"", side[k]);
        json_put(f, o->lag_prefix);
        fprintf(f, ".%s.sum.f32\"]}", side[k]);
    }
    fprintf(f, "}\n");
    if (fclose(f) != 0) FAIL("writing %.160s: %s", path, strerror(errno));
    return 0;
}

/* --match PREFIX: the row files are complete; PREFIX.json with the options, both info records and the detections of each side over all
 * its rows (iqgpu_match_peaks at MATCH_RATIO) */
static int write_match(Ctx *x)
{
    static const char *const side[2] = {"in", "out"}, *const plane[3] = {"peak.f32", "at.u32", "sum.f32"};
    Shard *sh = x->sh;
    const Options *o = x->o;
    const double rate[2] = {x->d.input_rate_hz, x->d.target_rate_hz};
    const iqgpu_match_opts *mo = &x->mt_opts;
    char path[4096];
    snprintf(path, sizeof(path), "%s.json", o->match_prefix);
    FILE *f = fopen(path, "w");
    if (!f) FAIL("writing %.160s: %s", path, strerror(errno));
    fprintf(f, "{\"nfft\": %u, \"block_frames\": %u, \"n_templates\": %u, \"template_frames\": %u, \"ratio\": %.17g, \"shifts_hz\": [", mo->nfft,
            mo->block_frames, mo->n_templates, mo->template_frames, MATCH_RATIO);
    for (uint32_t i = 0; i < x->mt_nhz; i++) fprintf(f, "%s%.17g", i ? ", " : "", x->mt_hz[i]);
    fprintf(f, "]");
    for (int k = 0; k < 2; k++) {
        static const uint32_t none[8] = {0};
        iqgpu_match_info info;
        const size_t n = x->mt_all_n[k];
        size_t found = 0;
        for (int q = 0; q < 3; q++) {
            FILE *rows = x->mt_f[k][q];
            x->mt_f[k][q] = NULL;
            if (fclose(rows) != 0) { fclose(f); FAIL("writing %.160s.%s.%s: %s", o->match_prefix, side[k], plane[q], strerror(errno)); }
        }
        if (iqgpu_match_read_open(x->mt[k], NULL, NULL, NULL, &info) != IQGPU_OK) { fclose(f); FAIL("%s", iqgpu_last_error()); }
        const float *pk = n ? (const float *)x->mt_all[k][0] : (const float *)none, *sm = n ? (const float *)x->mt_all[k][2] : (const float *)none;
        const uint32_t *at = n ? x->mt_all[k][1] : none;
        int rc = iqgpu_match_peaks(pk, at, sm, n, mo, MATCH_RATIO, NULL, 0, &found);      /* the count first */
        iqgpu_match_peak *d = (iqgpu_match_peak *)malloc((found ? found : 1) * sizeof(*d));
        if ((rc != IQGPU_OK && rc != IQGPU_ECAPACITY) || !d) { free(d); fclose(f); FAIL("--match: %s", d ? iqgpu_last_error() : "out of memory for the detections"); }
        if (iqgpu_match_peaks(pk, at, sm, n, mo, MATCH_RATIO, d, found, &found) != IQGPU_OK) { free(d); fclose(f); FAIL("%s", iqgpu_last_error()); }
        fprintf(f, ", \"%s\": {\"sample_rate\": %.17g, \"frames\": %llu, \"segments\": %llu, \"rows\": %llu, \"open_segments\": %u, \"template_energy\": [",
                side[k], rate[k], (unsigned long long)info.frames, (unsigned long long)info.segments, (unsigned long long)info.rows, info.open_segments);
        for (uint32_t t = 0; t < mo->n_templates; t++) fprintf(f, "%s%.17g", t ? ", " : "", info.template_energy[t]);
        fprintf(f, "], \"detections\": [");
        for (size_t i = 0; i < found; i++) {
            fprintf(f, "%s{\"first_frame\": %llu, \"template\": %u, \"peak\": %.9g, \"ratio\": ", i ? ", " : "", (unsigned long long)d[i].first_frame,
                    d[i].template_index, (double)d[i].peak);
            if (d[i].ratio - d[i].ratio == 0.0) fprintf(f, "%.17g}", d[i].ratio); else fprintf(f, "null}");      /* (+inf: the row's other positions hold no power) */
        }
        free(d);
        fprintf(f, "], \"files\": [");
        for (int q = 0; q < 3; q++) {
            fprintf(f, "%s\"", q ? ", " : "");
            json_put(f, o->match_prefix);
            fprintf(f, ".%s.%s\"", side[k], plane[q]);
        }
        fprintf(f, "]}");
    }
    fprintf(f, "}\n");
    if (fclose(f) != 0) FAIL("writing %.160s: %s", path, strerror(errno));
    return 0;
}

/* --seamless-rms, --seamless-dc-rms: what the seam behind this range is checked against, and what the range behind it restarts from if the check fails */
static int save_checkpoint(Ctx *x)
{
    Shard *sh = x->sh;
    size_t need = 0;
    CK(iqgpu_chain_get_agc_state(x->chain, &sh->rms_end_state));
    (void)iqgpu_chain_save_state(x->chain, NULL, 0, &need);          /* (a size query: IQGPU_ECAPACITY) */
    free(sh->blob);
    sh->blob = malloc(need ? need : 1);
    if (!sh->blob) FAIL("out of memory for a checkpoint of %zu bytes", need);
    CK(iqgpu_chain_save_state(x->chain, sh->blob, need, &sh->blob_bytes));
    return 0;
}

static void *run_shard(void *arg)
{
    Shard *sh = (Shard *)arg;
    const Options *o = sh->opt;
    Ctx x;
    const double t0 = now_s();
    memset(&x, 0, sizeof(x));
    x.sh = sh; x.o = o; x.in_fd = x.out_fd = -1;
    x.d = o->desc;
    x.d.device_ordinal = o->device0 + (sh->shard % o->devices);
    x.ibps = iqgpu_get_bytes_per_sample(x.d.in_format); x.obps = iqgpu_get_bytes_per_sample(x.d.out_format);

    /* this thread -- and with it the pages it touches first and the buffers it pins -- onto the socket of its GPU, before anything
     * touches that GPU.  Best effort: a host that hides its topology leaves the thread where it is (numa_node stays -1) */
    sh->device = x.d.device_ordinal; sh->numa_node = -1;
    if (!o->no_bind) { int node = -1; if (iqgpu_bind_thread_to_device(x.d.device_ordinal, &node) == IQGPU_OK) sh->numa_node = node; }

    if (o->dry) dry_shard(&x);
    else {
        if (!ctx_open(&x) && !enter_stream(&x) && !stream_range(&x) && !(o->psd_prefix && write_psd(&x)) && !(o->sgram_prefix && write_sgram(&x)) && !(o->env_prefix && write_env(&x)) && !(o->lag_prefix && write_lag(&x)) && !(o->match_prefix && write_match(&x)) && !(o->stats_prefix && read_stats(&x)) && MODES[o->mode].certify) save_checkpoint(&x);
        /* (a shard that fails early still keeps the rendezvous of the passes: the others wait there) */
        while (sh->barriers < MODES[o->mode].barriers) rendezvous(&x, NULL, NULL);
    }
    ctx_close(&x);
    sh->seconds = now_s() - t0;
    return NULL;
}

static void usage(void)
{
    fprintf(stderr,
            "iqgpu_run -i IN --raw-file-input-rate HZ --raw-file-input-sample-format FMT -o OUT --output-rate HZ\n"
            "          [--output-sample-format FMT] [--freq-shift HZ] [--shift-after-resample] [--gain G] [--dc-block]\n"
            "          [--iq-factors MAG:PHASE | --iq-calibrate (the factors from the head of the input, printed as --iq-factors takes them)] [--no-resample] [--lowpass HZ] [--highpass HZ] [--pass-range A:B] [--stopband A:B]\n"
            "          [--transition-width HZ] [--attenuation DB] [--filter-taps N] [--filter-type fir|fft] [--filter-fft-size N]\n"
            "          [--chunk-frames N (default 4194304)] [--shards N] [--devices N] [--device D] [--synthetic FRAMES [--synthetic-hash SEED]]\n"
            "          [--seamless (with --shards: the shards continue ONE stream -- the stitched output is what --shards 1 writes)]\n"
            "          [--seamless-agc (--seamless for chains with the digital output AGC: a measure pass, one walk, then the ordinary pass)]\n"
            "          [--seamless-dc (the exact --seamless for --dc-block chains without an AGC: a measure pass over the input, one walk, then the ordinary pass)]\n"
            "          [--seamless-rms (--seamless for chains with the dx / local output AGC: seek from a bounded window, seams certified, a range behind a seam that is not is redone)]\n"
            "          [--seamless-dc-rms (the exact --seamless for --dc-block chains with the dx / local AGC: DC measure, walk, then --seamless-rms's seek, certificate and redo)]\n"
            "          [--seamless-dc-agc (the exact --seamless for --dc-block chains with the digital AGC: DC measure, walk, shadow AGC measure, walk, then the ordinary pass)]\n"
            "          [--stats PREFIX (plain runs and independent --shards: counts, rails, extrema, peak, histogram and moments of the input and of the output bytes, merged in shard order, as PREFIX.json)]\n"
            "          [--psd PREFIX (plain single-stream runs: the power spectra of the input and of the output -- Hann, 1024 bins -- as PREFIX.in.f64, PREFIX.out.f64, PREFIX.json)]\n"
            "          [--lag PREFIX [--lag-list d1,d2,..] [--lag-block B] (the same runs: the lag products x[n] conj(x[n - d]) and the power per row of B frames (4096) of the input and of the output for up to four lags d (1), rows appended as they finish to PREFIX.in.lag.f32, PREFIX.in.sum.f32, PREFIX.out.lag.f32, PREFIX.out.sum.f32; PREFIX.json with the frequency estimate and the coherence per lag)]\n"
            "          [--match PREFIX --match-template FILE.cf32 [--match-block B] [--match-shifts hz1,hz2,..] (the same runs: the correlation of the input and of the output with the template of 2 .. 2049 cf32 frames in FILE.cf32 -- with --match-shifts, with its one to eight copies shifted by those offsets in Hz -- per row of B start positions (4096): the largest power, where it is and the sum, rows appended as they finish to PREFIX.{in,out}.peak.f32 / .at.u32 / .sum.f32; PREFIX.json with the detections at ratio 100)]\n"
            "          [--envelope PREFIX [--envelope-block B] (the same runs: the power per row of B frames (4096) of the input and of the output, rows appended as they finish to PREFIX.in.f32, PREFIX.out.f32; PREFIX.json with the bursts of the input)]\n"
            "          [--sgram PREFIX [--sgram-row-segments R] (the same runs: the spectrum per row of R segments (32) of the input and of the output, rows appended as they finish to PREFIX.in.f32, PREFIX.out.f32; PREFIX.json)]\n"
            "          [--no-numa-bind] [--quiet] [--debug NAME=VALUE (iqgpu_debug_set)]\n"
            "          [--dry-placement (plan the shards, bind every shard thread, size its buffers, report as JSON: no GPU call)]\n");
}

/* the command line into *o; 0, or the exit status */
static int parse_args(int argc, char **argv, Options *o)
{
    memset(o, 0, sizeof(*o));
    iqgpu_chain_desc_init(&o->desc);
    o->chunk_frames = 1u << 22; o->shards = 1; o->devices = 1;
    double in_rate = 0, out_rate = 0;
    for (int i = 1; i < argc; i++) {
        const char *a = argv[i];
#define NEXT (i + 1 < argc ? argv[++i] : (usage(), exit(2), ""))
        if (!strcmp(a, "-i") || !strcmp(a, "--input")) { const char *v = NEXT; if (!strcmp(v, "raw-file")) v = NEXT; o->in_path = v; }
        else if (!strcmp(a, "-o") || !strcmp(a, "--output")) { const char *v = NEXT; if (!strcmp(v, "raw-file")) v = NEXT; o->out_path = v; }
        else if (!strcmp(a, "--raw-file-input-rate")) in_rate = atof(NEXT);
        else if (!strcmp(a, "--raw-file-input-sample-format")) o->desc.in_format = fmt_from_name(NEXT);
        else if (!strcmp(a, "--output-rate")) out_rate = atof(NEXT);
        else if (!strcmp(a, "--output-sample-format")) o->desc.out_format = fmt_from_name(NEXT);
        else if (!strcmp(a, "--freq-shift")) o->desc.shift_hz = atof(NEXT);
        else if (!strcmp(a, "--shift-after-resample")) o->desc.shift_after_resample = 1;
        else if (!strcmp(a, "--gain")) o->desc.gain = (float)atof(NEXT);
        else if (!strcmp(a, "--dc-block")) o->desc.dc_block_enable = 1;
        else if (!strcmp(a, "--iq-factors")) { o->desc.iq_correct_enable = 1; o->have_iq_factors = 1; sscanf(NEXT, "%f:%f", &o->desc.iq_mag, &o->desc.iq_phase); }
        else if (!strcmp(a, "--iq-calibrate")) o->iq_calibrate = 1;
        else if (!strcmp(a, "--psd")) o->psd_prefix = NEXT;
        else if (!strcmp(a, "--stats")) o->stats_prefix = NEXT;
        else if (!strcmp(a, "--sgram")) o->sgram_prefix = NEXT;
        else if (!strcmp(a, "--envelope")) o->env_prefix = NEXT;
        else if (!strcmp(a, "--lag")) o->lag_prefix = NEXT;
        else if (!strcmp(a, "--lag-list")) o->lag_list = NEXT;
        else if (!strcmp(a, "--lag-block")) { const long long r = atoll(NEXT); o->lag_block = r >= 64 && r <= (1 << 24) && (r & (r - 1)) == 0 ? (unsigned)r : ~0u; }
        else if (!strcmp(a, "--match")) o->match_prefix = NEXT;
        else if (!strcmp(a, "--match-template")) o->match_template = NEXT;
        else if (!strcmp(a, "--match-shifts")) o->match_shifts = NEXT;
        else if (!strcmp(a, "--match-block")) { const long long r = atoll(NEXT); o->match_block = r >= 512 && r <= (1 << 24) && (r & (r - 1)) == 0 ? (unsigned)r : ~0u; }
        else if (!strcmp(a, "--envelope-block")) { const long long r = atoll(NEXT); o->env_block = r >= 64 && r <= (1 << 24) && (r & (r - 1)) == 0 ? (unsigned)r : ~0u; }
        else if (!strcmp(a, "--sgram-row-segments")) { const long long r = atoll(NEXT); o->sgram_row_segments = r >= 1 && r <= (1 << 20) ? (unsigned)r : ~0u; }
        else if (!strcmp(a, "--no-resample")) o->desc.no_resample = 1;
        else if (!strcmp(a, "--lowpass") || !strcmp(a, "--highpass")) {
            if (o->desc.n_filters >= 5) REFUSE(2, "at most 5 filters\n");
            iqgpu_filter_req *r = &o->desc.filters[o->desc.n_filters++];
            r->type = !strcmp(a, "--lowpass") ? IQGPU_FILTER_LOWPASS : IQGPU_FILTER_HIGHPASS; r->f1_hz = (float)atof(NEXT); r->f2_hz = 0;
        } else if (!strcmp(a, "--pass-range") || !strcmp(a, "--stopband")) {
            if (o->desc.n_filters >= 5) REFUSE(2, "at most 5 filters\n");
            float s = 0, e = 0; sscanf(NEXT, "%f:%f", &s, &e);
            iqgpu_filter_req *r = &o->desc.filters[o->desc.n_filters++];
            r->type = !strcmp(a, "--pass-range") ? IQGPU_FILTER_PASSBAND : IQGPU_FILTER_STOPBAND;
            const float bw = e - s; r->f1_hz = s + (bw / 2.0f); r->f2_hz = bw;     /* src/config.c:203-214 */
        }
        else if (!strcmp(a, "--transition-width")) o->desc.transition_width_hz = (float)atof(NEXT);
        else if (!strcmp(a, "--attenuation")) o->desc.attenuation_db = (float)atof(NEXT);
        else if (!strcmp(a, "--filter-taps")) { int t = atoi(NEXT); if (t && t % 2 == 0) t++; o->desc.filter_taps = t; }   /* src/config.c:233-236 */
        else if (!strcmp(a, "--filter-type")) { const char *v = NEXT; o->desc.filter_impl = !strcmp(v, "fft") ? IQGPU_FILTER_IMPL_FFT : IQGPU_FILTER_IMPL_FIR; }
        else if (!strcmp(a, "--filter-fft-size")) o->desc.fft_size = atoi(NEXT);
        else if (!strcmp(a, "--output-agc")) { o->desc.agc_enable = 1; if (!o->desc.agc_profile) o->desc.agc_profile = IQGPU_AGC_LOCAL; }   /* src/config.c:306-310 */
        else if (!strcmp(a, "--agc-profile")) { const char *v = NEXT; o->desc.agc_enable = 1;
            o->desc.agc_profile = !strcasecmp(v, "dx") ? IQGPU_AGC_DX : !strcasecmp(v, "local") ? IQGPU_AGC_LOCAL : !strcasecmp(v, "digital") ? IQGPU_AGC_DIGITAL : -1; }
        else if (!strcmp(a, "--agc-target")) o->desc.agc_target = (float)atof(NEXT);
        else if (!strcmp(a, "--chunk-frames")) o->chunk_frames = (size_t)atoll(NEXT);
        else if (!strcmp(a, "--shards")) { o->shards = atoi(NEXT); o->have_shards = 1; }
        else if (!strcmp(a, "--devices")) o->devices = atoi(NEXT);
        else if (!strcmp(a, "--device")) o->device0 = atoi(NEXT);
        else if (!strcmp(a, "--synthetic")) o->synthetic_frames = atoll(NEXT);
        else if (!strcmp(a, "--synthetic-hash")) { o->have_hash = 1; o->hash_seed = strtoull(NEXT, NULL, 0); }
        else if (!strcmp(a, "--no-numa-bind")) o->no_bind = 1;
        else if (!strcmp(a, "--dry-placement")) o->dry = 1;
        else if (!strcmp(a, "--debug")) {              /* --debug name=value -> iqgpu_debug_set (the library reads no environment) */
            char kv[512]; snprintf(kv, sizeof(kv), "%s", NEXT);
            char *eq = strchr(kv, '=');
            if (!eq) REFUSE(2, "--debug wants name=value\n");
            *eq = 0;
            if (iqgpu_debug_set(kv, eq + 1) != IQGPU_OK) REFUSE(2, "%s\n", iqgpu_last_error());
        }
        else if (!strcmp(a, "--quiet")) o->quiet = 1;
        else {
            Mode m = M_INDEPENDENT;
            for (int k = M_SEAMLESS; k < M_COUNT; k++) if (!strcmp(a, MODES[k].flag)) m = (Mode)k;
            if (m == M_INDEPENDENT) { usage(); return 2; }
            if (o->mode == M_INDEPENDENT) o->mode = m;
            else if (o->mode != m) o->clash = m;
        }
#undef NEXT
    }
    if (o->desc.in_format < 0 || o->desc.out_format < 0) REFUSE(2, "unknown sample format\n");
    if (o->have_hash && (o->synthetic_frames <= 0 || o->desc.in_format == IQGPU_FMT_CF32)) REFUSE(2, "--synthetic-hash needs --synthetic FRAMES and an integer input format\n");
    if (!(in_rate > 0) || (!o->desc.no_resample && !(out_rate > 0)) || (!o->in_path && o->synthetic_frames <= 0)) { usage(); return 2; }
    o->desc.input_rate_hz = in_rate; o->desc.target_rate_hz = o->desc.no_resample ? in_rate : out_rate;
    if (o->shards < 1) o->shards = 1;
    if (o->devices < 1) o->devices = 1;
    return 0;
}

/* What the job's mode asks, before anything is looked at or planned; 0, or the exit status.  Options that do not go together: 2, as for
 * every other misuse of the command line.  A chain the recipe does not cover -- what the library would refuse at its first call, in the
 * library's words -- : 1 */
static int validate(const Options *o)
{
    const ModeRow *m = &MODES[o->mode];
    const size_t agc_chunk = agc_chunk_of(&o->desc);
    if (o->clash != M_INDEPENDENT) REFUSE(2, "%s excludes %s\n", m->flag, MODES[o->clash].flag);
    if (o->iq_calibrate && o->have_iq_factors) REFUSE(2, "--iq-calibrate excludes --iq-factors\n");
    /* (the spectrum of ONE stream as one accumulator sees it: sharded spectra are a sum on the host that nothing here defines yet) */
    if (o->psd_prefix && (o->have_shards || o->mode != M_INDEPENDENT || o->iq_calibrate))
        REFUSE(2, "usage: --psd is for plain single-stream runs: it excludes --shards, every --seamless* mode and --iq-calibrate\n");
    if (o->psd_prefix && strlen(o->psd_prefix) > 3000) REFUSE(2, "usage: --psd: the prefix is too long\n");
    /* (statistics merge exactly: independent shards are fine; the seamless modes run passes this option has no place in yet) */
    if (o->stats_prefix && (o->mode != M_INDEPENDENT || o->iq_calibrate))
        REFUSE(2, "usage: --stats is for plain runs and independent --shards: it excludes every --seamless* mode and --iq-calibrate\n");
    if (o->stats_prefix && strlen(o->stats_prefix) > 3000) REFUSE(2, "usage: --stats: the prefix is too long\n");
    if (o->sgram_prefix && (o->have_shards || o->mode != M_INDEPENDENT || o->iq_calibrate))
        REFUSE(2, "usage: --sgram is for plain single-stream runs: it excludes --shards, every --seamless* mode and --iq-calibrate\n");
    if (o->sgram_prefix && strlen(o->sgram_prefix) > 3000) REFUSE(2, "usage: --sgram: the prefix is too long\n");
    if (o->lag_prefix && (o->have_shards || o->mode != M_INDEPENDENT || o->iq_calibrate))
        REFUSE(2, "usage: --lag is for plain single-stream runs: it excludes --shards, every --seamless* mode and --iq-calibrate\n");
    if (o->lag_prefix && strlen(o->lag_prefix) > 3000) REFUSE(2, "usage: --lag: the prefix is too long\n");
    if (o->lag_block && (!o->lag_prefix || o->lag_block == ~0u)) REFUSE(2, "usage: --lag-block B goes with --lag PREFIX, B a power of two in 64 .. 16777216\n");
    {
        iqgpu_lag_opts lo;
        if ((o->lag_list && !o->lag_prefix) || lag_opts_of(o, &lo))
            REFUSE(2, "usage: --lag-list d1,d2,.. goes with --lag PREFIX: one to four lags, strictly increasing, each 1 .. 65536\n");
    }
    if (o->match_prefix && (o->have_shards || o->mode != M_INDEPENDENT || o->iq_calibrate))
        REFUSE(2, "usage: --match is for plain single-stream runs: it excludes --shards, every --seamless* mode and --iq-calibrate\n");
    if (o->match_prefix && strlen(o->match_prefix) > 3000) REFUSE(2, "usage: --match: the prefix is too long\n");
    if (!o->match_prefix != !o->match_template) REFUSE(2, "usage: --match PREFIX and --match-template FILE.cf32 go together\n");
    if (o->match_block && (!o->match_prefix || o->match_block == ~0u)) REFUSE(2, "usage: --match-block B goes with --match PREFIX, B a power of two in 512 .. 16777216\n");
    {
        double hz[8];
        uint32_t nhz;
        if ((o->match_shifts && !o->match_prefix) || match_shifts_of(o, hz, &nhz))
            REFUSE(2, "usage: --match-shifts hz1,hz2,.. goes with --match PREFIX: one to eight offsets in Hz\n");
    }
    if (o->match_prefix) {
        /* the template and the options are checked before anything is written: the file, then the library's own rules (B against nfft) */
        char why[512];
        uint32_t L = 0;
        uint64_t rows;
        iqgpu_match_opts mo;
        float *t = match_template_of(o->match_template, &L, why, sizeof(why));
        if (!t) REFUSE(2, "usage: %s\n", why);
        free(t);
        iqgpu_match_opts_init(&mo);
        if (o->match_block) mo.block_frames = o->match_block;
        mo.template_frames = L;
        if (iqgpu_match_rows(&mo, 0, &rows) != IQGPU_OK) REFUSE(2, "usage: --match-block: %s\n", iqgpu_last_error());
    }
    if (o->env_prefix && (o->have_shards || o->mode != M_INDEPENDENT || o->iq_calibrate))
        REFUSE(2, "usage: --envelope is for plain single-stream runs: it excludes --shards, every --seamless* mode and --iq-calibrate\n");
    if (o->env_prefix && strlen(o->env_prefix) > 3000) REFUSE(2, "usage: --envelope: the prefix is too long\n");
    if (o->env_block && (!o->env_prefix || o->env_block == ~0u)) REFUSE(2, "usage: --envelope-block B goes with --envelope PREFIX, B a power of two in 64 .. 16777216\n");
    if (o->sgram_row_segments && (!o->sgram_prefix || o->sgram_row_segments == ~0u)) REFUSE(2, "usage: --sgram-row-segments R goes with --sgram PREFIX, R in 1 .. 1048576\n");
    for (const unsigned char *c = m->checks; *c != C_END; c++) switch (*c) {
    case C_SHARDS: if (!o->have_shards) REFUSE(2, "%s needs --shards N\n", m->flag); break;
    case C_HAS_AGC: if (o->desc.agc_enable) REFUSE(1, "%s: a chain with the output AGC is not covered (its measure route may cut a call into other segments "
        "than its process route)%s\n", m->flag, o->desc.agc_profile == IQGPU_AGC_DIGITAL ? "; --seamless-agc shards it to the DC bound" : ""); break;
    case C_NO_AGC: if (!o->desc.agc_enable) REFUSE(1, "%s: the chain has no output AGC (use %s)\n", m->flag, m->sans_agc); break;
    case C_NO_DC: if (!o->desc.dc_block_enable) REFUSE(1, "%s: the chain has no DC blocker: give --dc-block, or use %s\n", m->flag, m->sans_dc); break;
    case C_DIGITAL: if (o->desc.agc_profile == IQGPU_AGC_DIGITAL) REFUSE(1, "%s: the digital AGC profile works chunk by chunk; this mode is for the profiles "
        "dx / local (use --seamless-dc-agc)\n", m->flag); break;
    case C_PROFILE: if (o->desc.agc_profile != IQGPU_AGC_DIGITAL) REFUSE(1, "%s: the AGC profiles dx / local carry a per-sample loop state that no table of "
        "per-chunk figures reproduces exactly; only the digital profile is sharded seamlessly\n", m->flag); break;
    /* (the passes have to read the SAME stream: the constant filling of a bare --synthetic is no stream, its buffers differ) */
    case C_TWICE: if (o->synthetic_frames > 0 && !o->have_hash) REFUSE(2, "%s needs a stream it can read twice: an input file, or --synthetic with "
        "--synthetic-hash\n", m->flag); break;
    case C_CHUNK0: if (o->chunk_frames == 0) REFUSE(2, "%s: --chunk-frames 0\n", m->flag); break;
    case C_CHUNK_AGC: if (o->chunk_frames == 0 || o->chunk_frames % agc_chunk) REFUSE(2, "%s: --chunk-frames has to be a multiple of the AGC chunk (%zu frames)\n",
        m->flag, agc_chunk); break;
    }
    return 0;
}

/* --iq-calibrate: before any shard starts, ONE chain calibrates on the head of the input -- the blocks iqgpu_chain_calibrate_iq picks from
 * its first 2^24 frames (blocks are independent of what lies between them, so only they are read) -- and the result goes into the
 * description every shard is created from, as --iq-factors would have put it there.  0, or the exit status */
static int calibrate_head(Options *o, long long total_frames, size_t ibps)
{
    iqgpu_iq_calib_opts co;
    iqgpu_iq_calib_opts_init(&co);
    const long long head = total_frames < (1ll << 24) ? total_frames : (1ll << 24);
    if (head < 1024) REFUSE(1, "--iq-calibrate: the input has fewer than 1024 frames\n");
    const long long n = head / 1024 < (long long)co.max_blocks ? head / 1024 : (long long)co.max_blocks;
    const long long stride = head / n > 1024 ? head / n : 1024;
    char err[256] = "";
    int in_fd = -1, rc = 0;
    if (o->in_path && o->synthetic_frames <= 0 && (in_fd = open(o->in_path, O_RDONLY)) < 0) REFUSE(1, "open %s: %s\n", o->in_path, strerror(errno));
    void *buf = malloc((size_t)n * 1024 * ibps);
    iqgpu_chain *c = NULL;
    iqgpu_iq_calib_report r;
    if (!buf) { fprintf(stderr, "--iq-calibrate: out of memory\n"); rc = 1; }
    for (long long b = 0; !rc && b < n; b++)
        if (read_frames(o, in_fd, o->desc.in_format, ibps, b * stride, 1024, (char *)buf + (size_t)b * 1024 * ibps, err, sizeof(err))) { fprintf(stderr, "--iq-calibrate: %s\n", err); rc = 1; }
    if (!rc) {
        iqgpu_chain_desc d = o->desc;
        d.device_ordinal = o->device0;
        co.max_blocks = (uint32_t)n;
        if (iqgpu_chain_create(&d, &c) != IQGPU_OK || iqgpu_chain_calibrate_iq(c, buf, (size_t)n * 1024, &co, &r) != IQGPU_OK) { fprintf(stderr, "--iq-calibrate: %s\n", iqgpu_last_error()); rc = 1; }
    }
    if (c) iqgpu_chain_destroy(c);
    free(buf);
    if (in_fd >= 0) close(in_fd);
    if (rc) return rc;
    o->desc.iq_correct_enable = 1; o->desc.iq_mag = r.mag; o->desc.iq_phase = r.phase;
    printf("iq_calibrate: --iq-factors %.9g:%.9g found=%d blocks=%u/%u levels=%u total=%.9g->%.9g\n", r.mag, r.phase, r.found, r.blocks_used, r.blocks_taken,
           r.n_levels, r.total_at_center0, r.total_at_best);
    fflush(stdout);
    if (!r.found) fprintf(stderr, "--iq-calibrate: no block of the head has %g dB of peak-to-average power: the factors stay %g:%g (no correction measured)\n",
                          (double)co.power_threshold_db, (double)r.mag, (double)r.phase);
    return 0;
}

static iqgpu_chain_desc desc_without(const iqgpu_chain_desc *d, int off)
{
    iqgpu_chain_desc r = *d;
    if (off & F_DC) r.dc_block_enable = 0;
    if (off & F_AGC) r.agc_enable = 0;
    return r;
}

/* The shard plan; 0, or the exit status.  Equal frame ranges, the last takes the rest.  Independent shards: every output behind the one
 * in front, counted by the closed form of a fresh chain.  Seamless modes: ONE stream, cut at multiples of the mode's grid; preroll, place
 * and count from the stream's closed forms, with the stages off that the mode's row names (none of the three depends on a stage whose
 * state the recipe carries, iqgpu.h) */
static int plan_shards(const Options *o, Shard *sh, long long total_frames, size_t obps)
{
    const ModeRow *m = &MODES[o->mode];
    const int seamless = o->mode != M_INDEPENDENT;
    const long long per = total_frames / o->shards, cf = (long long)o->chunk_frames, agc_chunk = (long long)agc_chunk_of(&o->desc);
    const iqgpu_chain_desc d_pre = desc_without(&o->desc, m->preroll_off), d_place = desc_without(&o->desc, m->place_off);
    uint64_t memory = 0;
    /* (a chain the seek refuses is refused here, in the library's words) */
    if (seamless && m->preroll_fn(&d_pre, &memory) != IQGPU_OK) REFUSE(1, "%s: %s\n", m->flag, iqgpu_last_error());
    const long long preroll = m->whole_calls ? ((long long)memory + cf - 1) / cf * cf : (long long)memory;
    long long grid = seamless ? 4096 : 1, off = 0;
    if (m->grid_agc) grid = lcm(grid, agc_chunk);
    if (m->grid_chunk) grid = lcm(grid, cf);
    for (int s = 0; s < o->shards; s++) {
        const long long next = (s == o->shards - 1) ? total_frames : ((long long)(s + 1) * per) / grid * grid;
        uint64_t first_out = 0, nout = 0;
        size_t fresh_out = 0;
        sh[s].opt = o; sh[s].shard = s;
        sh[s].first_frame = ((long long)s * per) / grid * grid;
        sh[s].frames = next - sh[s].first_frame;
        if (sh[s].frames <= 0 && m->grid_words) REFUSE(1, "%s: %lld frames are too few for %d shards on a grid of %lld frames%s: shard %d would be empty\n", m->flag,
            total_frames, o->shards, grid, m->grid_words, s);
        if (!seamless) {
            /* (decimating or interpolating resampler, FFT-block quantisation in front of or behind it) */
            if (iqgpu_design_out_frames(&o->desc, (size_t)sh[s].frames, &fresh_out) != IQGPU_OK) REFUSE(1, "%s\n", iqgpu_last_error());
            sh[s].out_offset_bytes = off;
            sh[s].planned_out = (long long)fresh_out;
            off += (long long)fresh_out * (long long)obps;
            continue;
        }
        sh[s].preroll_frames = sh[s].first_frame < preroll ? sh[s].first_frame : preroll;
        if (iqgpu_design_out_frames_range(&d_place, (uint64_t)sh[s].first_frame, (uint64_t)sh[s].frames, &first_out, &nout) != IQGPU_OK) REFUSE(1, "%s\n", iqgpu_last_error());
        sh[s].out_offset_bytes = (long long)first_out * (long long)obps;
        sh[s].planned_out = (long long)nout;
        if (o->dry && m->dry_rows && s < o->shards - 1) {
            /* what the measuring passes will record: one DC row per call (at least: a call the AGC's lock cuts gives two), one AGC row per
             * AGC chunk of every call */
            const long long full = sh[s].frames / cf, rest = sh[s].frames % cf;
            if (m->dry_rows & F_DC) sh[s].n_dc_rows = (sh[s].frames + cf - 1) / cf;
            if (m->dry_rows & F_AGC) sh[s].agc_rows = full * ((cf + agc_chunk - 1) / agc_chunk) + (rest + agc_chunk - 1) / agc_chunk;
        }
    }
    return 0;
}

/* --seamless-rms, --seamless-dc-rms: the seam certificate (iqgpu.h), in order.  Shard s started from the state shard s-1 ended in, bit for bit: its
 * bytes are the single stream's, given that shard s-1's are.  Otherwise its range again from shard s-1's checkpoint, in a thread
 * of its own like the first time, and the seam behind it is checked against the new end state.  seams: certified, ranges redone */
static int certify_seams(const Options *o, Shard *sh, pthread_t *th, long long *frames_out, int seams[2])
{
    int rc = 0;
    for (int s = 1; s < o->shards && rc == 0; s++) {
        const iqgpu_agc_state *e = &sh[s - 1].rms_end_state, *b = &sh[s].rms_seek_state;
        if (!memcmp(&e->current_gain, &b->current_gain, sizeof(float)) && !memcmp(&e->peak_memory, &b->peak_memory, sizeof(float)) &&
            e->samples_seen == b->samples_seen) { sh[s].certified = 1; seams[0]++; continue; }
        sh[s].redo_blob = sh[s - 1].blob; sh[s].redo_bytes = sh[s - 1].blob_bytes; sh[s].redone = 1; seams[1]++;
        *frames_out -= sh[s].frames_out;
        sh[s].rc = 0; sh[s].err[0] = 0;
        pthread_create(&th[s], NULL, run_shard, &sh[s]);
        pthread_join(th[s], NULL);
        if (sh[s].rc) { fprintf(stderr, "shard %d failed when its range was redone: %s\n", s, sh[s].err); rc = 1; }
        *frames_out += sh[s].frames_out;
    }
    return rc;
}

/* what the job's mode adds to the report: in front of the keys of the top-level object (sh NULL; seams: as above), behind those of a shard */
static void mode_keys(char *kv, size_t cap, const Options *o, const Shard *sh, const int seams[2])
{
    const ModeRow *m = &MODES[o->mode];
    kv[0] = 0;
    if (o->mode == M_INDEPENDENT) return;
    if (!sh) {
        const int n = snprintf(kv, cap, "\"%s\": true, ", m->json_key);
        if (m->certify && !o->dry) snprintf(kv + n, cap - (size_t)n, "\"seams\": %d, \"seams_certified\": %d, \"ranges_redone\": %d, ", o->shards - 1, seams[0], seams[1]);
        return;
    }
    int n = snprintf(kv, cap, ", \"preroll_frames\": %lld", sh->preroll_frames);
    if (o->dry) {
        if (m->dry_rows & F_DC) n += snprintf(kv + n, cap - (size_t)n, ", \"dc_rows\": %lld", sh->n_dc_rows);
        if (m->dry_rows & F_AGC) snprintf(kv + n, cap - (size_t)n, ", \"agc_rows\": %lld", sh->agc_rows);
        return;
    }
    kv += n; cap -= (size_t)n;
    switch (o->mode) {
    case M_RMS:
        snprintf(kv, cap, ", \"certified\": %s, \"redone\": %s, \"end\": {\"peak_memory\": %.9g, \"current_gain\": %.9g, \"samples_seen\": %llu}",
                 sh->certified ? "true" : "false", sh->redone ? "true" : "false", (double)sh->rms_end_state.peak_memory, (double)sh->rms_end_state.current_gain,
                 (unsigned long long)sh->rms_end_state.samples_seen);
        break;
    case M_DC_RMS:
        snprintf(kv, cap, ", \"measure_seconds\": %.6f, \"dc_rows\": %lld, \"dc_entry\": {\"re\": %.17g, \"im\": %.17g}, \"certified\": %s, \"redone\": %s, "
                 "\"end\": {\"peak_memory\": %.9g, \"current_gain\": %.9g, \"samples_seen\": %llu}", sh->measure_seconds, sh->n_dc_rows, sh->dc_entry.re, sh->dc_entry.im,
                 sh->certified ? "true" : "false", sh->redone ? "true" : "false", (double)sh->rms_end_state.peak_memory, (double)sh->rms_end_state.current_gain,
                 (unsigned long long)sh->rms_end_state.samples_seen);
        break;
    case M_AGC:
        snprintf(kv, cap, ", \"measure_seconds\": %.6f, \"agc_rows\": %lld, \"entry\": {\"locked\": %d, \"peak_memory\": %.9g, \"current_gain\": %.9g, "
                 "\"last_strong_peak_time\": %.17g, \"samples_seen\": %llu}", sh->measure_seconds, sh->agc_rows, sh->entry.locked, (double)sh->entry.peak_memory,
                 (double)sh->entry.current_gain, sh->entry.last_strong_peak_time, (unsigned long long)sh->entry.samples_seen);
        break;
    case M_DC:
        snprintf(kv, cap, ", \"measure_seconds\": %.6f, \"dc_rows\": %lld, \"entry\": {\"re\": %.17g, \"im\": %.17g}", sh->measure_seconds, sh->n_dc_rows,
                 sh->dc_entry.re, sh->dc_entry.im);
        break;
    case M_DC_AGC:
        snprintf(kv, cap, ", \"measure_seconds\": %.6f, \"dc_rows\": %lld, \"agc_rows\": %lld, \"dc_entry\": {\"re\": %.17g, \"im\": %.17g}, \"entry\": {\"locked\": %d, "
                 "\"current_gain\": %.9g, \"samples_seen\": %llu}", sh->measure_seconds, sh->n_dc_rows, sh->agc_rows, sh->dc_entry.re, sh->dc_entry.im, sh->entry.locked,
                 (double)sh->entry.current_gain, (unsigned long long)sh->entry.samples_seen);
        break;
    default:
        break;
    }
}

/* one JSON line: the placement as planned (`distinct_devices` is what an N-shard job on N GPUs must show), or the run */
static void report(const Options *o, const Shard *sh, long long total_frames, long long frames_out, double dt, double stream_s, const int seams[2])
{
    const size_t ibps = iqgpu_get_bytes_per_sample(o->desc.in_format), obps = iqgpu_get_bytes_per_sample(o->desc.out_format);
    char kv[512];
    mode_keys(kv, sizeof(kv), o, NULL, seams);
    if (o->dry) {
        int distinct = 0;
        for (int s = 0; s < o->shards; s++) { int seen = 0; for (int q = 0; q < s; q++) if (!strcmp(sh[q].bus_id, sh[s].bus_id) && sh[q].device == sh[s].device) seen = 1; if (!seen) distinct++; }
        printf("{\"dry_placement\": true, %s\"frames_in\": %lld, \"frames_out\": %lld, \"shards\": %d, \"devices\": %d, \"distinct_devices\": %d, \"per_shard\": [",
               kv, total_frames, frames_out, o->shards, o->devices, distinct);
    } else {
        printf("{%s\"frames_in\": %lld, \"frames_out\": %lld, \"shards\": %d, \"devices\": %d, \"seconds\": %.6f, \"msps_end_to_end\": %.3f, \"stream_seconds\": %.6f, \"msps_streaming\": %.3f, "
               "\"h2d_GBs\": %.3f, \"d2h_GBs\": %.3f, \"in_bytes_per_frame\": %zu, \"out_bytes_per_frame\": %zu, \"input\": \"%s\", \"per_shard\": [",
               kv, total_frames, frames_out, o->shards, o->devices, dt, total_frames / dt / 1e6, stream_s, stream_s > 0 ? total_frames / stream_s / 1e6 : 0.0,
               stream_s > 0 ? (double)total_frames * (double)ibps / stream_s / 1e9 : 0.0, stream_s > 0 ? (double)frames_out * (double)obps / stream_s / 1e9 : 0.0, ibps, obps,
               o->synthetic_frames <= 0 ? "file" : o->have_hash ? "synthetic-hash" : "synthetic-constant");
    }
    for (int s = 0; s < o->shards; s++) {
        mode_keys(kv, sizeof(kv), o, &sh[s], seams);
        if (o->dry)
            printf("%s{\"shard\": %d, \"device\": %d, \"pci_bus_id\": \"%s\", \"numa_node\": %d, \"cpus_allowed\": %d, \"first_frame\": %lld, \"frames_in\": %lld, \"planned_out\": %lld, "
                   "\"out_offset_bytes\": %lld, \"pinned_bytes\": %lld, \"hbm_bytes\": %lld%s}", s ? ", " : "", s, sh[s].device, sh[s].bus_id, sh[s].numa_node, sh[s].cpus_allowed,
                   sh[s].first_frame, sh[s].frames, sh[s].planned_out, sh[s].out_offset_bytes, sh[s].pinned_bytes, sh[s].hbm_bytes, kv);
        else
            printf("%s{\"shard\": %d, \"device\": %d, \"numa_node\": %d, \"first_frame\": %lld, \"frames_in\": %lld, \"frames_out\": %lld, \"planned_out\": %lld, \"out_offset_bytes\": %lld, \"seconds\": %.6f%s}",
                   s ? ", " : "", s, sh[s].device, sh[s].numa_node, sh[s].first_frame, sh[s].frames, sh[s].frames_out, sh[s].planned_out, sh[s].out_offset_bytes, sh[s].stream_seconds, kv);
    }
    printf("]}\n");
}

int main(int argc, char **argv)
{
    Options o;
    int rc = parse_args(argc, argv, &o);
    if (!rc) rc = validate(&o);
    if (rc) return rc;

    const size_t ibps = iqgpu_get_bytes_per_sample(o.desc.in_format), obps = iqgpu_get_bytes_per_sample(o.desc.out_format);
    long long total_frames = o.synthetic_frames;
    if (total_frames <= 0) {
        struct stat st;
        if (stat(o.in_path, &st) != 0) REFUSE(1, "stat %s: %s\n", o.in_path, strerror(errno));
        total_frames = (long long)(st.st_size / (off_t)ibps);
    }
    Shard *sh = (Shard *)calloc((size_t)o.shards, sizeof(Shard));
    iqgpu_chain_info info;
    if (iqgpu_design_probe(&o.desc, &info, NULL, 0, NULL, 0, NULL, 0) != IQGPU_OK) REFUSE(1, "%s\n", iqgpu_last_error());
    if (o.iq_calibrate && !o.dry && (rc = calibrate_head(&o, total_frames, ibps)) != 0) { free(sh); return rc; }
    rc = plan_shards(&o, sh, total_frames, obps);
    if (rc) return rc;
    g_shards = sh;
    if (MODES[o.mode].barriers && !o.dry && pthread_barrier_init(&g_pass, NULL, (unsigned)o.shards) != 0) REFUSE(1, "pthread_barrier_init failed\n");
    if (o.out_path && !o.dry) { int fd = open(o.out_path, O_WRONLY | O_CREAT | O_TRUNC, 0644); if (fd >= 0) close(fd); }

    const double t0 = now_s();
    pthread_t *th = (pthread_t *)calloc((size_t)o.shards, sizeof(pthread_t));
    for (int s = 0; s < o.shards; s++) pthread_create(&th[s], NULL, run_shard, &sh[s]);
    long long frames_out = 0;
    double stream_s = 0;
    for (int s = 0; s < o.shards; s++) {
        pthread_join(th[s], NULL);
        if (sh[s].rc) { fprintf(stderr, "shard %d failed: %s\n", s, sh[s].err); rc = 1; }
        frames_out += sh[s].frames_out;
        if (sh[s].stream_seconds > stream_s) stream_s = sh[s].stream_seconds;
    }
    int seams[2] = {0, 0};
    if (MODES[o.mode].certify && !o.dry && rc == 0) rc = certify_seams(&o, sh, th, &frames_out, seams);
    if (o.stats_prefix && !o.dry && rc == 0) rc = write_stats(&o, sh);
    if (o.dry || !o.quiet) report(&o, sh, total_frames, frames_out, now_s() - t0, stream_s, seams);
    for (int s = 0; s < o.shards; s++) if (sh[s].rows) iqgpu_host_free_pinned(sh[s].rows);
    for (int s = 0; s < o.shards; s++) { free(sh[s].dc_rows); free(sh[s].dc_call_rows); free(sh[s].blob); }
    free(th); free(sh);
    return rc;
}
