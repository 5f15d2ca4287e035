/*
 * iqgpu.h -- C ABI of libiqgpu: the MI355X (gfx950) replacement for iq_tool's
 * pre_processor -> resampler -> post_processor sample path.
 *
 * One `iqgpu_chain` handle stands in for the three DSP stage threads of the reference
 * (/root/reference/src/pipeline.c:436-595) for ONE stream.  It is what a single "GPU stage"
 * thread sitting between reader_output_queue and the writer would call; see INTEGRATION.md for
 * the binding a maintainer adds on the reference side.
 *
 * Conventions (they mirror the reference's, src/pipeline.c / include/resampler.h):
 *   - the caller owns every host buffer; handles are opaque; one thread per handle; handles are
 *     independent (one per GPU shard);
 *   - the stream is continuous across calls: any split of the input into calls produces the
 *     same output bytes (all in-scope operators are chunk-size invariant).  The
 *     one exception is the reference's own: the "digital" output AGC works chunk by chunk, so with
 *     that profile every call is cut into agc_chunk_frames-sized chunks from its first frame
 *     (the "dx" / "local" profiles are per-sample loops: any split gives the same bytes);
 *   - nothing is flushed at end of stream (resampler / FIR tails and the FFT-filter remainder
 *     are dropped exactly as the reference drops them, src/filter.c:521-525);
 *   - frames_out may be 0 (resampler group buffering, FFT block quantisation);
 *   - every entry point returns 0 on success or a negative IQGPU_E* code, with a message
 *     available from iqgpu_last_error().  There is no CPU fallback: without a usable HIP
 *     device every compute entry point fails with IQGPU_ENODEV.
 */
#ifndef IQGPU_H_
#define IQGPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IQGPU_ABI_VERSION 9

/* Sample formats: numerically equal to the reference's format_t (include/common_types.h:33-37) */
enum {
    IQGPU_FMT_CU8 = 8, IQGPU_FMT_CS8 = 9, IQGPU_FMT_CU16 = 10, IQGPU_FMT_CS16 = 11,
    IQGPU_FMT_CS24 = 12, IQGPU_FMT_CU32 = 13, IQGPU_FMT_CS32 = 14, IQGPU_FMT_CF32 = 15,
    IQGPU_FMT_SC16Q11 = 16
};
/* == FilterType (include/common_types.h:45-51) */
enum { IQGPU_FILTER_NONE = 0, IQGPU_FILTER_LOWPASS = 1, IQGPU_FILTER_HIGHPASS = 2,
       IQGPU_FILTER_PASSBAND = 3, IQGPU_FILTER_STOPBAND = 4 };
/* == FilterTypeRequest (include/common_types.h:61-65) */
enum { IQGPU_FILTER_IMPL_AUTO = 0, IQGPU_FILTER_IMPL_FIR = 1, IQGPU_FILTER_IMPL_FFT = 2 };
/* == FilterImplementationType (include/common_types.h:53-59) */
enum { IQGPU_FI_NONE = 0, IQGPU_FI_FIR_SYMMETRIC = 1, IQGPU_FI_FIR_ASYMMETRIC = 2,
       IQGPU_FI_FFT_SYMMETRIC = 3, IQGPU_FI_FFT_ASYMMETRIC = 4 };

enum {
    IQGPU_OK = 0,
    IQGPU_EINVAL = -1,      /* bad argument / NULL handle */
    IQGPU_ENODEV = -2,      /* no HIP device, or device_ordinal out of range */
    IQGPU_ENOMEM = -3,      /* device or host allocation failed */
    IQGPU_ERATIO = -4,      /* ratio not finite or outside [1e-3, 1e3]   (src/setup.c:109-112) */
    IQGPU_EFORMAT = -5,     /* unhandled sample format                    (src/sample_convert.c:203-206) */
    IQGPU_ESHIFT = -6,      /* shift beyond 5x rate, or shift_after_resample without a shift (src/frequency_shift.c:36-49) */
    IQGPU_EFILTER = -7,     /* filter band beyond output Nyquist, fft size too small, too many stages (src/filter.c:80-84, 321-325) */
    IQGPU_ECAPACITY = -8,   /* out_capacity_bytes too small for this call */
    IQGPU_EHIP = -9,        /* a HIP runtime call failed */
    IQGPU_EUNSUPPORTED = -10/* the placement calls: a *_VISIBLE_DEVICES list that is not plain indices                */
                            /* iqgpu_chain_seek and the two range-design calls: a chain with the output AGC              */
                            /* the AGC two-pass calls (measure*, agc_advance, seek_agc*): profile dx / local, CLOCK_WALL */
                            /* iqgpu_chain_save_state: a chain on IQGPU_AGC_CLOCK_WALL                                   */
                            /* iqgpu_chain_seek_rms* / iqgpu_design_preroll_frames_rms: profile digital, the DC blocker  */
};

typedef struct iqgpu_chain iqgpu_chain; /* opaque, like resampler_t (include/resampler.h:25-26) */

typedef struct { int type; float f1_hz, f2_hz; } iqgpu_filter_req; /* == FilterRequest: f1 = cutoff or centre, f2 = bandwidth */

/* Mirrors the AppConfig / AppResources fields the path reads (include/app_context.h:66-138). */
typedef struct {
    int    in_format, out_format;       /* IQGPU_FMT_*                                                      */
    double input_rate_hz;               /* source_info.samplerate                                           */
    double target_rate_hz;              /* config->target_rate; r = (float)(target/input)  src/setup.c:107  */
    float  resample_ratio;              /* if > 0: use this float ratio as-is (create_resampler's argument,  */
                                        /*   src/resampler.c:20) instead of deriving it from the rates      */
    float  gain;                        /* config->gain, applied at unpack (src/pre_processor.c:21-22)      */
    double shift_hz;                    /* resources->nco_shift_hz (sign selects mix up / down)             */
    int    shift_after_resample;        /* config->shift_after_resample                                     */
    int    dc_block_enable;             /* config->dc_block.enable                                          */
    int    iq_correct_enable;           /* config->iq_correction.enable                                     */
    float  iq_mag, iq_phase;            /* initial correction factors (reference starts at 0,0)             */
    int    no_resample;                 /* config->no_resample                                              */
    int    n_filters;                   /* config->num_filter_requests (<= 5)                               */
    iqgpu_filter_req filters[5];        /* config->filter_requests                                          */
    float  transition_width_hz;         /* config->transition_width_hz_arg (0 = auto)                       */
    float  attenuation_db;              /* config->attenuation_db_arg (0 = 60 dB)                           */
    int    filter_taps;                 /* config->filter_taps_arg AFTER the odd bump of src/config.c:233-236 (0 = auto) */
    int    filter_impl;                 /* IQGPU_FILTER_IMPL_*  (config->filter_type_request)               */
    int    fft_size;                    /* config->filter_fft_size_arg (0 = auto)                           */
    /* GPU-only knobs */
    int    device_ordinal;              /* HIP device index                                                 */
    size_t block_samples;               /* input samples per workgroup block, multiple of 2048; 0 = auto (one run per resident wave) */
    /* output AGC, between the post NCO and the pack (src/post_processor.c:55-57, src/agc.c) */
    int    agc_enable;                  /* config->output_agc.enable                                        */
    int    agc_profile;                 /* IQGPU_AGC_*  (config->output_agc.profile): DIGITAL, or liquid's agc_crcf as DX / LOCAL */
    float  agc_target;                  /* config->output_agc.target_level_arg (0 = AGC_DIGITAL_PEAK_TARGET) */
    int    agc_clock;                   /* IQGPU_AGC_CLOCK_*: what stands in for get_monotonic_time_sec()    */
    uint32_t agc_chunk_frames;          /* input frames per reference chunk, 0 = 16384 (PIPELINE_CHUNK_BASE_SAMPLES): */
                                        /*   every process() call is cut into chunks of this many input frames, */
                                        /*   counted from the start of the call, and agc_apply sees one chunk at a time */
} iqgpu_chain_desc;

/* AgcProfile, include/common_types.h:77-82 */
enum { IQGPU_AGC_OFF = 0, IQGPU_AGC_DX = 1, IQGPU_AGC_LOCAL = 2, IQGPU_AGC_DIGITAL = 3 };
/* SAMPLES: time of the output stream (samples_seen / target_rate) -- deterministic, and equal to the
 * wall clock when the reference runs in real time.  WALL: CLOCK_MONOTONIC read once per process() call. */
enum { IQGPU_AGC_CLOCK_SAMPLES = 0, IQGPU_AGC_CLOCK_WALL = 1 };

/* AppResources' AGC fields (include/app_context.h:227-231) */
typedef struct {
    int      locked;
    float    peak_memory;               /* profiles dx / local: agc_crcf's y2_prime (smoothed output energy) */
    float    current_gain;              /* profiles dx / local: agc_crcf's gain                              */
    int      reserved;
    double   last_strong_peak_time;
    uint64_t samples_seen;
} iqgpu_agc_state;

/* What create() derived; for diagnostics and for parity tests of the design path. */
typedef struct {
    float    ratio;                     /* float32 resampling ratio                                         */
    int      interp;                    /* 1 if ratio > 1                                                   */
    int      num_halfband_stages;       /* S                                                                */
    int      stage_m[16];               /* half-band semi-lengths in run order (highest rate first)         */
    float    rate_arb;                  /* arbitrary-resampler rate                                         */
    uint32_t arb_step;                  /* 24-bit fixed-point phase step                                    */
    uint32_t nco_dtheta;                /* uint32 NCO phase increment                                       */
    float    dc_alpha;                  /* float32 alpha of the DC blocker                                  */
    int      filter_post_resample;      /* apply_user_filter_post_resample                                  */
    int      filter_impl;               /* IQGPU_FI_*                                                       */
    uint32_t filter_ntaps;
    uint32_t filter_block;              /* fftfilt block size (0 for FIR)                                   */
    uint32_t history_samples;           /* processed input samples kept between calls                       */
} iqgpu_chain_info;

/* Per-kernel device time accumulated by HIP events on the chain's stream (profiling mode only). */
enum { IQGPU_K_DC_PREFIX = 0, IQGPU_K_DC_SCAN = 1, IQGPU_K_FRONT = 2, IQGPU_K_FILTER = 3, IQGPU_K_MOVE = 4, IQGPU_K_AGC = 5,
    IQGPU_K_CASCADE = 6, IQGPU_K_COUNT = 8 };
typedef struct {
    uint64_t launches[IQGPU_K_COUNT];
    double   ms[IQGPU_K_COUNT];
} iqgpu_profile;

/* ---- library ---- */
int         iqgpu_abi_version(void);
const char *iqgpu_last_error(void);              /* thread-local message of the last failure        */
int         iqgpu_device_count(void);            /* number of HIP devices, 0 if none / no runtime   */
/* PCI bus id ("0000:05:00.0") of device `ordinal` (hipDeviceGetPCIBusId): what a multi-GPU launcher logs to show that its
 * ranks sit on distinct devices (bench.py `config.devices`; the reference has no counterpart: it runs on the host) */
int         iqgpu_device_pci_bus_id(int ordinal, char *buf, size_t cap);
/* NUMA placement of whoever feeds a GPU (ABI v5).  No counterpart in the reference: it is one host process whose stage threads
 * stay on the CPU (src/pipeline.c:96-116); here every bench rank / harness shard thread streams through pinned buffers into ONE
 * device and should sit on that device's socket.  Both read sysfs only (KFD topology -> PCI address -> numa_node /
 * local_cpulist) and make NO HIP call, so they can -- and should -- run before the first GPU call of the process or thread and
 * before its pinned buffers are allocated.  *node = -1 when the host does not say (single node, VM); IQGPU_EUNSUPPORTED when a
 * *_VISIBLE_DEVICES variable holds something other than indices (the device order is then not derived and nothing is bound).
 * iqgpu_bind_thread_to_device: sched_setaffinity of the CALLING THREAD to the node's CPUs (intersected with its current mask)
 * and a preferred-node memory policy for it; threads created afterwards inherit both. */
int         iqgpu_device_numa_node(int ordinal, int *node, char *pci_bus_id, size_t cap);
int         iqgpu_bind_thread_to_device(int ordinal, int *node);

/* ---- chain lifecycle: replaces _create_dsp_components/_destroy_dsp_components (src/pipeline.c:138-157) ---- */
void   iqgpu_chain_desc_init(iqgpu_chain_desc *d);                 /* reference defaults: gain 1, cs16->cs16, no ops */
int    iqgpu_chain_create(const iqgpu_chain_desc *d, iqgpu_chain **out);
void   iqgpu_chain_destroy(iqgpu_chain *c);
int    iqgpu_chain_get_info(const iqgpu_chain *c, iqgpu_chain_info *info);
/* copies min(cap, ntaps) complex taps (re,im interleaved) of the combined user filter; returns ntaps */
int    iqgpu_chain_get_filter_taps(const iqgpu_chain *c, float *re_im, size_t cap_taps);
/* The create-time design path alone (ratio, half-band plan, NCO increment, filter placement and
 * taps) without touching a device: same validation and error codes as iqgpu_chain_create.
 * filter_taps_re_im / hb_taps / arb_proto may be NULL.  hb_taps receives the 4m+1 prototype of
 * every half-band stage back to back in run order; arb_proto the 3584 scaled polyphase taps. */
int    iqgpu_design_probe(const iqgpu_chain_desc *d, iqgpu_chain_info *info,
                          float *filter_taps_re_im, size_t cap_taps,
                          float *hb_taps, size_t cap_hb, float *arb_proto, size_t cap_arb);

/* frames a FRESH chain of this description emits for a stream of frames_in frames (no device needed): the
 * closed form of the resampler law and the FFT-block quantisation on whichever side of the resampler the filter
 * sits.  What a stitching writer uses to place the outputs of independent shards (8 iq_tool runs + cat); for shards that
 * continue ONE stream see iqgpu_design_out_frames_range below. */
int    iqgpu_design_out_frames(const iqgpu_chain_desc *d, size_t frames_in, size_t *frames_out);

/* ---- seamless range sharding (ABI v7): start a chain at any position of ONE stream ----
 * Everything a chain carries from call to call is either a closed form of the number of input frames consumed (open decimation
 * group, resampler phase, both NCO phases, pending FFT-block samples) or finite FIR memory (half-band, polyphase, user-filter
 * and overlap-save histories).  iqgpu_chain_seek sets the first from the position and refills the second by running the frames
 * in front of the position through the ordinary kernels with the output dropped.  N chains that each seek to the start of their
 * range and process it then write, stitched in order, the stream ONE chain writes: byte for byte on every chain without a DC
 * blocker.  The DC blocker is a decaying IIR: its state is warmed up over ceil(ln(1e6) / alpha) extra frames.  A state error e
 * decays as (1 - alpha)^n and reaches the output as alpha * e, and |state| <= max|x| / alpha, so behind that warm-up the output
 * differs from the single stream's by at most 1e-6 of full scale (a tenth of the 1e-5 parity bar) and less with every frame;
 * a seek whose warm-up starts at frame 0 is exact.  The output AGC is a function of the whole prefix of the stream (scan / lock /
 * creep of the digital profile, agc_crcf's loop of dx / local): no warm-up bounds it, and these calls refuse such chains with
 * IQGPU_EUNSUPPORTED.  Positions are 64-bit; first_frame + frames_in beyond 2^39 frames is IQGPU_EINVAL (the 24-bit fixed-point
 * phase arithmetic holds that far and is never allowed to wrap).
 *
 * iqgpu_design_preroll_frames: input frames in front of a seam that a chain of this description has to see (output discarded)
 * so that everything it emits afterwards is what the single stream emits: its FIR memory expressed in input frames (plus the DC
 * warm-up).  0 for a pointwise chain.  No device; same validation and error codes as iqgpu_chain_create.
 * iqgpu_design_out_frames_range: what ONE stream of this description emits while it consumes input frames
 * [first_frame, first_frame + frames_in): index of the first of those output frames in the stream's output, and how many.  For
 * any cut points the ranges tile the output: frames_out sums to iqgpu_design_out_frames of the whole.  No device. */
int    iqgpu_design_preroll_frames(const iqgpu_chain_desc *d, uint64_t *frames);
int    iqgpu_design_out_frames_range(const iqgpu_chain_desc *d, uint64_t first_frame, uint64_t frames_in,
                                     uint64_t *out_first, uint64_t *frames_out);

/* ---- per-chunk: replaces pre_processor_apply_chain (src/pre_processor.c:10), resampler_execute
 *      (include/resampler.h:48) and post_processor_apply_chain (src/post_processor.c:9) in one call ---- */
int    iqgpu_chain_process(iqgpu_chain *c, const void *raw_in, size_t frames_in,
                           void *out, size_t out_capacity_bytes, size_t *frames_out);
/* Same, with both buffers already in device memory (HBM) of the chain's device.  Asynchronous on the
 * chain's stream; *frames_out is exact on return (it is a closed form of the stream position). */
int    iqgpu_chain_process_device(iqgpu_chain *c, const void *d_raw_in, size_t frames_in,
                                  void *d_out, size_t out_capacity_bytes, size_t *frames_out);
/* Pipelined form of iqgpu_chain_process for a stage thread that must not stall on PCIe: submit() queues the
 * batch's H2D copy and returns with the batch's exact *frames_out (a closed form of the stream position behind
 * the batches already submitted) and a ticket; the batch's kernels and its D2H copy are queued by the submit()
 * calls that follow (three and five batches later) or by collect(), which blocks until the batch's output
 * bytes are in `out`.  Up to iqgpu_chain_pipeline_depth() batches may be in flight; copies of one batch
 * overlap the kernels of its neighbours.  The pipeline makes progress inside submit() / collect() only, and a
 * failure of a batch's kernels (IQGPU_EHIP ...) is reported by the call that launches them -- a later submit()
 * or the batch's collect() -- after which the handle is poisoned until iqgpu_chain_reset(), as with process().
 * The I/Q factors a batch runs with are those in force at its submit().  raw_in / out should be pinned (iqgpu_host_malloc_pinned) --
 * pageable memory works but serialises -- and must stay untouched until the ticket is collected.  Batches are
 * processed in submit order: the stream is continuous across them exactly as across iqgpu_chain_process calls
 * (this is what replaces the reference's chunk hand-off between its three stage threads, src/pipeline.c:436-595).
 * How long submit() may block: normally the ~10 us of queueing.  On a chain with the digital output AGC fused into its last kernel
 * (agc_enable, profile `digital`, past the lock) the launch of batch N first reads the AGC verdict of batch N-1 from a pinned word,
 * i.e. it waits until batch N-1's kernels have FINISHED (polled; after 0.25 s it falls back to a stream synchronise): submit() then
 * blocks for at most one batch's kernel time (0.02 - 1.3 ms at 2^18 - 2^28 frames).  Chains without that AGC never wait for device work
 * in submit(). */
int    iqgpu_chain_submit(iqgpu_chain *c, const void *raw_in, size_t frames_in,
                          void *out, size_t out_capacity_bytes, size_t *frames_out, uint64_t *ticket);
int    iqgpu_chain_collect(iqgpu_chain *c, uint64_t ticket);
int    iqgpu_chain_pipeline_depth(void);
/* == pre_processor_reset + resampler_reset + post_processor_reset (stream discontinuity) */
int    iqgpu_chain_reset(iqgpu_chain *c);
/* Puts the chain at stream frame first_frame.  preroll: the preroll_frames input frames that END at first_frame, in host memory
 * (_device: in device memory of the chain's device); preroll_frames <= first_frame, and at least
 * min(first_frame, iqgpu_design_preroll_frames) -- a shorter warm-up would be a silent seam and is IQGPU_EINVAL; longer is
 * allowed.  It does what iqgpu_chain_reset does (batches in flight and a pending AGC verdict are resolved first, histories and
 * the DC state are zeroed, a poisoned handle is cleared), drops pending FFT-block samples as well, sets the stream position to the
 * closed form at first_frame - preroll_frames and runs the preroll through the ordinary per-call path into a buffer the chain
 * owns.  Both variants return with the chain's stream idle.  Afterwards process / process_device / submit behave as if the chain
 * had consumed frames [0, first_frame) of the stream (to the DC bound above).  first_frame == 0 without a preroll leaves a fresh
 * chain.  When an argument is refused the chain is left reset (at frame 0).  IQGPU_EUNSUPPORTED for first_frame > 0 on a chain
 * with the output AGC. */
int    iqgpu_chain_seek(iqgpu_chain *c, uint64_t first_frame, const void *preroll, size_t preroll_frames);
int    iqgpu_chain_seek_device(iqgpu_chain *c, uint64_t first_frame, const void *d_preroll, size_t preroll_frames);
/* ---- seamless range sharding of chains with the DIGITAL output AGC (ABI v8): two passes ----
 * The calls above refuse a chain with the output AGC, and keep doing so: its state at a position is a function of the whole stream in
 * front of it.  For the digital profile that function factors.  What agc_apply measures of a chunk is the chunk's peak max |x| BEFORE
 * the gain, which does not depend on the AGC state; the state (iqgpu_agc_state) then advances chunk by chunk as a function of
 * (state, that chunk's peak, that chunk's output length) alone, with IQGPU_AGC_CLOCK_SAMPLES; and the gain of a chunk follows from
 * the state in front of it and its own peak.  So a capture of F frames is cut over N chains (one per GPU) like this, and the
 * stitched output is, byte for byte, what ONE chain writes (to the DC bound above on chains with the DC blocker):
 *   0. Placement does not depend on the AGC.  With `na` = a copy of the description with agc_enable = 0:
 *      P = iqgpu_design_preroll_frames(&na), and iqgpu_design_out_frames_range(&na, first, frames, ...) places every range's output.
 *      Cut points are multiples of lcm(agc_chunk_frames, the frames per process call) -- the digital AGC works on the chunks of each
 *      call, so every call of every chain has to lie on the single stream's call and chunk grid -- and of 4096 (see above).
 *   1. Measure (all ranges but the last, in parallel): iqgpu_chain_seek_agc(c, first, preroll, P', NULL) with P' = min(first, P),
 *      then iqgpu_chain_measure (from host memory: iqgpu_chain_measure_submit / _collect) over the range in the calls the single
 *      stream would make.  Every call yields one iqgpu_agc_chunk row
 *      per chunk; keep them in order.
 *   2. Walk (any one chain, a fraction of a second): st = iqgpu_chain_agc_initial_state; for every range s in order:
 *      entry[s] = st, then iqgpu_chain_agc_advance(c, &st, rows of range s, n, NULL).
 *   3. Process (all ranges in parallel): iqgpu_chain_seek_agc(c, first, preroll, P', &entry[s]), then the ordinary process /
 *      process_device / submit loop over the range in the same calls as pass 1.
 * iqgpu_chain_measure, _agc_advance and _seek_agc: IQGPU_EINVAL on a chain without the output AGC, IQGPU_EUNSUPPORTED for the profiles dx / local (agc_crcf's
 * loop forgets its past only approximately: no table of per-chunk figures carries its state exactly) and for IQGPU_AGC_CLOCK_WALL
 * (a wall clock has no value at a stream position). */
typedef struct {
    double   peak2;                     /* max re^2 + im^2 (exact products and sum, in double) over the chunk's frames in front of the AGC */
    uint32_t frames_out;                /* how many frames that is (0: an empty chunk, which never reaches agc_apply) */
    uint32_t reserved;
} iqgpu_agc_chunk;
/* The chain consumes the frames exactly as iqgpu_chain_process would (position, histories, NCO phases, FFT remainder and DC state all
 * advance), emits nothing, leaves the AGC state alone, and reports one row per agc_chunk_frames-sized chunk of THIS call, cut from
 * its first frame like process(): ceil(frames_in / agc_chunk_frames) rows; IQGPU_ECAPACITY when cap is below that.  On the device: the
 * chain's fastest unfused kernels, one reduction pass over their cf32 output, one copy of the rows to the host -- no scan, no gain,
 * no pack, no samples to the host.  Both variants return with the chain's stream idle and the rows in `rows` (host memory). */
int    iqgpu_chain_measure(iqgpu_chain *c, const void *raw_in, size_t frames_in, iqgpu_agc_chunk *rows, size_t cap, size_t *n_rows);
int    iqgpu_chain_measure_device(iqgpu_chain *c, const void *d_raw_in, size_t frames_in, iqgpu_agc_chunk *rows, size_t cap, size_t *n_rows);
/* Pipelined form of iqgpu_chain_measure (ABI v9), as iqgpu_chain_submit is of iqgpu_chain_process: pass 1 of a host-fed job at the
 * rate of the copy engine instead of copy, kernels and row copy one after the other.  The batch takes a slot of the SAME pipeline
 * as iqgpu_chain_submit -- same tickets, same iqgpu_chain_pipeline_depth() -- and is collected with iqgpu_chain_collect(c, ticket).
 * *n_rows = ceil(frames_in / agc_chunk_frames) is exact on return; the rows themselves are copied into `rows` (host memory, pinned
 * for the copy to be asynchronous) by the batch's drain step and are there once the ticket is collected.  raw_in and rows must stay
 * untouched until then.  Batches run in submit order on the chain's stream, and measure batches may be mixed with iqgpu_chain_submit
 * batches on one chain: they advance the one stream position in order, as mixed process / measure calls do.  A measure batch neither
 * reads nor writes the AGC state, so its launch never waits for an AGC verdict of its own; the verdict a process batch in front of
 * it still owes is resolved first, as before any batch.  frames_in == 0 takes a ticket and yields no rows.  Errors: those of
 * iqgpu_chain_measure (IQGPU_EINVAL without the output AGC, IQGPU_EUNSUPPORTED for dx / local and the wall clock, IQGPU_ECAPACITY
 * when cap is below the row count) and the pipeline's (IQGPU_EINVAL when every slot is in flight; a kernel failure is reported by
 * the call that launches the batch); a refused call leaves the handle exactly as it was. */
int    iqgpu_chain_measure_submit(iqgpu_chain *c, const void *raw_in, size_t frames_in, iqgpu_agc_chunk *rows, size_t cap,
                                  size_t *n_rows, uint64_t *ticket);
/* agc_apply's state machine over a table: *st is advanced over rows[0 .. n) (rows with frames_out == 0 are skipped, as empty chunks
 * never reach agc_apply); gains, if not NULL, receives the gain every row is multiplied with (n floats).  It runs the kernel that
 * walks the chunks of an ordinary call, so the state and the gains are the ordinary path's bit for bit, however the rows are grouped
 * into calls.  Uses the chain's target level, rate and device; does not touch the chain's own AGC state or stream position.
 * Rows of iqgpu_chain_measure always qualify; a table built by hand must keep peak2 >= 0 (no NaN) and the frames_out of any 64
 * consecutive rows below 2^31 in sum (the walk adds 64 lengths in 32 bits: the bound iqgpu_chain_create puts on agc_chunk_frames),
 * else IQGPU_EINVAL. */
int    iqgpu_chain_agc_advance(iqgpu_chain *c, iqgpu_agc_state *st, const iqgpu_agc_chunk *rows, size_t n, float *gains);
/* counterpart of iqgpu_chain_get_agc_state for a fresh stream: what agc_create / agc_reset leave (no device call) */
int    iqgpu_chain_agc_initial_state(const iqgpu_chain *c, iqgpu_agc_state *st);
/* iqgpu_chain_seek for chains with the digital AGC; arguments, preroll length rules and what is reset are iqgpu_chain_seek's.  The
 * preroll runs with the AGC out of the way: nothing it emits is kept and the AGC state is not advanced by it.  entry != NULL: the
 * chain then carries *entry as its AGC state (on the device and in every host mirror of it), as if it had processed
 * [0, first_frame).  entry == NULL: the AGC state is the fresh one -- what a measuring chain needs, which never reads it. */
int    iqgpu_chain_seek_agc(iqgpu_chain *c, uint64_t first_frame, const void *preroll, size_t preroll_frames, const iqgpu_agc_state *entry);
int    iqgpu_chain_seek_agc_device(iqgpu_chain *c, uint64_t first_frame, const void *d_preroll, size_t preroll_frames,
                                   const iqgpu_agc_state *entry);
/* ---- EXACT seamless range sharding of chains with the DC blocker: carry the blocker's state (additive, still ABI v9) ----
 * iqgpu_chain_seek warms the DC blocker up over ceil(ln(1e6) / alpha) extra frames and meets the single stream to 1e-6 of full scale.
 * The calls below meet it byte for byte and need no such warm-up.  The blocker is a one-pole recurrence, so what a process CALL does
 * to its state v is an affine map, v_after = f * v_before + g, whose pair (f, g) -- computed in double by the kernel that computes the
 * state of an ordinary call -- depends on the call's input frames and on how the call is cut into the front kernel's segments, and
 * NOT on v_before.  So a range is measured without knowing its entering state, one row per call, at the cost of one read of the
 * input (k_dc_prefix and the scan: no front kernel, no filter, no output); one walk over the rows gives the state in front of every
 * call; and a seek that is handed that state replaces the warm-up.
 * Contract.  The single stream is processed in calls on a grid of C frames (calls [k C, (k+1) C), the last one may be shorter).  Cut
 * points are multiples of C and of 4096.  With `nd` = a copy of the description with dc_block_enable = 0 and
 * P_fir = iqgpu_design_preroll_frames(&nd), the preroll of a range is the ceil(P_fir / C) whole grid calls in front of its cut (all
 * of [0, cut) when that is less), passed with call_frames = C, and at_preroll_start is the walked state in front of the first of
 * those calls.  Under these rules the stitched output equals the single stream's BYTE FOR BYTE: every call a shard makes is a call
 * the single stream makes, from the same state.  (The segments of a call also depend on whether its input address is 16-byte
 * aligned: the host variants stage every call as iqgpu_chain_process does; with the _device variants give every call the alignment
 * the single stream's call has.)  A preroll off the grid keeps the DC state exact and leaves the histories, and so the first
 * outputs, only within the bound of iqgpu_chain_seek.
 * Recipe:
 *   1. Measure (all ranges but the last, in parallel): ONE iqgpu_chain_dc_measure_range over the range (below: every grid call of it in
 *      one submission), or iqgpu_chain_dc_measure for every grid call of the range; one row per call, in order, the same rows either way.
 *   2. Walk (any one chain): st = {0, 0}; ONE iqgpu_chain_dc_advance over all rows with before[]: before[k] is the state in front of
 *      grid call k.
 *   3. Process (all ranges in parallel): iqgpu_chain_seek_dc(c, cut, preroll, n C, C, &before[cut / C - n]), then the ordinary
 *      process / process_device / submit loop over the range on the grid.
 * Errors: IQGPU_EINVAL for a chain without the DC blocker, a NULL argument, a position beyond 2^39 frames, a preroll shorter than
 * min(first_frame, P_fir) or not a multiple of call_frames, and (dc_advance) a row whose f is not in (0, 1] or whose g is not finite;
 * IQGPU_EUNSUPPORTED from dc_measure, dc_advance and seek_dc for a chain with the output AGC (its measure route may cut a call into
 * other segments than its process route; such chains keep iqgpu_chain_seek_agc and the bound above).  iqgpu_chain_get_dc_state works
 * on any chain with the blocker.  A refused iqgpu_chain_seek_dc leaves the chain as a refused iqgpu_chain_seek does: reset.
 * Call length: f = (1 - alpha)^frames is computed in double and underflows to 0 once frames * alpha exceeds about 745 (alpha =
 * 2 pi 10 Hz / rate: 1.18e8 frames at 10 MS/s, 2.8e7 at 2.4 MS/s).  iqgpu_chain_dc_measure still returns such a row -- f = 0 is then
 * the true map in double, v_after = g -- but iqgpu_chain_dc_advance refuses it with the other rows no measurement of a walkable
 * call gives: keep the calls of the grid below that length (the harness's default is 2^22 frames). */
typedef struct { double re, im; } iqgpu_dc_state;                          /* the blocker's v, in double as the chain keeps it */
typedef struct { double f, g_re, g_im; uint64_t frames; } iqgpu_dc_row;    /* one CALL: v_after = f * v_before + g */
/* synchronises the chain's stream and reports the blocker's state behind the last call */
int    iqgpu_chain_get_dc_state(iqgpu_chain *c, iqgpu_dc_state *st);
/* The map of the call iqgpu_chain_process[_device] would make of these frames_in frames at stream position first_frame: planned as
 * that call (same routing, same segments, the chain's switch snapshot), of which only k_dc_prefix and the scan are launched.  Returns
 * with the stream idle and leaves the handle exactly as it was: position, histories, DC state and pipeline untouched. */
int    iqgpu_chain_dc_measure(iqgpu_chain *c, uint64_t first_frame, const void *raw_in, size_t frames_in, iqgpu_dc_row *row);
int    iqgpu_chain_dc_measure_device(iqgpu_chain *c, uint64_t first_frame, const void *d_raw_in, size_t frames_in, iqgpu_dc_row *row);
/* *st walked over rows[0 .. n) on the device, by the expression behind the ordinary call's state update (one definition): the
 * walked state is the ordinary path's bit for bit.  before, if not NULL, receives the state in front of every row (n entries); *st
 * ends behind the last row.  Touches neither the chain's own DC state nor its position. */
int    iqgpu_chain_dc_advance(iqgpu_chain *c, iqgpu_dc_state *st, const iqgpu_dc_row *rows, size_t n, iqgpu_dc_state *before);
/* iqgpu_chain_seek with two differences: the preroll it asks for is min(first_frame, P_fir) -- no DC warm-up -- and
 * *at_preroll_start (NULL: zero) becomes the blocker's state before the preroll runs.  The preroll runs through the ordinary path in
 * calls of call_frames frames; call_frames == 0: one call. */
int    iqgpu_chain_seek_dc(iqgpu_chain *c, uint64_t first_frame, const void *preroll, size_t preroll_frames, size_t call_frames,
                           const iqgpu_dc_state *at_preroll_start);
int    iqgpu_chain_seek_dc_device(iqgpu_chain *c, uint64_t first_frame, const void *d_preroll, size_t preroll_frames, size_t call_frames,
                                  const iqgpu_dc_state *at_preroll_start);
/* ---- EXACT seamless range sharding of chains with the DC blocker AND the digital output AGC (additive, still ABI v9) ----
 * The two exact recipes above refuse each other's chains: iqgpu_chain_dc_measure* / _dc_advance / _seek_dc* answer
 * IQGPU_EUNSUPPORTED on a chain with the AGC, and iqgpu_chain_seek_agc meets a chain with the blocker only to the 1e-6 warm-up bound,
 * so that the AGC's decisions ride on a stream that is not bit-equal.  The calls below are the third recipe, for chains with
 * dc_block_enable and agc_enable / IQGPU_AGC_DIGITAL / IQGPU_AGC_CLOCK_SAMPLES (the shape of the reference's hd-radio-isolate preset).
 * What stood in the way: past the AGC's lock the library applies the gain in the chain's last kernel, and the call that holds the
 * locking chunk is CUT into two pieces -- the unfused head up to that chunk, the fused rest -- each planned on its own, so the
 * blocker's state is rounded once per piece, over that piece's segments.  The cut is a closed form of the stream position and the
 * call grid, not of any AGC value: the stream locks on the first non-empty chunk that starts after 2 s of output, and with calls on a
 * grid of multiples of agc_chunk_frames every chunk starts on such a multiple from frame 0.  So a chain can be told how the single
 * stream cuts the call at any position without knowing its AGC state, and these calls plan every call through the one function
 * that cuts the ordinary call.
 * A SHADOW call is the ordinary call at its position with nothing kept: the same pieces, each with the ordinary piece's plan and
 * segments and the same DC-state update, histories and position; the gain of a scratch state (1.0) where the ordinary piece
 * applies the gain in its front kernel, the cf32 output of the same filter launch where it applies it in the filter's epilogue; no
 * verdict, no fallback, nothing to the caller; the chain's AGC state neither read nor written; the host's mirrors of "locked" and
 * "frames seen", from which the next call's cut follows, advanced as the ordinary call advances them.
 * Contract: the union of the two above.  The single stream is processed on a grid of C frames; C and every cut are multiples of
 * agc_chunk_frames and of 4096; the preroll of a range is the ceil(P_fir / C) grid calls in front of its cut (all of [0, cut) when
 * that is less), with P_fir = iqgpu_design_preroll_frames of the description with dc_block_enable = 0 and agc_enable = 0.
 * Recipe:
 *   1. DC measure (all ranges but the last, in parallel): ONE iqgpu_chain_dcagc_dc_measure_range over the range (it returns first_row[]),
 *      or iqgpu_chain_dcagc_dc_measure for every grid call, in order -- the same rows either way.  A call yields
 *      ONE ROW PER PIECE (1 or 2: two for the call the single stream cuts); keep all rows and note the first row index of every call.
 *      The two maps of a cut call must not be merged: the single stream rounds its state behind each piece.
 *   2. DC walk (any one chain): st = {0, 0}; one iqgpu_chain_dcagc_dc_advance over all rows with before[]: the state in front of
 *      grid call k is before[first_row[k]].
 *   3. AGC measure (all ranges but the last, in parallel): iqgpu_chain_dcagc_seek(c, cut, preroll, n C, C, &dc_before, NULL) with
 *      dc_before the walked state in front of the first preroll call, then iqgpu_chain_dcagc_measure over the range on the grid;
 *      keep the rows in order.  (No pipelined form: iqgpu_chain_measure_submit makes no shadow calls; pass 3 is synchronous.)
 *   4. AGC walk, as above: iqgpu_chain_agc_initial_state, iqgpu_chain_agc_advance per range, entry[s] in front of range s.
 *   5. Process (all ranges in parallel): iqgpu_chain_dcagc_seek(..., &dc_before, &entry[s]), then the ordinary process /
 *      process_device / submit loop over the range on the grid.
 * The stitched bytes, the DC state and the AGC state equal the single stream's bit for bit.  With the _device variants give every
 * call the alignment (mod 16 bytes) the single stream's call has, as for iqgpu_chain_seek_dc_device.  Cost: pass 1 reads the input
 * once (k_dc_prefix and the scan), pass 3 is one process pass without the copy of the output, pass 5 is the process pass.
 * The I/Q correction factors are whatever the caller sets, the same on every chain; factors moved by the optimiser are a function
 * of wall time and outside this contract.
 * Errors.  IQGPU_EINVAL: a chain without the blocker or without the AGC; a NULL argument; a position beyond 2^39 frames; first_frame,
 * call_frames or a preroll that is not a multiple of agc_chunk_frames; a preroll shorter than min(first_frame, P_fir) or not whole
 * calls; a DC state that is not finite; agc_entry->locked outside {0, 1}; cap < 2 (dcagc_dc_measure); a row iqgpu_chain_dc_advance
 * refuses.  IQGPU_ECAPACITY: cap below ceil(frames_in / agc_chunk_frames) (dcagc_measure, as iqgpu_chain_measure).
 * IQGPU_EUNSUPPORTED: the AGC profiles dx / local and IQGPU_AGC_CLOCK_WALL.  A refused seek leaves the chain reset; a refused
 * measure leaves the handle as it was. */
/* The maps of the call iqgpu_chain_process[_device] would make of these frames at first_frame (a multiple of agc_chunk_frames): one
 * row per piece, in order, rows[i].frames the piece's length; cap >= 2.  Every piece is planned as the ordinary piece (routing,
 * segments, its own start address' alignment); only k_dc_prefix and the scan are launched.  Leaves the handle exactly as it was. */
int    iqgpu_chain_dcagc_dc_measure(iqgpu_chain *c, uint64_t first_frame, const void *raw_in, size_t frames_in, iqgpu_dc_row *rows,
                                    size_t cap, size_t *n_rows);
int    iqgpu_chain_dcagc_dc_measure_device(iqgpu_chain *c, uint64_t first_frame, const void *d_raw_in, size_t frames_in, iqgpu_dc_row *rows,
                                           size_t cap, size_t *n_rows);
/* iqgpu_chain_dc_advance's walk (same kernel, one definition) for these chains */
int    iqgpu_chain_dcagc_dc_advance(iqgpu_chain *c, iqgpu_dc_state *st, const iqgpu_dc_row *rows, size_t n, iqgpu_dc_state *before);
/* The chain at first_frame: reset; *dc_at_preroll_start (NULL: zero) as the blocker's state in front of the preroll; the host's lock /
 * seen mirrors at their closed form at first_frame - preroll_frames; the preroll as SHADOW calls of call_frames frames (0: one
 * call); then *agc_entry (NULL: the fresh state, for a measuring chain) installed as iqgpu_chain_seek_agc installs it. */
int    iqgpu_chain_dcagc_seek(iqgpu_chain *c, uint64_t first_frame, const void *preroll, size_t preroll_frames, size_t call_frames,
                              const iqgpu_dc_state *dc_at_preroll_start, const iqgpu_agc_state *agc_entry);
int    iqgpu_chain_dcagc_seek_device(iqgpu_chain *c, uint64_t first_frame, const void *d_preroll, size_t preroll_frames, size_t call_frames,
                                     const iqgpu_dc_state *dc_at_preroll_start, const iqgpu_agc_state *agc_entry);
/* The AGC rows of the ordinary call at the chain's position, as a SHADOW call: consumes the frames like iqgpu_chain_process (position,
 * histories, DC state, lock / seen mirrors), emits nothing, leaves the AGC state alone; one row per chunk of the call, the rows of
 * a cut call joined in chunk order, every peak2 exact.  Returns with the stream idle. */
int    iqgpu_chain_dcagc_measure(iqgpu_chain *c, const void *raw_in, size_t frames_in, iqgpu_agc_chunk *rows, size_t cap, size_t *n_rows);
int    iqgpu_chain_dcagc_measure_device(iqgpu_chain *c, const void *d_raw_in, size_t frames_in, iqgpu_agc_chunk *rows, size_t cap,
                                        size_t *n_rows);
/* ---- seamless range sharding of chains with the DX / LOCAL output AGC: a bounded window and a seam certificate (additive, still ABI v9) ----
 * Every seek above refuses the profiles dx / local, and keeps doing so: agc_crcf's per-sample loop has no closed form and no table of
 * per-chunk figures carries its state.  What the library's own kernels make of it does have a bounded window (agc.hip).  The output
 * is cut into chunks on a grid that belongs to the STREAM (chunk k = output frames [k C, (k+1) C), C = max(256, warm / 16), warm =
 * 26 / alpha: 2600 / 256 for local, 260 000 / 16 250 for dx), and every chunk runs a trajectory of its own: it starts warm samples
 * ahead of k C from a guess made of 256 samples of that window alone -- within warm samples of the reset: at the reset, from the reset
 * state -- and is ACCEPTED when it arrives within 2e-6 of where the chunk before it left.  What the single stream emits for an
 * accepted chunk, and the state it carries through and behind it, is that trajectory bit for bit, under any split into calls.  So
 * the state in front of output frame `cut` is a function of the warm + C pre-AGC samples in front of it at most: iqgpu_chain_seek_rms
 * re-runs the trajectory of chunk (cut - 1) / C -- one definition of its start and of the per-sample step with the streaming
 * kernel -- over the samples its preroll has produced, and the chain continues the single stream byte for byte.
 * The exception is a chunk whose speculation was REJECTED: the loop freezes its gain while the smoothed output energy is <= 1e-6, so
 * through a silent stretch the state is a value from arbitrarily far back, which no bounded window knows; the single stream then
 * re-runs that chunk from its predecessor's end, and a seek into it lands on the speculated state instead.  That cannot be known
 * from the window -- but it shows at the seam, at no cost:
 * THE SEAM CERTIFICATE.  Ranges s = 0 .. N-1 of one stream, each on a chain of its own: range 0 from a fresh chain, range s > 0 behind
 * iqgpu_chain_seek_rms(first[s]).  Read E[s] = iqgpu_chain_get_agc_state after range s has been processed (and keep its
 * iqgpu_chain_save_state blob), and S[s+1] = iqgpu_chain_get_agc_state of chain s+1 right after its seek.  If current_gain,
 * peak_memory and samples_seen of S[s+1] and E[s] are bit-equal, chain s+1 started from the state chain s ended in; when that holds
 * at every seam in order, E[s] is the single stream's state at every cut (induction from range 0) and the stitched output is the
 * single stream's byte for byte.  A seam that differs: iqgpu_chain_load_state of chain s's end-of-range blob into chain s+1, process
 * range s+1 again, take its new end state as E[s+1] and re-check seam s+2 against it.  The output is thus always the single
 * stream's; the work is parallel wherever the seams certify and sequential only for a range behind a seam that does not.
 * When a seam does not certify: when the single stream's chunk that holds the last output in front of the cut was rejected -- in
 * practice a cut inside or just behind a stretch whose AGC output energy stays <= 1e-6 (digital silence, a gap in the capture) for
 * more than a chunk.  On a capture that carries signal or receiver noise there, every seam certifies.  One more case: a chain with
 * an FFT user filter.  Its overlap-save windows start at the head of a call's buffer, so the last bits of what the filter emits --
 * the AGC's input -- follow the cuts of the calls, and the preroll is a call of its own: such a seam certifies where the single
 * stream made that very call ([first_frame - preroll_frames, first_frame)) and as a rule not elsewhere.  The certificate catches
 * it like the silent case, and the fallback gives the single stream's bytes.  FIR filters and chains without a filter: any calls.
 * iqgpu_design_preroll_frames_rms (no device): P_rms = P_fir + E, with P_fir = iqgpu_design_preroll_frames of the description with
 * agc_enable = 0 and E the input frames that make the chain emit at least n = warm + C outputs wherever they lie in the stream.  With
 * 2^S the half-band factor, step the 24-bit phase step (iqgpu_chain_info.arb_step), B the FFT block of the user filter and
 * q = B - 1 (0 without an FFT filter):  no resampler E = n + q;  r < 1 (the filter behind the resampler)
 * E = ceil((n + q) step / 2^24) * 2^S;  r >= 1 (the filter in front) E = ceil(ceil(n / 2^S) step / 2^24) + q.  (E frames close at
 * least E / 2^S groups, g groups give at least floor(g 2^24 / step) resampler outputs, a block boundary holds back at most q.)
 * Validation and error codes of iqgpu_design_probe, then the refusals of iqgpu_chain_seek_rms.
 * iqgpu_chain_seek_rms[_device]: arguments, reset semantics and preroll rule of iqgpu_chain_seek with P_rms for the preroll:
 * preroll_frames >= min(first_frame, P_rms), longer is allowed.  The preroll runs through the ordinary kernels with the AGC out of
 * the way (cf32 kept on the device; the I/Q probe takes no block); then one launch of k_agc_rms_seek leaves gain, peak_memory and
 * samples_seen at first_frame in the chain's AGC state, and the last warm pre-AGC samples become the warm-up window of the calls to
 * come.  Returns with the stream idle; first_frame == 0 leaves a fresh chain.  Placement: iqgpu_design_out_frames_range of the
 * description with agc_enable = 0.  Cuts: any frame (multiples of 4096 keep the input alignment of the single stream's calls); the
 * calls behind a seek may have any lengths.  Cost: the preroll, plus at most warm + C dependent loop steps on one lane.
 * Errors.  IQGPU_EINVAL: a chain without the output AGC, a NULL argument, a position beyond 2^39 frames, a preroll shorter than
 * min(first_frame, P_rms) or longer than first_frame.  IQGPU_EUNSUPPORTED: the digital profile (it has iqgpu_chain_seek_agc); a chain
 * with the DC blocker (its exact route needs a call grid and a walked state, iqgpu_chain_seek_dc; iqgpu_chain_dcrms_* below compose
 * the two).  A refused seek leaves the chain reset. */
int    iqgpu_design_preroll_frames_rms(const iqgpu_chain_desc *d, uint64_t *frames);
int    iqgpu_chain_seek_rms(iqgpu_chain *c, uint64_t first_frame, const void *preroll, size_t preroll_frames);
int    iqgpu_chain_seek_rms_device(iqgpu_chain *c, uint64_t first_frame, const void *d_preroll, size_t preroll_frames);
/* ---- EXACT seamless range sharding of chains with the DC blocker AND the DX / LOCAL output AGC (additive, still ABI v9) ----
 * The last chain shape without a seek: iqgpu_chain_seek_rms* refuses the blocker, iqgpu_chain_dc_measure* / _dc_advance / _seek_dc*
 * refuse a chain with the AGC, iqgpu_chain_dcagc_* refuse dx / local -- and all of them keep doing so.  The calls below compose
 * iqgpu_chain_seek_dc and iqgpu_chain_seek_rms.  Why they fit: a dx / local chain never cuts a call (only the digital profile has its
 * gain fused into the chain's last kernel), so every call is ONE piece on the unfused route -- cf32 into the AGC's buffer, then the RMS
 * kernels -- and the blocker's map of a call is one row, planned as that call.  iqgpu_chain_seek_rms needs the pre-AGC cf32 samples in
 * front of the cut to be the single stream's bit for bit; behind the blocker they are only if the blocker's state is, which the 1e-6
 * warm-up of iqgpu_chain_seek does not give: the state is walked and the preroll is made of the single stream's own calls, as for
 * iqgpu_chain_seek_dc.  The cf32 outputs of those preroll calls are gathered contiguously on the device and k_agc_rms_seek runs over
 * them as in iqgpu_chain_seek_rms.
 * Contract: the union of the two.  The single stream is processed in calls on a grid of C frames (the last call may be shorter); C and
 * every cut are multiples of 4096.  P = iqgpu_design_preroll_frames_dcrms = iqgpu_design_preroll_frames_rms of the description with
 * dc_block_enable = 0.  The preroll of a range is the ceil(P / C) whole grid calls in front of its cut (all of [0, cut) when that is
 * less), passed with call_frames = C, and dc_at_preroll_start is the walked state in front of the first of those calls.  With the
 * _device variants give every call the alignment (mod 16 bytes) the single stream's call has.  Behind such a seek the SEAM CERTIFICATE
 * of iqgpu_chain_seek_rms and its checkpoint fallback apply unchanged (a cut in or behind a stretch whose AGC output energy stays
 * <= 1e-6 for more than a chunk does not certify; behind the blocker a constant input, digital silence included, comes out as the
 * blocker's decaying state, which may or may not stay under that threshold).  The calls behind the seek are the grid's calls: the blocker's
 * state is rounded once per call.  Placement: iqgpu_design_out_frames_range of the description with agc_enable = 0.
 * Recipe:
 *   1. DC measure (all ranges but the last, in parallel): ONE iqgpu_chain_dcrms_dc_measure_range over the range, or
 *      iqgpu_chain_dcrms_dc_measure for every grid call; one row each, in order, the same rows either way.
 *   2. Walk (any one chain): st = {0, 0}; ONE iqgpu_chain_dcrms_dc_advance over all rows with before[]: before[k] is the state in
 *      front of grid call k.
 *   3. Process (all ranges in parallel): iqgpu_chain_dcrms_seek(c, cut, preroll, n C, C, &before[cut / C - n]), read S[s] =
 *      iqgpu_chain_get_agc_state, then the ordinary process / process_device / submit loop over the range on the grid; read E[s] and
 *      keep the iqgpu_chain_save_state blob.
 *   4. The certificate per seam, in order (see iqgpu_chain_seek_rms): a range behind a seam that does not certify is redone from
 *      iqgpu_chain_load_state of the range in front.
 * Where the seams certify, the stitched bytes, the DC state and the AGC state are the single stream's bit for bit; elsewhere the
 * fallback makes them so.
 * FFT user filters.  iqgpu_chain_seek_rms certifies such a chain only where the single stream made the very call its preroll is.  Here
 * the preroll calls ARE the single stream's calls (same position, same length, same pending samples, so the same overlap-save
 * windows).  Observed (tests/test_gpu_seek_dcrms.py, shape local_fft_cf32: NRSC-5 rate, passband FFT filter, cf32 out, C = 65 536, cuts
 * at 4 C and 10 C): both seams certified and the stitched bytes were the single stream's without the fallback.  This is an
 * observation, not a promise: the certificate decides, and the fallback covers a seam that does not certify.
 * iqgpu_design_preroll_frames_dcrms (no device): validation and error codes of iqgpu_design_probe, then IQGPU_EINVAL for a description
 * without the blocker or without the AGC and IQGPU_EUNSUPPORTED for the digital profile.
 * iqgpu_chain_dcrms_dc_measure[_device]: iqgpu_chain_dc_measure for these chains -- ONE row, the call planned as the ordinary call at
 * first_frame, only k_dc_prefix and the scan launched, the handle left exactly as it was.
 * iqgpu_chain_dcrms_dc_advance: iqgpu_chain_dc_advance's walk (same kernel, one definition, same row checks) for these chains.
 * iqgpu_chain_dcrms_seek[_device]: reset; *dc_at_preroll_start (NULL: zero) becomes the blocker's state in front of the preroll; the
 * preroll runs in calls of call_frames frames (0: one call), each staged like a call of iqgpu_chain_process, with the AGC out of the
 * way and the I/Q probe left alone; then one launch of k_agc_rms_seek over the gathered cf32 samples leaves gain, peak_memory and
 * samples_seen at first_frame, the last warm samples become the warm-up window of the calls to come, and iqgpu_chain_tell reports
 * first_frame.  Preroll rule: min(first_frame, P) <= preroll_frames <= first_frame, a whole number of calls when call_frames != 0.
 * first_frame == 0 leaves a fresh chain.  Returns with the stream idle.
 * Errors.  IQGPU_EINVAL: a chain without the blocker or without the AGC; a NULL argument; a position beyond 2^39 frames; a preroll
 * shorter than min(first_frame, P), longer than first_frame or not whole calls; a DC state that is not finite; a row
 * iqgpu_chain_dc_advance refuses.  IQGPU_EUNSUPPORTED: the digital profile (iqgpu_chain_dcagc_*).  A refused seek leaves the chain
 * reset; a refused measure leaves the handle as it was. */
int    iqgpu_design_preroll_frames_dcrms(const iqgpu_chain_desc *d, uint64_t *frames);
int    iqgpu_chain_dcrms_dc_measure(iqgpu_chain *c, uint64_t first_frame, const void *raw_in, size_t frames_in, iqgpu_dc_row *row);
int    iqgpu_chain_dcrms_dc_measure_device(iqgpu_chain *c, uint64_t first_frame, const void *d_raw_in, size_t frames_in, iqgpu_dc_row *row);
int    iqgpu_chain_dcrms_dc_advance(iqgpu_chain *c, iqgpu_dc_state *st, const iqgpu_dc_row *rows, size_t n, iqgpu_dc_state *before);
int    iqgpu_chain_dcrms_seek(iqgpu_chain *c, uint64_t first_frame, const void *preroll, size_t preroll_frames, size_t call_frames,
                              const iqgpu_dc_state *dc_at_preroll_start);
int    iqgpu_chain_dcrms_seek_device(iqgpu_chain *c, uint64_t first_frame, const void *d_preroll, size_t preroll_frames, size_t call_frames,
                                     const iqgpu_dc_state *dc_at_preroll_start);
/* ---- pass 1 of the three exact recipes over a whole RANGE in one call (additive, still ABI v9) ----
 * iqgpu_chain_dc_measure, _dcagc_dc_measure and _dcrms_dc_measure plan a call, launch two small kernels, copy 32 bytes back and
 * synchronise -- once per grid call, so that the pass spends most of its time between its kernels.  The calls below measure every grid
 * call of a range in ONE submission and synchronise once.  The frames [first_frame, first_frame + frames_in) are cut into the grid
 * calls [first_frame + k call_frames, ...), the last one may be shorter; first_frame is a multiple of call_frames.  rows receives
 * exactly the rows a loop of the family's per-call form over those calls writes, in order and BIT FOR BIT: one row per call (Dc,
 * DcRms); one row per piece, 1 or 2 per call, cut as iqgpu_chain_dcagc_dc_measure cuts it and never merged (DcAgc).  first_row, when
 * not NULL, receives the index of every call's first row (ceil(frames_in / call_frames) entries); *n_rows the total.  Every piece is
 * planned by the planning of the per-call form and computed by the device functions behind k_dc_prefix and k_dc_scan (k_dc_prefix_batch,
 * k_dc_scan_batch: a table of pieces in device memory, iqgpu_dc_measure_range_launch_entries() of them per launch, longer ranges in
 * several launches).  The handle is left exactly as it was -- position, histories, DC state, pipeline -- and the call returns with the
 * stream idle.  Rows with f == 0 (calls past the underflow length) are returned as the per-call form returns them.
 * _device: call k reads d_raw_in + k call_frames bytes_per_frame, and the alignment (mod 16 bytes) of THAT address enters its plan, as
 * for the per-call _device form: a misaligned base gives the rows of the per-call _device loop on the same addresses.
 * Host variants: the input is staged through device memory in slices of whole calls (2^24 frames, at least one call), two buffers,
 * the copy of slice s + 1 queued while the kernels of slice s run.  call_frames is a multiple of 4096, so every staged call starts
 * 16-byte aligned, as iqgpu_chain_process stages it: the rows are the per-call host form's rows.
 * Rules: call_frames is a non-zero multiple of 4096 -- for DcAgc, call_frames and first_frame are multiples of agc_chunk_frames too --
 * and positions stay within 2^39 frames, else IQGPU_EINVAL; so are a NULL chain, rows or n_rows, and a NULL buffer with frames_in != 0.
 * The chain is checked as by the family's other calls (IQGPU_EINVAL without the blocker, IQGPU_EUNSUPPORTED for the AGC shapes the
 * family refuses), under the new call's name.  cap below the row count: IQGPU_ECAPACITY with *n_rows set to the count needed (no
 * device call is made; cap = 2 ceil(frames_in / call_frames) always suffices).  frames_in == 0 writes no rows and succeeds.  A refused
 * call leaves the handle as it was. */
int    iqgpu_chain_dc_measure_range(iqgpu_chain *c, uint64_t first_frame, const void *raw_in, size_t frames_in, size_t call_frames,
                                    iqgpu_dc_row *rows, size_t cap, size_t *n_rows, uint32_t *first_row);
int    iqgpu_chain_dc_measure_range_device(iqgpu_chain *c, uint64_t first_frame, const void *d_raw_in, size_t frames_in, size_t call_frames,
                                           iqgpu_dc_row *rows, size_t cap, size_t *n_rows, uint32_t *first_row);
int    iqgpu_chain_dcagc_dc_measure_range(iqgpu_chain *c, uint64_t first_frame, const void *raw_in, size_t frames_in, size_t call_frames,
                                          iqgpu_dc_row *rows, size_t cap, size_t *n_rows, uint32_t *first_row);
int    iqgpu_chain_dcagc_dc_measure_range_device(iqgpu_chain *c, uint64_t first_frame, const void *d_raw_in, size_t frames_in,
                                                 size_t call_frames, iqgpu_dc_row *rows, size_t cap, size_t *n_rows, uint32_t *first_row);
int    iqgpu_chain_dcrms_dc_measure_range(iqgpu_chain *c, uint64_t first_frame, const void *raw_in, size_t frames_in, size_t call_frames,
                                          iqgpu_dc_row *rows, size_t cap, size_t *n_rows, uint32_t *first_row);
int    iqgpu_chain_dcrms_dc_measure_range_device(iqgpu_chain *c, uint64_t first_frame, const void *d_raw_in, size_t frames_in,
                                                 size_t call_frames, iqgpu_dc_row *rows, size_t cap, size_t *n_rows, uint32_t *first_row);
/* entries (pieces of calls) one launch of the range form's kernels holds; no device call */
size_t iqgpu_dc_measure_range_launch_entries(void);
/* ---- checkpoint / resume: everything a chain carries from call to call, in a caller-owned blob (additive, still ABI v9) ----
 * The seek calls above rebuild the state at a stream position from a closed form and a preroll, and refuse what has no such form.
 * These two calls need none: iqgpu_chain_save_state copies the state out between two calls, iqgpu_chain_load_state puts it into a
 * chain of the same description -- in this process or another, on this device or another -- and that chain continues the stream
 * byte for byte: the same kernels on the same state in the same calls.  They cover every chain the library builds: the output AGC
 * in all three profiles, the DC blocker with the AGC, factors moved by the I/Q optimiser.
 * What is carried: the stream position (open decimation group, resampler phase, both NCO phases, pending FFT-block samples) and
 * the two frame counters of iqgpu_chain_tell; the half-band / polyphase history of the front kernel and, behind k_cascade, of its
 * last stage; the user filter's [L-1 history][pending] buffer front; the history of the r >= 1 resampler; the DC blocker's state;
 * the AGC state with the host's mirrors of it and, for dx / local, the warm-up window and the position of its chunk grid; the I/Q
 * correction factors in force.  Not carried: the description itself (the loading chain is created from it as usual), the stream
 * and device the chain runs on, profiling, the I/Q probe, batches in flight (save runs them to their end first).
 * The blob: a 64-byte header (magic, format_version, total size, fingerprint, the two counters, a 64-bit checksum over all the
 * rest), the host-side words, then the device buffers as logical contents -- which buffer of a ping-pong pair is current is not
 * stored.  Its size is FIXED per description: buffers whose live length varies are stored at their maximum (the filter front at
 * L-1 + block) with the unused tail zeroed, so iqgpu_design_state_size needs no device and equals *bytes of every save, and the
 * blob is a function of the state alone: the same state gives the same bytes.  Little-endian, as the host is.
 * The fingerprint covers everything the layout and the meaning of the contents depend on: the description's fields that shape the
 * design and what the design derived from them (ratio bits, half-band plan, phase step, NCO step, filter taps and block, history
 * sizes, AGC chunk, target and profile, formats, gain, block_samples) and the chain's snapshot of the diagnostic switches, which
 * decides the routing and with it the history layouts.  It does not cover the I/Q factors, device_ordinal, the stream or profiling.
 * Refused: iqgpu_chain_save_state on a chain with IQGPU_AGC_CLOCK_WALL is IQGPU_EUNSUPPORTED (a monotonic clock reading means
 * nothing in another process: the policy of the two-pass calls); on a poisoned chain IQGPU_EHIP; with cap below the blob's size
 * IQGPU_ECAPACITY, *bytes set to the size needed (blob may then be NULL with cap 0: a size query).  iqgpu_chain_load_state checks
 * everything BEFORE it touches the chain -- NULL, size, magic, format_version, checksum, fingerprint against this chain, the range of
 * the position words -- and answers IQGPU_EINVAL with a message that names the mismatch; a refused load leaves the chain exactly as it
 * was (unlike a refused seek, which leaves it reset: here the validation is total).
 * iqgpu_chain_save_state first runs every batch already submitted and resolves a pending AGC verdict, as iqgpu_chain_get_agc_state
 * does, then copies; it changes nothing: a chain that saved continues exactly like one that did not, and the tickets in flight are
 * collected as usual.  iqgpu_chain_load_state then does what iqgpu_chain_reset does (batches in flight and a pending verdict
 * resolved, the poison cleared), installs the state and returns with the chain's stream idle; per-call scratch is left as after a
 * reset.  A stage thread checkpoints between calls; with batches in flight it collects the tickets it still wants first or after.
 * iqgpu_chain_tell: input frames consumed and output frames emitted since the last reset -- after a seek: first_frame and the index
 * of the stream's output frame there -- behind every batch already submitted (what submit() has promised, like
 * iqgpu_chain_next_out_frames).  No device call.
 * iqgpu_state_inspect: magic, version, size and checksum of a blob, and the header's figures; no device, no chain. */
typedef struct {
    uint32_t format_version;            /* of the blob layout                                     */
    uint32_t reserved;
    uint64_t bytes;                     /* total blob size                                        */
    uint64_t fingerprint;               /* of everything the layout and contents depend on        */
    uint64_t frames_in;                 /* input frames consumed since the last reset / seek base */
    uint64_t frames_out;                /* output frames emitted since then                       */
} iqgpu_state_info;
#define IQGPU_STATE_FORMAT_VERSION 1
/* size of the blob of a chain of this description; no device; same validation and error codes as iqgpu_design_probe */
int    iqgpu_design_state_size(const iqgpu_chain_desc *d, size_t *bytes);
int    iqgpu_state_inspect(const void *blob, size_t bytes, iqgpu_state_info *info);
int    iqgpu_chain_tell(iqgpu_chain *c, uint64_t *frames_in, uint64_t *frames_out);
int    iqgpu_chain_save_state(iqgpu_chain *c, void *blob, size_t cap, size_t *bytes);
int    iqgpu_chain_load_state(iqgpu_chain *c, const void *blob, size_t bytes);
/* what the I/Q optimiser thread publishes (src/iq_correct.c:141-152 reads them once per chunk) */
int    iqgpu_chain_set_iq_factors(iqgpu_chain *c, float mag, float phase);
/* synchronises the chain's stream and reports the AGC state (agc.c keeps it in AppResources) */
int    iqgpu_chain_get_agc_state(iqgpu_chain *c, iqgpu_agc_state *st);
/* upper bound on frames_out for a call with frames_in frames (>= ceil(n*max(1,r))+128 (+ FFT block),
 * the reference's buffer rule src/pipeline.c:246-258) */
size_t iqgpu_chain_max_out_frames(const iqgpu_chain *c, size_t frames_in);
/* exact number of frames the NEXT call with frames_in frames will produce */
size_t iqgpu_chain_next_out_frames(const iqgpu_chain *c, size_t frames_in);

/* ---- I/Q imbalance optimiser (host CPU, like the reference's): produces the factors iq_correct_apply consumes ----
 * iq_correct_init / iq_correct_run_optimization / helpers (src/iq_correct.c:85-139, 154-219, 315-393), the
 * optimiser thread's body (src/utility_threads.c:35-47) and the 1024-sample hand-off (src/pipeline.c:468-476).
 * A 1024-point Hamming-windowed spectrum of a pre-processed block, the squared dB asymmetry of its two halves over
 * the inner 90 % of the bins as utility, 25 random +-1e-4 steps per run, 5 % smoothing, at most one run per 500 ms
 * and only on blocks whose peak-to-average power is >= 20 dB. */
typedef struct iqgpu_iq_optimizer iqgpu_iq_optimizer;
typedef float (*iqgpu_rand_dir_fn)(void *user);   /* > 0: +1, else -1  (stands in for _get_random_direction, iq_correct.c:391) */
typedef struct {
    uint64_t calls, runs, skipped_interval, skipped_power, accepted;   /* accepted: candidates that raised the metric */
    float    initial_metric, final_metric;                            /* of the last run */
    float    average_power_db, power_range_db;                        /* of the last power estimate (iq_correct.c:362-389) */
} iqgpu_iq_optimizer_stats;
int   iqgpu_iq_optimizer_create(iqgpu_iq_optimizer **out);            /* factors (0, 0); srand(time) like iq_correct_init */
void  iqgpu_iq_optimizer_destroy(iqgpu_iq_optimizer *o);
/* direction source: by default libc rand() > RAND_MAX / 2 as in the reference (irreproducible by design);
 * seed() switches to a private minstd generator, set_rng() to the caller's function */
int   iqgpu_iq_optimizer_seed(iqgpu_iq_optimizer *o, uint32_t seed);
int   iqgpu_iq_optimizer_set_rng(iqgpu_iq_optimizer *o, iqgpu_rand_dir_fn fn, void *user);
int   iqgpu_iq_optimizer_set_factors(iqgpu_iq_optimizer *o, float mag, float phase);
int   iqgpu_iq_optimizer_get_factors(iqgpu_iq_optimizer *o, float *mag, float *phase);
int   iqgpu_iq_optimizer_get_stats(iqgpu_iq_optimizer *o, iqgpu_iq_optimizer_stats *st);
/* _calculate_imbalance_metric (iq_correct.c:339-360) of one 1024-sample cf32 block for candidate factors */
float iqgpu_iq_optimizer_metric(iqgpu_iq_optimizer *o, const float *block_re_im_1024, float mag, float phase);
/* iq_correct_run_optimization on one 1024-sample cf32 block; now_sec < 0 reads CLOCK_MONOTONIC as the reference
 * does, otherwise the caller's clock (e.g. stream time) gates the 500 ms interval.  *updated = 1 if factors changed. */
int   iqgpu_iq_optimizer_run(iqgpu_iq_optimizer *o, const float *block_re_im_1024, double now_sec, int *updated);
int   iqgpu_iq_optimizer_touch(iqgpu_iq_optimizer *o, double now_sec); /* restart the interval (iq_correct.c:294-297) */
/* The block the reference hands over: the first 1024 samples of a chunk AFTER unpack / dc block / iq correct / pre NCO
 * (src/pipeline.c:468-476; a shift behind the resampler is not part of it).  With the probe enabled a call leaves that block of
 * its first chunk in a pinned host buffer; read() waits for it.  *valid = 0 while there is none.  Which call:
 *   1. The block is the head of the first ORDINARY stream call of at least 1024 frames since the previous read --
 *      iqgpu_chain_process, _process_device, a batch of _submit -- with the I/Q factors that call applies (a submitted batch:
 *      those at its submit).  While a block is staged and unread no later call replaces it; once read it is returned by every
 *      read until a later call has left the next one.  The block is the head of the whole call, however the library cuts it.
 *   2. Calls that are no chunk of the running stream neither leave a block nor occupy the slot: the preroll inside
 *      iqgpu_chain_seek*, _seek_agc*, _seek_dc*, _dcagc_seek*, _seek_rms*, _dcrms_seek*, and iqgpu_chain_measure, _measure_device,
 *      _measure_submit, _dc_measure* (the _range forms too), _dcagc_dc_measure*, _dcagc_measure* (shadow calls leave no block),
 *      _dcrms_dc_measure*.
 *   3. iqgpu_chain_reset, every iqgpu_chain_seek* (iqgpu_chain_dcagc_seek*, iqgpu_chain_seek_rms* and iqgpu_chain_dcrms_seek* too) and
 *      iqgpu_chain_load_state drop a staged or held block (it belongs to the
 *      stream position the chain leaves): *valid = 0 until the next call of rule 1.
 *   4. A call shorter than 1024 frames leaves the slot as it is. */
int   iqgpu_chain_enable_iq_probe(iqgpu_chain *c, int enable);
int   iqgpu_chain_read_iq_probe(iqgpu_chain *c, float *block_re_im_1024, int *valid);
/* the optimiser thread's loop body: read the probe, run, publish with iqgpu_chain_set_iq_factors */
int   iqgpu_iq_optimizer_service(iqgpu_iq_optimizer *o, iqgpu_chain *c, double now_sec, int *updated);

/* ---- I/Q calibration: the optimiser's utility over many blocks and a grid of candidates, searched deterministically (additive, still ABI v9) ----
 * No counterpart in the reference.  Its optimiser above is a randomised +-1e-4 climb on ONE 1024-sample block per run behind a
 * 500 ms wall clock: its factors are a function of wall time, which no sharded or checkpointed job can reproduce.  The calls below
 * evaluate the reference's OWN utility -- same Hamming window, same dB spectrum, same bins i in [25, 486) with the pair 1023 - i, same
 * -80 dB gate, the same 20 dB peak-to-average gate per block -- over many blocks of a capture and a grid of candidate factors, and
 * search that surface by a fixed rule.  The result is one (mag, phase) pair, a pure function of the capture bytes and the options:
 * computed once in front of a job and handed to every shard with iqgpu_chain_set_iq_factors or in the description.  The streaming
 * optimiser, the probe and every other entry point are as they were.
 * The search (one function, iq_optimizer.cpp; the evaluator -- host metric or k_iq_metric -- is its only parameter).  A level's
 * candidates are the grid x grid pairs (centre_mag + (im - h) step, centre_phase + (ip - h) step), h = (grid - 1) / 2, candidate
 * index c = im * grid + ip, in float; level 0 is centred on (center_mag, center_phase) with step = 2 span / (grid - 1).
 * total[c] = the sum, in double and in block order, of metric[b][c] over the blocks whose power_range_db >= power_threshold_db.  The
 * pick is the candidate with the largest total; ties go to the one nearest the centre ((im - h)^2 + (ip - h)^2), then to the lowest
 * index.  The next level is centred on the pick with step <- step * 2 / (grid - 1); the search stops behind the first level whose step
 * is <= min_step, or behind 16 levels (grid = 3 keeps its step: it walks, up to 16 levels, and does not refine).  The factors are
 * the last level's pick.  power_threshold_db may be zero or negative: every block then counts.
 * Errors: IQGPU_EINVAL for a NULL argument, grid even or outside [3, 15], span, min_step or max_blocks not positive, any option
 * not finite, n_blocks == 0, a stride or an input below 1024 frames; the report is then all zero. */
typedef struct { float mag, phase; } iqgpu_iq_cand;
typedef struct {
    uint32_t max_blocks;          /* chain calls: blocks taken from the input, evenly spread (64) */
    uint32_t grid;                /* candidates per axis and level: odd, 3 .. 15 (9) */
    float    span;                /* level 0 reaches centre +- span on both axes (0.1) */
    float    min_step;            /* the level whose step is <= this is the last (1e-4: IQ_BASE_INCREMENT) */
    float    power_threshold_db;  /* blocks below this peak-to-average power do not count (20: IQ_CORRECTION_POWER_THRESHOLD_DB) */
    float    center_mag, center_phase;   /* centre of level 0 (0, 0) */
} iqgpu_iq_calib_opts;
void iqgpu_iq_calib_opts_init(iqgpu_iq_calib_opts *o);             /* the defaults in parentheses above */
typedef struct { float center_mag, center_phase, step; uint32_t pick; uint32_t reserved; double total_at_pick; } iqgpu_iq_calib_level;
typedef struct {
    int      found;               /* 0: no block passed the power gate -- mag, phase are the centre, n_levels = 0 */
    float    mag, phase;          /* the result: what iqgpu_chain_set_iq_factors / iq_mag, iq_phase of a description take */
    double   total_at_center0;    /* total of the centre of level 0: the utility before calibration */
    double   total_at_best;       /* total of the last level's pick */
    uint32_t blocks_taken;        /* blocks evaluated */
    uint32_t blocks_used;         /* ... of which passed the power gate */
    uint32_t n_levels;            /* entries of level[] */
    uint32_t evaluations;         /* candidates evaluated, over all levels (each on every block taken) */
    iqgpu_iq_calib_level level[16];
} iqgpu_iq_calib_report;
/* The utility (_calculate_imbalance_metric) of every (block, candidate) on the device: block b is the 1024 cf32 samples at
 * blocks_re_im + 2 * b * stride_frames floats (stride_frames >= 1024), metric[b * n_cand + c] its utility under cands[c], and
 * power_range_db[b] (NULL: not wanted) its peak-to-average power (_estimate_power).  One forward transform per block and tile of
 * candidates -- the correction is linear and the window real, so a candidate needs none of its own -- and a fixed summation order:
 * two calls on the same input give the same bits, and so do the host and the _device form.  Any n_cand >= 1: lists longer than
 * the per-launch bound (iqgpu_iq_metric_geometry) go in several launches.  The host form stages the blocks, not the gaps between
 * them; the _device form reads device memory of `device` on hip_stream (NULL: the null stream), writes host memory, and returns with
 * that stream idle.  Within 2e-4 max(1, |m|) of iqgpu_iq_optimizer_metric where no compared bin stands at the -80 dB gate.
 * d_blocks_re_im and every block start in it are aligned to 8 bytes (one cf32 sample; any stride_frames keeps that).  A
 * diagnostic and test entry point, not one for a loop: every call allocates and frees its device buffers and uploads its tables
 * (12 KB) again; iqgpu_chain_calibrate_iq keeps them with the chain. */
int   iqgpu_iq_metric_batch(int device, const float *blocks_re_im, size_t n_blocks, size_t stride_frames,
                            const iqgpu_iq_cand *cands, size_t n_cand, float *metric, float *power_range_db);
int   iqgpu_iq_metric_batch_device(int device, const float *d_blocks_re_im, size_t n_blocks, size_t stride_frames,
                                   const iqgpu_iq_cand *cands, size_t n_cand, float *metric, float *power_range_db, void *hip_stream);
/* diagnostics: candidates per launch of k_iq_metric and per wave of it (either pointer may be NULL); what a test needs to reach
 * the boundaries of iqgpu_iq_metric_batch, nothing a caller has to know */
void  iqgpu_iq_metric_geometry(size_t *cands_per_launch, size_t *cand_tile);
/* The search with the HOST metric (iqgpu_iq_optimizer_metric's, one definition) over blocks laid out as for iqgpu_iq_metric_batch.
 * No device.  Neither reads nor moves the optimiser's own factors, clock or statistics. */
int   iqgpu_iq_optimizer_calibrate(iqgpu_iq_optimizer *o, const float *blocks_re_im, size_t n_blocks, size_t stride_frames,
                                   const iqgpu_iq_calib_opts *opts, iqgpu_iq_calib_report *rep);
/* The search with k_iq_metric over blocks k_iq_blocks gathers from raw input in the chain's in_format: n = min(max_blocks,
 * frames_in / 1024) blocks, block b the 1024 frames from frame b * max(1024, frames_in / n).  A block is taken where iq_correct_apply
 * acts: behind unpack, gain and -- on a chain with the DC blocker -- the blocker run from a ZERO state with the chain's alpha (what
 * iq_correct_run_initial_calibration sees: a fresh pre-processor), with NO I/Q correction and NO NCO.  This differs from the
 * streaming probe (iqgpu_chain_read_iq_probe) on a chain with a pre-resample shift, on purpose: in front of the mixer the image of
 * the imbalance is mirror-symmetric about bin 0, which is what the utility measures; behind it, it is not.
 * Leaves the handle exactly as it was -- position, histories, DC state, AGC state, I/Q factors, probe slot and pipeline untouched --
 * and returns with the stream idle, like iqgpu_chain_dc_measure.  Neither needs nor sets iq_correct_enable: the caller publishes
 * rep->mag, rep->phase.  The host form stages the blocks it needs, not the whole input. */
int   iqgpu_chain_calibrate_iq(iqgpu_chain *c, const void *raw_in, size_t frames_in,
                               const iqgpu_iq_calib_opts *opts, iqgpu_iq_calib_report *rep);
int   iqgpu_chain_calibrate_iq_device(iqgpu_chain *c, const void *d_raw_in, size_t frames_in,
                                      const iqgpu_iq_calib_opts *opts, iqgpu_iq_calib_report *rep);
/* diagnostics and tests, no part of the calibration recipe: the blocks iqgpu_chain_calibrate_iq[_device] would evaluate, as cf32,
 * e.g. to evaluate them with the host metric.  blocks_re_im holds cap_blocks x 1024
 * samples, *n_blocks the number written.  Same selection, same kernel, same guarantees for the handle. */
int   iqgpu_chain_calibrate_iq_blocks(iqgpu_chain *c, const void *raw_in, size_t frames_in, uint32_t max_blocks,
                                      float *blocks_re_im, size_t cap_blocks, size_t *n_blocks);
int   iqgpu_chain_calibrate_iq_blocks_device(iqgpu_chain *c, const void *d_raw_in, size_t frames_in, uint32_t max_blocks,
                                             float *blocks_re_im, size_t cap_blocks, size_t *n_blocks);

/* ---- power spectrum of a stream: an averaged (Welch) periodogram with a max-hold trace, accumulated on the device (additive, still ABI v9) ----
 * No counterpart in the reference.  An accumulator over ONE stream of frames in ONE sample format, independent of any chain: it
 * serves the raw capture (a chain's in_format) and a chain's output (its out_format, packed integer output included: what the
 * writer writes) alike.  Where does the signal sit in the capture, is the stop band down in the output: both are read off it.
 * Segments: segment s is frames [s hop, s hop + nfft) of everything pushed since the last reset;
 * segments = frames < nfft ? 0 : (frames - nfft) / hop + 1.  The grid belongs to the stream, not to the calls: the accumulator carries
 * the trailing frames a later segment still needs (at most nfft - 1) in a device buffer of its own.
 * Per segment: x = the frame through the library's unpack (the expressions of iqgpu_convert_block_to_cf32) and the gain,
 * X_s[k] = sum_i w[i] x[s hop + i] exp(-2 pi i ik / nfft) in float.
 * Outputs, both in natural bin order (k = 0 is DC, k >= nfft / 2 the negative frequencies), either pointer may be NULL:
 *   sum_power[k]  = sum_s |X_s[k]|^2: each term the float value re^2 + im^2, summed in double.  Nothing is normalised.
 *   peak_power[k] = max_s |X_s[k]|^2 in float.
 * window_sum and window_sum_sq (the sums of w and w^2 over the float table, in double) are what a caller needs for the dBFS of a tone,
 * sum / (segments window_sum^2), or for power per Hz, sum / (segments rate window_sum_sq).
 * Windows: periodic (DFT-even) forms evaluated in double, rounded once to float, uploaded at create; iqgpu_psd_window returns the
 * same table.  HANN 0.5 - 0.5 cos(2 pi i / N); HAMMING 0.54 - 0.46 cos(2 pi i / N); BLACKMAN_HARRIS, 4 terms: 0.35875, 0.48829,
 * 0.14128, 0.01168.
 * THE RESULT IS A FUNCTION OF THE PUSHED FRAMES AND THE OPTIONS ALONE, BIT FOR BIT: any split of the stream into push calls, host or
 * device, of any lengths (one frame; lengths that are no multiples of hop) gives the same sum_power, peak_power and info -- the
 * convention of the chain above carried over.  The summation order belongs to the stream: segments are grouped by stream index into
 * pages of segments_per_page (iqgpu_psd_geometry) consecutive segments; a page is summed per bin in segment order, the total is
 * the pages added in page order, the open page (the one the stream position lies in) is kept apart and continued by the next push,
 * and read reports total + open.  Shards that each accumulate a range add their sum_power, take the max of their peak_power and add
 * their segments on the host: that sum is NOT promised bit-equal to the single stream's, and segments that straddle a cut are simply
 * not taken.
 * Errors: IQGPU_EINVAL for a NULL argument (of iqgpu_psd_window: o or w; sum and sum_sq may be NULL), nfft / hop / window outside
 * the lists, a gain that is not finite, cap < nfft; IQGPU_EFORMAT for an unknown format; IQGPU_ENODEV from create without a usable
 * device; IQGPU_ENOMEM; IQGPU_EHIP.  A refused call leaves the accumulator as it was; frames == 0 succeeds and changes nothing; one
 * thread per handle.  Non-finite input frames propagate by IEEE rules into the sum_power bins of their segments; what peak_power
 * reports for those segments is unspecified; accumulators that never see such frames are unaffected.
 * Streams: push_device is asynchronous on the stream it is given (NULL: the null stream) and the input must stay valid until that
 * stream has passed the work, as for iqgpu_chain_process_device; a push on another stream than the previous push's first waits for
 * that push's work.  push stages host memory through a device buffer of the handle, in bounded slices, on a stream of the handle,
 * and returns with the work queued and the caller's memory free.  read and reset synchronise, and behind either the handle refers to
 * no stream of the caller's (destroy waits for the stream of a push that nothing has waited for since).  d_raw needs frame alignment only.
 * Behind iqgpu_chain_process_device(c, .., d_out, .., &n) the spectrum of the output is
 * iqgpu_psd_push_device(p, d_out, n, iqgpu_chain_get_stream(c)). */
enum { IQGPU_PSD_RECT = 0, IQGPU_PSD_HANN = 1, IQGPU_PSD_HAMMING = 2, IQGPU_PSD_BLACKMAN_HARRIS = 3 };
typedef struct {
    uint32_t nfft;                /* 1024, 2048 or 4096 (1024) */
    uint32_t hop;                 /* frames between segment starts: nfft, nfft / 2 or nfft / 4 (nfft / 2) */
    int      window;              /* IQGPU_PSD_* (HANN) */
    float    gain;                /* applied at unpack, as iqgpu_chain_desc.gain (1) */
} iqgpu_psd_opts;
typedef struct {
    uint64_t frames, segments;    /* pushed since the last reset; segments accumulated */
    uint32_t nfft, hop;
    double   window_sum, window_sum_sq;
} iqgpu_psd_info;
typedef struct iqgpu_psd iqgpu_psd;
void  iqgpu_psd_opts_init(iqgpu_psd_opts *o);                      /* the defaults in parentheses above */
/* no device: the window table of the options (cap: room in w, in values) and its two sums; the segments of a stream of `frames` */
int   iqgpu_psd_window(const iqgpu_psd_opts *o, float *w, size_t cap, double *sum, double *sum_sq);
int   iqgpu_psd_segments(const iqgpu_psd_opts *o, uint64_t frames, uint64_t *segments);
/* diagnostics, for tests: the segments of a page -- what it takes to reach the page boundaries, nothing a caller has to know */
void  iqgpu_psd_geometry(size_t *segments_per_page);
int   iqgpu_psd_create(int device, int format, const iqgpu_psd_opts *o, iqgpu_psd **out);
void  iqgpu_psd_destroy(iqgpu_psd *p);
int   iqgpu_psd_reset(iqgpu_psd *p);
int   iqgpu_psd_push(iqgpu_psd *p, const void *raw, size_t frames);                                  /* host memory */
int   iqgpu_psd_push_device(iqgpu_psd *p, const void *d_raw, size_t frames, void *hip_stream);      /* device memory, asynchronous on hip_stream */
int   iqgpu_psd_read(iqgpu_psd *p, double *sum_power, float *peak_power, iqgpu_psd_info *info);     /* [nfft] each; synchronises */

/* ---- spectrogram: the power spectrum per time row, emitted as the stream goes by (additive, still ABI v9) ----
 * No counterpart in the reference.  iqgpu_psd answers where a signal sits; the rows of this accumulator answer when: is the carrier
 * there from the start, does it drift, is the interferer a burst.  One stream of frames in one sample format, independent of any
 * chain, with the calling convention of iqgpu_chain_process[_device]: stream-continuous, output the caller owns, a capacity check,
 * a row count back.
 * The options are iqgpu_psd_opts' (nfft, hop, window, gain: same lists, same meaning) and row_segments = R, 1 .. 2^20.
 * Segments: the power spectrum's grid.  Segment s is frames [s hop, s hop + nfft) of everything pushed since the last reset, and
 * X_s[k], p_s[k] = re^2 + im^2 in float are computed exactly as there: same unpack, gain, window table and transform.
 * Rows: row r is segments [r R, (r + 1) R): it starts at frame r R hop and spans (R - 1) hop + nfft frames;
 * rows = segments / R, rounded down.  Per finished row, [nfft] floats each, natural bin order (k = 0 is DC), nothing normalised:
 *   row_sum[r][k]  = sum over the row's segments of p_s[k], summed in double in the order below, rounded ONCE to float (nearest even)
 *   row_peak[r][k] = max over the row's segments of p_s[k], in float.
 * Summation order: it belongs to the stream, not to the calls.  A row is cut into cells of segments_per_page (iqgpu_psd_geometry: 32)
 * consecutive segments counted from the row's first segment, the last cell may be short; a cell is summed per bin in segment order
 * from 0.0 in double; the row is ((0.0 + cell 0) + cell 1) + ... in double.
 * EQUALITY WITH THE POWER SPECTRUM: row r equals, bit for bit, a fresh iqgpu_psd of the same nfft / hop / window / gain that was
 * pushed exactly the row's frames [r R hop, r R hop + (R - 1) hop + nfft): (float)sum_power[k] == row_sum[r][k] and
 * peak_power[k] == row_peak[r][k].  (That accumulator's pages are this row's cells.)
 * The open row: the segments behind the last finished row stay on the device.  iqgpu_sgram_read_open returns them as sum_power
 * (double, not rounded) and peak_power with info.open_segments = segments % R -- equal, bit for bit, to iqgpu_psd_read of a fresh
 * iqgpu_psd pushed the frames of those segments, all zero when open_segments == 0 -- so a caller can flush the ragged end of a stream.
 * It observes and does not disturb.
 * ROWS AND OPEN ROW ARE A FUNCTION OF THE PUSHED FRAMES AND THE OPTIONS ALONE, BIT FOR BIT: any split of the stream into push calls,
 * host or device, of any lengths (one frame; no multiple of hop; ending inside a cell or on a row boundary) gives the same rows in
 * the same order -- the rows each call returned, concatenated -- and the same open row.
 * push / push_device: row_sum and row_peak receive the rows the call finishes, [rows][nfft] floats densely packed, in host / device
 * memory; either may be NULL (that plane is not produced).  *rows (rows may be NULL) is pure arithmetic and is set when the call
 * returns, for the asynchronous push_device too; iqgpu_sgram_max_rows(p, frames) is what the NEXT push of `frames` would return,
 * exact, from the handle's position.  cap_rows (the room in each plane given, in rows) smaller than that: IQGPU_ECAPACITY before
 * anything is queued, the handle as it was, *rows = 0.
 * Errors: IQGPU_EINVAL for a NULL argument (p; raw with frames > 0; o; out; iqgpu_sgram_rows' rows), nfft / hop / window outside the
 * lists, a gain that is not finite, row_segments outside 1 .. 2^20; IQGPU_EFORMAT for an unknown format; IQGPU_ENODEV from create
 * without a usable device; IQGPU_ECAPACITY; IQGPU_ENOMEM; IQGPU_EHIP.  A refused call leaves the accumulator as it was; frames == 0
 * succeeds with *rows = 0 and changes nothing; a push that failed half way poisons the handle (IQGPU_EHIP from push / read_open)
 * until reset; one thread per handle.  Non-finite input frames propagate as documented for the power spectrum: by IEEE rules into
 * the row_sum bins of the rows of their segments, row_peak of those rows unspecified, other rows unaffected.
 * Streams: as for iqgpu_psd_push_device.  push_device is asynchronous on the stream it is given (NULL: the null stream); input and
 * output planes must stay valid until that stream has passed the work; a push on another stream than the previous push's first waits
 * for that push's work.  push stages host memory through device buffers of the handle, in bounded slices, on a stream of the handle,
 * and returns with the caller's input free and the rows in host memory.  read_open and reset synchronise, and behind either the
 * handle refers to no stream of the caller's; destroy waits for the stream of a push that nothing has waited for since.
 * Behind iqgpu_chain_process_device(c, .., d_out, .., &n) the rows of the output are
 * iqgpu_sgram_push_device(p, d_out, n, d_rows, NULL, cap, &rows, iqgpu_chain_get_stream(c)). */
typedef struct {
    uint32_t nfft;                /* 1024, 2048 or 4096 (1024) */
    uint32_t hop;                 /* frames between segment starts: nfft, nfft / 2 or nfft / 4 (nfft / 2) */
    int      window;              /* IQGPU_PSD_* (HANN) */
    float    gain;                /* applied at unpack, as iqgpu_chain_desc.gain (1) */
    uint32_t row_segments;        /* R: segments summed into one row, 1 .. 2^20 (32) */
} iqgpu_sgram_opts;
typedef struct {
    uint64_t frames, segments, rows;      /* pushed since the last reset; whole segments of them; rows finished = segments / R */
    uint32_t open_segments;               /* segments of the open row = segments % R */
    uint32_t nfft, hop, row_segments;
    double   window_sum, window_sum_sq;   /* as in iqgpu_psd_info */
} iqgpu_sgram_info;
typedef struct iqgpu_sgram iqgpu_sgram;
void   iqgpu_sgram_opts_init(iqgpu_sgram_opts *o);                  /* the defaults in parentheses above */
/* no device: the rows a stream of `frames` frames finishes */
int    iqgpu_sgram_rows(const iqgpu_sgram_opts *o, uint64_t frames, uint64_t *rows);
int    iqgpu_sgram_create(int device, int format, const iqgpu_sgram_opts *o, iqgpu_sgram **out);
void   iqgpu_sgram_destroy(iqgpu_sgram *p);
int    iqgpu_sgram_reset(iqgpu_sgram *p);
size_t iqgpu_sgram_max_rows(const iqgpu_sgram *p, size_t frames);   /* rows the NEXT push of `frames` finishes: exact; 0 for a NULL handle */
int    iqgpu_sgram_push(iqgpu_sgram *p, const void *raw, size_t frames, float *row_sum, float *row_peak, size_t cap_rows, size_t *rows);   /* host memory */
int    iqgpu_sgram_push_device(iqgpu_sgram *p, const void *d_raw, size_t frames, float *d_row_sum, float *d_row_peak, size_t cap_rows,
                               size_t *rows, void *hip_stream);     /* device memory, asynchronous on hip_stream */
int    iqgpu_sgram_read_open(iqgpu_sgram *p, double *sum_power, float *peak_power, iqgpu_sgram_info *info);   /* [nfft] each, either may be NULL; synchronises */

/* ---- capture statistics: counts, extrema, an amplitude histogram and the first two moments of a stream, accumulated on the device
 * (additive, still ABI v9) ----
 * No counterpart in the reference.  iqgpu_psd says where a signal sits and iqgpu_sgram when; this accumulator answers what a user asks
 * before building a chain at all: is the capture clipping, how many ADC bits does it use, how large is the DC offset, what gain
 * brings it to a sensible level, do I and Q carry the same power.  One stream of frames in one sample format, independent of any
 * chain; it serves a raw capture and a chain's output bytes alike (rail counts behind the integer pack, level behind the AGC).
 * There is NO gain: the result describes the bytes as they are, x = the library's unpack (the expressions of
 * iqgpu_convert_block_to_cf32) at gain 1.  A caller scales sum by g and sum_sq / sum_iq / peak_power by g^2 itself.
 * THE CONTRACT, per component c (0 = I, 1 = Q) of every frame, `code` the integer in the file (little endian; cs24 sign-extended):
 *   hist[c][bin]: the bin comes from INTEGER arithmetic on the code, never from the rounded float (cs32 codes k 2^24 - 1 round up to
 *   the next bin's edge in float).  Shifts of signed codes are arithmetic.
 *     cu8   code                  cs8     code + 128                        cu16  code >> 8           cs16  (code >> 8) + 128
 *     cs24  (code >> 16) + 128    sc16q11 clamp((code >> 4) + 128, 0, 255)  cu32  code >> 24          cs32  (code >> 24) + 128
 *     cf32  clamp(floor(v * 128) + 128, 0, 255) on the finite value v (v * 128 is exact in float; the clamp is taken first)
 *   rail_lo[c] / rail_hi[c]: components EQUAL to the format's lowest / highest code (cu8 0 / 255, cs8 -128 / 127, cu16 0 / 65535,
 *   cs16 -32768 / 32767, cs24 -2^23 / 2^23 - 1, cu32 0 / 2^32 - 1, cs32 -2^31 / 2^31 - 1); sc16q11: code <= -2048 / code >= 2047;
 *   cf32: v <= -1.0 / v >= 1.0.
 *   nonfinite_frames: cf32 only, frames with a NaN or Inf component.  They are counted (in frames too, and they keep their stream
 *   index) and enter NOTHING else, so one bad frame does not erase a report.  Below, "frame" means a finite one.
 *   min[c] / max[c]: of x, in float.  peak_power = max over frames of (double)re * re + (double)im * im -- both products are exact in
 *   double, the sum is rounded once; peak_frame = the stream index (frames since the last reset, from 0) of the FIRST frame that
 *   attains it.  With no finite frame min, max and peak_power are 0 and peak_frame is 0.
 *   sum[c] = sum of (double)x, sum_sq[c] = sum of (double)x * x, sum_iq = sum of (double)re * im: every term is exact in double, the
 *   additions round, in the order below.
 * ORDER-FREE FIELDS: the counts, the histogram, min / max, peak_power and peak_frame do not depend on any summation order: they are
 * exact.  THE FIVE DOUBLE SUMS: their order belongs to the stream, as in iqgpu_psd.  Frames (non-finite ones included: they hold their
 * place and add nothing) are grouped by stream index into pages of frames_per_page (iqgpu_stats_geometry: 65536) consecutive frames.
 * Within a page, frame i (its index in the page) belongs to column i mod 1024; a column is summed in increasing i from 0.0; when the
 * page closes the 1024 column sums are added in a fixed binary tree of adjacent pairs: level 0 adds columns (2 j, 2 j + 1), level 1
 * those sums pairwise again, ... ten levels.  The total is ((0.0 + page 0) + page 1) + ... in page order.  The open page (the one the
 * stream position lies in) is kept apart as its 1024 column sums and continued by the next push; read reports total + tree(open
 * columns) (total alone when the position is on a page boundary).
 * THE RESULT IS A FUNCTION OF THE PUSHED FRAMES ALONE, BIT FOR BIT: any split of the stream into push calls, host or device, of any
 * lengths (one frame; across a page boundary) and at any frame alignment gives the same iqgpu_stats_result.
 * Errors, streams, alignment: iqgpu_psd's.  IQGPU_EINVAL for a NULL argument; IQGPU_EFORMAT for an unknown format; IQGPU_ENODEV from
 * create without a usable device; IQGPU_ENOMEM; IQGPU_EHIP.  A refused call leaves the accumulator as it was; frames == 0 succeeds and
 * changes nothing; a push that failed half way poisons the handle (IQGPU_EHIP from push / read) until reset; one thread per handle.
 * push_device is asynchronous on the stream it is given (NULL: the null stream) and the input must stay valid until that stream has
 * passed the work; a push on another stream than the previous push's first waits for that push's work.  push stages host memory
 * through a device buffer of the handle, in bounded slices, on a stream of the handle, and returns with the work queued and the
 * caller's memory free.  read and reset synchronise, and behind either the handle refers to no stream of the caller's; read observes
 * and does not disturb.  d_raw needs frame alignment only (the frame's size; cs24: 2 bytes).
 * Behind iqgpu_chain_process_device(c, .., d_out, .., &n) the statistics of the output are
 * iqgpu_stats_push_device(p, d_out, n, iqgpu_chain_get_stream(c)).
 * iqgpu_stats_merge (host only, no device) CONCATENATES: `next` is the result of the stream directly behind `into`'s.  frames,
 * nonfinite_frames, the rails and the histogram add; min / max combine; the larger peak_power wins and on a tie the earlier frame
 * (into's); next->peak_frame is offset by into->frames; a side without finite frames is the identity for min / max / peak; the five
 * doubles add (into + next).  ALL INTEGER, EXTREMUM AND PEAK FIELDS OF A MERGE EQUAL THE SINGLE STREAM'S EXACTLY, for any cuts and any
 * grouping.  The five doubles of a merge are a sum of per-shard sums and, as for the power spectrum, are NOT promised bit-equal to
 * the single stream's.
 * iqgpu_stats_derive (host only), every figure in double in this operation order; a figure whose n or denominator is 0 (or whose
 * logarithm / root would not be real) is 0:
 *   n = frames - nonfinite_frames;  mean_i = sum[0] / n;  mean_q = sum[1] / n;  power = (sum_sq[0] + sum_sq[1]) / n;
 *   rms_dbfs = 10 log10(power);  peak_dbfs = 10 log10(peak_power);  crest_db = peak_dbfs - rms_dbfs (0 unless power and peak_power > 0);
 *   var_i = sum_sq[0] / n - mean_i * mean_i;  var_q = sum_sq[1] / n - mean_q * mean_q;
 *   iq_gain_ratio = sqrt(var_i / var_q) (var_q > 0, var_i >= 0);
 *   iq_phase_rad = asin(r), r = (sum_iq / n - mean_i * mean_q) / sqrt(var_i * var_q) clamped to [-1, 1] (var_i > 0 and var_q > 0);
 *   clip_fraction = (double)(rail_lo[0] + rail_lo[1] + rail_hi[0] + rail_hi[1]) / (2.0 * n);
 *   bins_used[c] = the non-empty bins of hist[c]. */
typedef struct {
    uint64_t frames;              /* pushed since the last reset */
    uint64_t nonfinite_frames;    /* cf32 only: frames with a NaN or Inf component; they enter NOTHING below */
    uint64_t rail_lo[2], rail_hi[2];   /* [0] = I, [1] = Q: components on the format's lowest / highest code */
    uint64_t hist[2][256];        /* amplitude histogram per component */
    float    min[2], max[2];      /* of the unpacked component at gain 1 */
    double   peak_power;          /* max over frames of (double)re*re + (double)im*im, sum rounded once */
    uint64_t peak_frame;          /* stream index of the FIRST frame that attains it */
    double   sum[2], sum_sq[2], sum_iq;   /* of (double)x, (double)x*x, (double)re*im: exact terms, order above */
} iqgpu_stats_result;
typedef struct {
    uint64_t n;                   /* finite frames */
    double   mean_i, mean_q, power, rms_dbfs, peak_dbfs, crest_db, var_i, var_q, iq_gain_ratio, iq_phase_rad, clip_fraction;
    uint32_t bins_used[2];
} iqgpu_stats_derived;
typedef struct iqgpu_stats iqgpu_stats;
/* diagnostics, for tests: the frames of a page -- what it takes to reach the page boundaries, nothing a caller has to know */
void  iqgpu_stats_geometry(size_t *frames_per_page);
int   iqgpu_stats_create(int device, int format, iqgpu_stats **out);
void  iqgpu_stats_destroy(iqgpu_stats *p);
int   iqgpu_stats_reset(iqgpu_stats *p);
int   iqgpu_stats_push(iqgpu_stats *p, const void *raw, size_t frames);                             /* host memory */
int   iqgpu_stats_push_device(iqgpu_stats *p, const void *d_raw, size_t frames, void *hip_stream);  /* device memory, asynchronous on hip_stream */
int   iqgpu_stats_read(iqgpu_stats *p, iqgpu_stats_result *r);                                      /* synchronises; observes, does not disturb */
/* host only, no device */
int   iqgpu_stats_merge(iqgpu_stats_result *into, const iqgpu_stats_result *next);   /* `next` is the stream directly behind `into` */
int   iqgpu_stats_derive(const iqgpu_stats_result *r, iqgpu_stats_derived *d);

/* ---- envelope: power, peak and rail count per block of B consecutive frames, emitted as the stream goes by (additive, still ABI v9) ----
 * No counterpart in the reference.  The cheap time axis of the family: where does the transmission begin and end, where are the
 * dropouts, where does it clip, does the output AGC pump.  One stream of frames in one sample format, independent of any chain, with
 * iqgpu_sgram's calling convention.  There is NO gain: like iqgpu_stats it describes the bytes, x = the library's unpack (the
 * expressions of iqgpu_convert_block_to_cf32) at gain 1.  The only option is block_frames = B, a power of two, 2^6 .. 2^24.
 * Rows: row r is frames [r B, (r + 1) B) of everything pushed since the last reset; rows = frames / B, rounded down; the rest is the
 * open row.
 * Per frame: p = (double)re * re + (double)im * im -- both products exact in double, the sum rounded once: iqgpu_stats' peak_power
 * term.  A cf32 frame with a NaN or Inf component holds its place, enters nothing below and is counted in info.nonfinite_frames.
 * Per finished row, densely packed, one value each:
 *   row_sum[r]  (float)  the sum of p over the row's frames, in double in the order below, rounded ONCE to float (nearest even).  Not
 *                        normalised: the mean power is row_sum / B.
 *   row_peak[r] (float)  the max of p over the row's frames, rounded once to float; 0 without a finite frame.
 *   row_rail[r] (uint32) the COMPONENTS of the row on a rail, by iqgpu_stats' rail_lo / rail_hi definition per format, 0 .. 2 B.
 * Summation order: it belongs to the stream, and it is iqgpu_stats' order applied per row.  A row is cut into cells of 65536
 * consecutive frames counted from the row's first frame (B <= 65536: one cell of B frames).  Within a cell, frame i (its index in the
 * cell) belongs to column i mod 1024; a column is summed in increasing i from 0.0; the 1024 column sums are added in the fixed tree of
 * adjacent pairs, ten levels (B <= 1024: the balanced adjacent-pair tree over the row's B terms, empty columns being +0.0); the row
 * is ((0.0 + cell 0) + cell 1) + ... in double.
 * ROWS AND OPEN ROW ARE A FUNCTION OF THE PUSHED FRAMES AND B ALONE, BIT FOR BIT: any split of the stream into push calls, host or
 * device, of any lengths (one frame; ending inside a row, on a row boundary, inside a cell) at frame alignment only (the frame's
 * size; cs24: 2 bytes) gives the same rows in the same order -- the rows each call returned, concatenated -- and the same open row.
 * With iqgpu_stats on the same bytes, for a stream of whole rows, exactly: (float)peak_power == max over r of row_peak[r], and
 * rail_lo[0] + rail_lo[1] + rail_hi[0] + rail_hi[1] == the sum of row_rail.
 * The open row: iqgpu_env_read_open returns its unrounded double sum (the total of its closed cells + tree(open columns)), its peak
 * in double and its rail count, all 0 when info.open_frames == 0.  It observes and does not disturb.
 * push / push_device: row_sum, row_peak and row_rail receive the rows the call finishes in host / device memory; any may be NULL (that
 * plane is not produced).  *rows (rows may be NULL) is pure arithmetic and is set when the call returns, for the asynchronous
 * push_device too; iqgpu_env_max_rows(p, frames) is what the NEXT push of `frames` would return, exact.  cap_rows (the room in each
 * plane given, in rows) smaller than that: IQGPU_ECAPACITY before anything is queued, the handle as it was, *rows = 0.
 * Errors, streams, poisoning, frames == 0, one thread per handle: iqgpu_sgram's, word for word (IQGPU_EINVAL for a NULL argument or a
 * block_frames outside the list).  Behind iqgpu_chain_process_device(c, .., d_out, .., &n) the rows of the output are
 * iqgpu_env_push_device(p, d_out, n, d_sum, d_peak, d_rail, cap, &rows, iqgpu_chain_get_stream(c)).
 * THE BURST FINDER (host only, no device) turns finished rows into ranges for iqgpu_chain_seek and the harness's range modes.  The
 * mean of a row is (double)row_sum[r] / B; thresholds `on` and `off` (off <= on) are on the mean, compared in double.
 *   A burst opens at the first row whose mean is >= on.  It closes in front of the first run of MORE than hang_rows consecutive rows
 *   whose mean is < off (a NaN mean counts as below off); shorter dips stay inside, and without such a run it lasts to the last row.
 *   A burst of fewer than min_rows rows is dropped.  The rest are widened by pad_rows rows on both sides, clipped to the stream, and
 *   bursts that then touch or overlap are joined.  first_frame and frames are multiples of B; peak_row is the first row of the
 *   (widened, joined) burst with the largest mean, peak_mean that mean.
 *   More bursts than cap: IQGPU_ECAPACITY with *n = the number needed (the first cap are written).
 * iqgpu_env_floor: the mean power of the row at rank floor(fraction (rows - 1)) of the ascending order of row_sum (NaN last), selected
 * exactly on a copy; fraction in [0, 1], rows >= 1.  What a caller derives on / off from: floor * 10^(dB / 10). */
typedef struct {
    uint32_t block_frames;        /* B: frames of a row, a power of two, 64 .. 2^24 (4096) */
} iqgpu_env_opts;
typedef struct {
    uint64_t frames, rows;        /* pushed since the last reset; rows finished = frames / B */
    uint64_t nonfinite_frames;    /* cf32 only: frames with a NaN or Inf component */
    uint32_t open_frames;         /* frames of the open row = frames % B */
    uint32_t block_frames;
} iqgpu_env_info;
typedef struct {
    uint32_t block_frames;        /* B of the rows */
    uint32_t min_rows, hang_rows, pad_rows;
    double   on, off;             /* thresholds on the mean power row_sum / B, off <= on */
} iqgpu_env_burst_opts;
typedef struct {
    uint64_t first_frame, frames; /* multiples of B */
    uint64_t peak_row;            /* the first row of the burst with the largest mean */
    double   peak_mean;
} iqgpu_env_burst;
typedef struct iqgpu_env iqgpu_env;
void   iqgpu_env_opts_init(iqgpu_env_opts *o);                      /* the default in parentheses above */
/* no device: the rows a stream of `frames` frames finishes */
int    iqgpu_env_rows(const iqgpu_env_opts *o, uint64_t frames, uint64_t *rows);
int    iqgpu_env_create(int device, int format, const iqgpu_env_opts *o, iqgpu_env **out);
void   iqgpu_env_destroy(iqgpu_env *p);
int    iqgpu_env_reset(iqgpu_env *p);
size_t iqgpu_env_max_rows(const iqgpu_env *p, size_t frames);       /* rows the NEXT push of `frames` finishes: exact; 0 for a NULL handle */
int    iqgpu_env_push(iqgpu_env *p, const void *raw, size_t frames, float *row_sum, float *row_peak, uint32_t *row_rail, size_t cap_rows,
                      size_t *rows);                                /* host memory */
int    iqgpu_env_push_device(iqgpu_env *p, const void *d_raw, size_t frames, float *d_row_sum, float *d_row_peak, uint32_t *d_row_rail,
                             size_t cap_rows, size_t *rows, void *hip_stream);   /* device memory, asynchronous on hip_stream */
int    iqgpu_env_read_open(iqgpu_env *p, double *sum, double *peak, uint32_t *rail, iqgpu_env_info *info);   /* any may be NULL; synchronises */
/* host only, no device */
int    iqgpu_env_bursts(const float *row_sum, size_t rows, const iqgpu_env_burst_opts *o, iqgpu_env_burst *out, size_t cap, size_t *n);
int    iqgpu_env_floor(const float *row_sum, size_t rows, uint32_t block_frames, double fraction, double *mean_power);

/* ---- lag products: R_d = sum of x[n] conj(x[n - d]) per block of B consecutive frames, emitted as the stream goes by (additive, still ABI v9) ----
 * No counterpart in the reference.  The cheap frequency axis of the family: arg R_1 / (2 pi) * fs is the classical coarse frequency
 * estimate of what a row holds, |R_d| / R_0 the coherence at lag d (the cyclic-prefix test of an OFDM stream: NRSC-5 repeats at lag
 * 2048 at 744 187.5 Hz) -- at the cost of reading the bytes once, no transform.  One stream of frames in one sample format,
 * independent of any chain, with iqgpu_env's calling convention.  There is NO gain: x = the library's unpack at gain 1, exactly as
 * iqgpu_env / iqgpu_stats.  Options: block_frames = B as iqgpu_env's, and 1 .. 4 strictly increasing lags, each 1 .. 65536.
 * Rows: iqgpu_env's.  Row r is frames [r B, (r + 1) B) of everything pushed since the last reset; the rest is the open row.
 * The lag term of frame n (its stream index since the last reset) and lag d exists for n >= d when both x[n] = a and x[n - d] = b are
 * finite:  re = (double)a.re * b.re + (double)a.im * b.im,  im = (double)a.im * b.re - (double)a.re * b.im  -- every product exact in
 * double, each sum or difference rounded once.  The term belongs to frame n: to its row, its cell and its column.  A frame with
 * n < d, or a pair with a non-finite member (cf32 only), contributes nothing to that lag: its column sum stays as it was (an absent
 * term is an absent addend, not a +0.0).  info.nonfinite_frames counts frames, as iqgpu_env's.  With this sign a tone at +f gives
 * arg R_d = +2 pi f d / fs.
 * Per finished row, densely packed:
 *   row_lag[r][l][2] (float)  re, im of lag l: the double sum of the row's terms in the order below, rounded ONCE to float.
 *   row_sum[r]       (float)  iqgpu_env's row_sum: the same per-frame term p, the same order; BIT-EQUAL to iqgpu_env's row_sum on the
 *                             same bytes and B.  It is R_0 of the row.
 * Summation order: iqgpu_env's (hence iqgpu_stats'), applied independently to each of the 2 n_lags + 1 components: cells of 65536
 * frames counted from the row's first frame; frame i of a cell in column i mod 1024; a column summed in increasing i from 0.0; the
 * ten-level tree of adjacent pairs over the columns (B <= 1024: the balanced pair tree over the row's B columns); the row is
 * ((0.0 + cell 0) + cell 1) + ... in double.
 * History: the partner of a frame may lie in an earlier push, an earlier row or an earlier launch.  The handle carries the last
 * lags[n_lags - 1] frames of the stream on the device; iqgpu_lag_reset empties that history with everything else.
 * ROWS AND OPEN ROW ARE A FUNCTION OF THE PUSHED FRAMES AND THE OPTIONS ALONE, BIT FOR BIT: any split of the stream into push calls,
 * host or device, of any lengths (one frame; shorter than the largest lag; ending inside a row or a cell) at frame alignment only
 * gives the same rows in the same order and the same open row.
 * The open row: iqgpu_lag_read_open returns the unrounded doubles of the open row -- lag[n_lags][2] and sum, each the total of its
 * closed cells + tree(open columns) -- all 0 when info.open_frames == 0.  It observes and does not disturb.
 * push / push_device, *rows, iqgpu_lag_max_rows, cap_rows and IQGPU_ECAPACITY, streams, poisoning, frames == 0, one thread per handle
 * and the error codes: iqgpu_env's, word for word; either plane may be NULL.  IQGPU_EINVAL also for n_lags outside 1 .. 4, a lag
 * outside 1 .. 65536 and lags that are not strictly increasing.  Behind iqgpu_chain_process_device(c, .., d_out, .., &n) the rows of
 * the output are iqgpu_lag_push_device(p, d_out, n, d_lag, d_sum, cap, &rows, iqgpu_chain_get_stream(c)).
 * Cost: a lag of at most 1024 frames takes its partner from on chip; a farther one loads the stream a second time (profiles/lag.md).
 * THE ESTIMATE (host only, no device).  iqgpu_lag_freq: hz = atan2(im, re) / (2 pi lag) * sample_rate in double, in that order of
 * operations; 0 when re == im == 0; IQGPU_EINVAL for a non-finite value, lag == 0 or sample_rate <= 0.
 * iqgpu_lag_estimate_rows adds (double)row_lag[r][lag_index][..] and (double)row_sum[r] over rows first_row .. first_row + n_rows - 1
 * (inside the `rows` given, else IQGPU_EINVAL) in increasing order from 0.0, skipping a row in which one of these three values is a
 * NaN; hz = iqgpu_lag_freq of the sums; coherence = hypot(re, im) / power, 0 unless power > 0; span_hz = sample_rate / lag, the width
 * of the unambiguous interval (-span_hz / 2, +span_hz / 2]: a frequency outside it comes back moved by a multiple of span_hz.
 * row_sum == NULL: power = coherence = 0.  An iqgpu_env_burst maps to first_row = first_frame / B, n_rows = frames / B.
 * THE SIGN: the chain's NCO multiplies by exp(+j theta) for shift_hz >= 0 (it mixes UP by shift_hz), so a burst estimated at hz is
 * centred by a chain description with shift_hz = -hz. */
typedef struct {
    uint32_t block_frames;        /* B: frames of a row, a power of two, 64 .. 2^24 (4096) */
    uint32_t n_lags;              /* 1 .. 4 (1) */
    uint32_t lags[4];             /* strictly increasing, each 1 .. 65536 ({1}) */
} iqgpu_lag_opts;
typedef struct {
    uint64_t frames, rows;        /* pushed since the last reset; rows finished = frames / B */
    uint64_t nonfinite_frames;    /* cf32 only: frames with a NaN or Inf component */
    uint32_t open_frames;         /* frames of the open row = frames % B */
    uint32_t block_frames, n_lags, lags[4];
} iqgpu_lag_info;
typedef struct {
    double re, im, power;         /* the sums over the rows */
    double hz, coherence, span_hz;
} iqgpu_lag_estimate;
typedef struct iqgpu_lag iqgpu_lag;
void   iqgpu_lag_opts_init(iqgpu_lag_opts *o);                      /* the defaults in parentheses above */
/* no device: the rows a stream of `frames` frames finishes */
int    iqgpu_lag_rows(const iqgpu_lag_opts *o, uint64_t frames, uint64_t *rows);
int    iqgpu_lag_create(int device, int format, const iqgpu_lag_opts *o, iqgpu_lag **out);
void   iqgpu_lag_destroy(iqgpu_lag *p);
int    iqgpu_lag_reset(iqgpu_lag *p);
size_t iqgpu_lag_max_rows(const iqgpu_lag *p, size_t frames);       /* rows the NEXT push of `frames` finishes: exact; 0 for a NULL handle */
int    iqgpu_lag_push(iqgpu_lag *p, const void *raw, size_t frames, float *row_lag, float *row_sum, size_t cap_rows, size_t *rows);   /* host memory */
int    iqgpu_lag_push_device(iqgpu_lag *p, const void *d_raw, size_t frames, float *d_row_lag, float *d_row_sum, size_t cap_rows,
                             size_t *rows, void *hip_stream);      /* device memory, asynchronous on hip_stream */
int    iqgpu_lag_read_open(iqgpu_lag *p, double *lag /* [n_lags][2] */, double *sum, iqgpu_lag_info *info);   /* any may be NULL; synchronises */
/* host only, no device */
int    iqgpu_lag_freq(double re, double im, uint32_t lag, double sample_rate, double *hz);
int    iqgpu_lag_estimate_rows(const float *row_lag, const float *row_sum, size_t rows, const iqgpu_lag_opts *o, uint32_t lag_index,
                               size_t first_row, size_t n_rows, double sample_rate, iqgpu_lag_estimate *out);

/* ---- template correlation: the matched filter of up to eight known waveforms per block of B start positions, emitted as the stream
 * goes by (additive, still ABI v9) ----
 * No counterpart in the reference.  iqgpu_env finds power to within a block and not below the noise floor, iqgpu_lag finds
 * periodicity, not position; this accumulator answers AT WHICH FRAME a waveform the caller knows starts -- a preamble, a sync word, a
 * chirp, a pilot symbol, a PN code -- and, with a small bank of frequency-shifted copies (iqgpu_match_shift_bank), the coarse offset
 * of a burst too short for iqgpu_lag.  One stream of frames in one sample format, independent of any chain, with iqgpu_sgram's
 * calling convention.  There is NO gain and NO window: x = the library's unpack at gain 1, exactly as iqgpu_stats / _env / _lag.
 * Options: nfft 1024, 2048 or 4096, 0 = the smallest of the three with nfft / 2 + 1 >= template_frames (info.nfft reports it);
 * block_frames = B, a power of two, nfft / 2 .. 2^24; n_templates 1 .. 8; template_frames = L, 2 .. nfft / 2 + 1.
 * Templates: n_templates * L cf32 frames in host memory, template t at templates[2 t L ..), read by iqgpu_match_create only; every
 * value finite, every template with energy above zero.  info.template_energy[t] = sum |h_t[k]|^2 in double.
 * Correlation: c_t[n] = sum over k < L of x[n + k] conj(h_t[k]) for start position n (a stream index since the last reset),
 * p_t[n] = re^2 + im^2 in float.  It is computed by overlap-save: with V = nfft / 2, segment s is frames [s V, s V + nfft) -- the power
 * spectrum's grid at hop = nfft / 2, the same count, the same carry -- and yields p_t[n] for n in [s V, (s + 1) V) as points 0 .. V - 1
 * of IFFT(X_s G_t), X_s the float transform of the segment and G_t = conj(FFT_nfft(h_t zero-padded)) / nfft evaluated once on the host
 * in double and rounded to float; L - 1 <= V keeps those points free of wrap-around.  START POSITIONS IN THE LAST nfft - V FRAMES OF
 * A STREAM BELONG TO NO WHOLE SEGMENT AND ARE NOT REPORTED: a stream of F frames reports positions 0 .. segments * V - 1,
 * segments = (F - nfft) / V + 1.  Pad the end of a capture with nfft / 2 frames of zeros to have every whole match reported.
 * Rows: row r is start positions [r B, (r + 1) B), that is B / V consecutive segments; rows = segments / (B / V), rounded down.
 * Per finished row, [n_templates] values each, densely packed:
 *   row_peak[r][t] (float)   the largest p_t[n] of the row
 *   row_at[r][t]   (uint32)  n - r B of the LOWEST n that attains it (an all-zero row: 0)
 *   row_sum[r][t]  (float)   sum of p_t[n] over the row, summed in double in the order below, rounded ONCE to float.
 * Summation order: it belongs to the stream, not to the calls.  Within a segment one fixed tree: thread j of nfft / 16 holds points
 * j + i nfft / 16, i = 0 .. 7, and adds them in increasing i from 0.0; the 64 threads of a wave are combined in six levels of pairs 1, 2,
 * 4, 8, 16 and 32 threads apart; the nfft / 1024 waves are added in wave order.  The row is ((0.0 + segment 0) + segment 1) + ... in
 * double.  The peak follows the same walk; a value replaces the held one only where it is greater, or equal at a lower n.
 * The open row: iqgpu_match_read_open returns sum (double, not rounded), peak and at, [n_templates] each, of the segments behind the
 * last finished row, all 0 when info.open_segments == 0.  It observes and does not disturb.
 * ROWS AND OPEN ROW ARE A FUNCTION OF THE PUSHED FRAMES AND THE OPTIONS ALONE, BIT FOR BIT: any split of the stream into push calls,
 * host or device, of any lengths (one frame; no multiple of V; ending inside a row) at frame alignment only gives the same rows in
 * the same order and the same open row.
 * push / push_device, *rows, iqgpu_match_max_rows, cap_rows (checked when any plane is given) and IQGPU_ECAPACITY, streams, poisoning,
 * frames == 0, one thread per handle and the error codes: iqgpu_sgram's, word for word; any plane may be NULL.  IQGPU_EINVAL also for
 * options outside the lists above, a template value that is not finite and a template without energy.  Non-finite cf32 input
 * propagates by IEEE rules into row_sum of the rows of its segments, as documented for the power spectrum; row_peak and row_at of
 * those rows are unspecified; other rows are unaffected.  Behind iqgpu_chain_process_device(c, .., d_out, .., &n) the rows of the
 * output are iqgpu_match_push_device(p, d_out, n, d_peak, d_at, d_sum, cap, &rows, iqgpu_chain_get_stream(c)).
 * Cost: per input frame 2 (1 + n_templates) transform points where iqgpu_psd at hop = nfft / 2 spends 2 (profiles/match.md).
 * THE BANK (host only, no device).  iqgpu_match_shift_bank: out[i][k] = tmpl[k] exp(+j 2 pi hz[i] k / sample_rate), evaluated in
 * double and rounded to float, n members of L frames.  A burst received hz[i] off centre correlates with member i; it is centred by
 * a chain with shift_hz = -hz[i] (the sign rule of iqgpu_lag_freq).
 * THE DETECTIONS (host only, no device).  iqgpu_match_peaks walks rows by row, then template: (r, t) is a detection when
 * row_peak > 0 and row_peak >= ratio * (row_sum - row_peak) / (B - 1), in double -- the peak against the mean of the row's other
 * positions.  Each is {first_frame = r B + row_at, template_index, peak, ratio = row_peak / that mean, +inf where the mean is 0}.
 * *n is the count found; cap smaller than that: the first cap are written and the call returns IQGPU_ECAPACITY.  A NaN row is none.
 * Normalised correlation is the caller's: p_t[n] / (template_energy[t] * the power of x over [n, n + L)), from iqgpu_env's rows. */
typedef struct {
    uint32_t nfft;                /* 0, 1024, 2048 or 4096 (0: the smallest that holds the template) */
    uint32_t block_frames;        /* B: start positions of a row, a power of two, nfft / 2 .. 2^24 (4096) */
    uint32_t n_templates;         /* 1 .. 8 (1) */
    uint32_t template_frames;     /* L: 2 .. nfft / 2 + 1 (0: the caller sets it) */
} iqgpu_match_opts;
typedef struct {
    uint64_t frames, segments, rows;      /* pushed since the last reset; whole segments of them; rows finished = segments / (B / V) */
    uint32_t open_segments;               /* segments of the open row = segments % (B / V) */
    uint32_t nfft, block_frames, n_templates, template_frames, reserved;
    double   template_energy[8];
} iqgpu_match_info;
typedef struct {
    uint64_t first_frame;         /* r B + row_at: the start position of the match in the stream */
    uint32_t template_index;
    float    peak;
    double   ratio;
} iqgpu_match_peak;
typedef struct iqgpu_match iqgpu_match;
void   iqgpu_match_opts_init(iqgpu_match_opts *o);                  /* the defaults in parentheses above */
/* no device: the rows a stream of `frames` frames finishes */
int    iqgpu_match_rows(const iqgpu_match_opts *o, uint64_t frames, uint64_t *rows);
int    iqgpu_match_create(int device, int format, const iqgpu_match_opts *o, const float *templates /* [n_templates][L][2] */, iqgpu_match **out);
void   iqgpu_match_destroy(iqgpu_match *p);
int    iqgpu_match_reset(iqgpu_match *p);
size_t iqgpu_match_max_rows(const iqgpu_match *p, size_t frames);   /* rows the NEXT push of `frames` finishes: exact; 0 for a NULL handle */
int    iqgpu_match_push(iqgpu_match *p, const void *raw, size_t frames, float *row_peak, uint32_t *row_at, float *row_sum, size_t cap_rows,
                        size_t *rows);                              /* host memory */
int    iqgpu_match_push_device(iqgpu_match *p, const void *d_raw, size_t frames, float *d_row_peak, uint32_t *d_row_at, float *d_row_sum,
                               size_t cap_rows, size_t *rows, void *hip_stream);     /* device memory, asynchronous on hip_stream */
int    iqgpu_match_read_open(iqgpu_match *p, double *sum, float *peak, uint32_t *at, iqgpu_match_info *info);   /* [n_templates] each, any may be NULL; synchronises */
/* host only, no device */
int    iqgpu_match_shift_bank(const float *tmpl, uint32_t template_frames, const double *hz, uint32_t n, double sample_rate, float *out);
int    iqgpu_match_peaks(const float *row_peak, const uint32_t *row_at, const float *row_sum, size_t rows, const iqgpu_match_opts *o,
                         double ratio, iqgpu_match_peak *out, size_t cap, size_t *n);

/* ---- WAV capture metadata -> frequency shift (host only): the step in front of the path for real captures ----
 * SdrMetadata and its parsers (src/input_wav.c:54-100, 146-438), the shift rule of wav_initialize (592-629). */
enum { IQGPU_SDR_UNKNOWN = 0, IQGPU_SDR_CONSOLE = 1, IQGPU_SDR_SHARP = 2, IQGPU_SDR_UNO = 3, IQGPU_SDR_CONNECT = 4 };
typedef struct {
    int     source_software;                    /* IQGPU_SDR_*                                                  */
    char    software_name[64], software_version[64], radio_model[128];
    int     software_name_present, software_version_present, radio_model_present;
    double  center_freq_hz;  int center_freq_hz_present;
    int64_t timestamp_unix;  int timestamp_unix_present;
    char    timestamp_str[64]; int timestamp_str_present;
    int     sdr_info_present;                   /* any metadata source produced something                      */
    /* what sf_open reports (SF_INFO) and the path needs */
    int32_t sample_rate, channels, bits_per_sample, format_tag;
    int     in_format;                          /* IQGPU_FMT_CS16 or IQGPU_FMT_CU8 (the two subtypes the reference accepts) */
    uint64_t data_offset, data_bytes, frames;
} iqgpu_wav_info;
void iqgpu_wav_info_init(iqgpu_wav_info *md);
/* one `auxi` chunk: SDR Console XML first, SDRuno / SDRconnect binary otherwise; 1 if anything was parsed */
int  iqgpu_wav_parse_auxi(const void *chunk, size_t size, iqgpu_wav_info *md);
/* SDR#-style base name: ..._<freq>Hz... and _YYYYMMDD_HHMMSSZ; fills only what the chunk left unset */
int  iqgpu_wav_parse_filename(const char *base_filename, iqgpu_wav_info *md);
/* header walk (RIFF / RF64: fmt, auxi, data) + both parsers; IQGPU_EFORMAT for != 2 channels or an unsupported subtype */
int  iqgpu_wav_probe(const char *path, iqgpu_wav_info *md);
/* resources->nco_shift_hz = center_freq_hz - (double)center_target (float option); IQGPU_ESHIFT when --freq-shift is also
 * given or the file has no centre frequency; 0 shift when the option is not used */
int  iqgpu_wav_shift_hz(const iqgpu_wav_info *md, float center_target_hz, float freq_shift_hz_arg, double *nco_shift_hz);

/* ---- stream / profiling plumbing ---- */
int    iqgpu_chain_set_stream(iqgpu_chain *c, void *hip_stream);   /* hipStream_t; NULL = chain's own stream */
void  *iqgpu_chain_get_stream(const iqgpu_chain *c);
int    iqgpu_chain_synchronize(iqgpu_chain *c);
int    iqgpu_chain_set_profiling(iqgpu_chain *c, int enable);      /* brackets every launch with HIP events  */
int    iqgpu_chain_get_profile(iqgpu_chain *c, iqgpu_profile *p);  /* synchronises, then reports and clears  */
/* name of the front kernel the LAST process call launched: "k_front_mid<6,nco>", "k_front_mid<6,nonco>", "k_front_mid<8,nco>" (the
 * outputs per lane of the instantiation and whether it mixes; ",cf32" = cf32 out to a filter, ",8bit" = 8-bit frames in or out,
 * ",gain" = 16-bit frames with a gain or of the sc16q11 scale), "k_front_s1", "k_front_fat", "k_front_s2", "k_cascade+k_front_s1",
 * "k_cascade2+k_front_s1", "k_front_p0", "k_p0fft16" (round 6, opt-in by iqgpu_debug_set("fuse_filter", "1"): resampler and post-resample
 * filter in one kernel, no front launch), "k_front", "k_front+k_interp"; "" before the first call.  Diagnostics, bench.py's
 * roofline.kernel */
const char *iqgpu_chain_front_kernel(const iqgpu_chain *c);

/* Diagnostic switches (ABI v6; no reference counterpart).  The library reads NO switch from the environment: kernel selection and
 * plan overrides used by the parity tests and the A/B tools go through this one entry point.  A chain takes the table as it
 * stands when iqgpu_chain_create runs, in one snapshot; later changes do not touch existing chains, and iqgpu_design_probe /
 * iqgpu_design_out_frames read the table without any effect on them.  name: "no_fast", "agc_nofuse", "force_generic",
 * "fft_log2n", ... (abi.cpp kSwitches; an unknown name is IQGPU_EINVAL); value NULL or "" clears the switch, name NULL clears all.
 * iqgpu_debug_list writes "name=value;name=value" of what is set (bench.py records it in config.debug). */
int    iqgpu_debug_set(const char *name, const char *value);
int    iqgpu_debug_list(char *buf, size_t cap);

/* diagnostic hook: copies the chain's 64 KiB scratch (per-phase cycle counters in builds
 * made with -DIQGPU_STAMPS) to the host and clears it */
int    iqgpu_chain_debug_read_scratch(iqgpu_chain *c, void *host_64k);

/* ---- operator-level entry points (same kernels, one operator enabled) ----
 * Names follow the reference functions they replace. Host buffers. */
size_t iqgpu_get_bytes_per_sample(int format);                                  /* get_bytes_per_sample, src/sample_convert.c:102 */
int    iqgpu_convert_block_to_cf32(const void *in, float *out_re_im, size_t frames,
                                   int in_format, float gain, int device);       /* convert_block_to_cf32, src/sample_convert.c:127 */
int    iqgpu_convert_cf32_to_block(const float *in_re_im, void *out, size_t frames,
                                   int out_format, int device);                  /* convert_cf32_to_block, src/sample_convert.c:213 */

/* ---- device memory helpers for hosts that have no HIP binding of their own (harness, ctypes) ---- */
int    iqgpu_device_malloc(int device, size_t bytes, void **d_ptr);
int    iqgpu_device_free(int device, void *d_ptr);
int    iqgpu_host_malloc_pinned(size_t bytes, void **h_ptr);
int    iqgpu_host_free_pinned(void *h_ptr);
int    iqgpu_memcpy_h2d(int device, void *d_dst, const void *h_src, size_t bytes);
int    iqgpu_memcpy_d2h(int device, void *h_dst, const void *d_src, size_t bytes);
int    iqgpu_memcpy_h2d_async(void *d_dst, const void *h_src, size_t bytes, void *hip_stream);
int    iqgpu_memcpy_d2h_async(void *h_dst, const void *d_src, size_t bytes, void *hip_stream);
int    iqgpu_stream_create(int device, void **hip_stream);
int    iqgpu_stream_destroy(void *hip_stream);
int    iqgpu_stream_synchronize(void *hip_stream);
int    iqgpu_event_create(void **hip_event);
int    iqgpu_event_destroy(void *hip_event);
int    iqgpu_event_record(void *hip_event, void *hip_stream);
int    iqgpu_stream_wait_event(void *hip_stream, void *hip_event);
int    iqgpu_event_elapsed_ms(void *start_event, void *stop_event, float *ms); /* synchronises on stop */

#ifdef __cplusplus
}
#endif
#endif /* IQGPU_H_ */
