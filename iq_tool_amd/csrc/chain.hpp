// chain.hpp -- internal to libiqgpu's host side: the chain object behind the opaque iqgpu_chain handle, the per-call plan and
// what the translation units of the C ABI share.  Not installed; include/iqgpu.h is the interface.
//   abi.cpp        library / lifecycle / state entry points, create-time design (design_chain)
//   plan.cpp       stream-position arithmetic (plan_call), the route of a call and its run geometry (Call::choose_route, plan_route)
//   process.cpp    one process() call: buffers, the stages in stream order, iqgpu_chain_process[_device]
//   seek.cpp       seamless range sharding: iqgpu_chain_seek[_agc | _dc], iqgpu_chain_measure, iqgpu_chain_agc_initial_state / _advance,
//                  iqgpu_chain_dc_measure / _dc_measure_range / _dc_advance, iqgpu_chain_dcagc_*, iqgpu_chain_dcrms_*
//   agc_host.cpp   host side of the output AGC: chunk map, fused / unfused split, verifier + fallback launches
//   pipeline.cpp   iqgpu_chain_submit / _measure_submit / _collect (pinned host buffers, three stages moved along by the host)
//   iq_calib.cpp   I/Q calibration: iqgpu_iq_metric_batch, iqgpu_chain_calibrate_iq (the search itself: iq_optimizer.cpp, no HIP)
//   psd.cpp        power spectrum of a stream: the iqgpu_psd accumulator (a handle of its own, independent of any chain; kernels psd.hip)
//   sgram.cpp      the power spectrum per time row: the iqgpu_sgram accumulator (around psd.cpp's stream core PsdStream; kernels sgram.hip)
//   state.cpp      checkpoint / resume: iqgpu_chain_tell, iqgpu_chain_save_state / _load_state, iqgpu_design_state_size (the blob's
//                  header, checksum and iqgpu_state_inspect: state_blob.cpp, which includes nothing of HIP)
#pragma once
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/iqgpu.h"
#include "design.hpp"
#include "kernels.hpp"

using namespace iqgpu;

// ---- error reporting (abi.cpp) ----
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
const char *last_error_text();
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail(IQGPU_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

inline double monotonic_sec() // get_monotonic_time_sec, src/utils.c
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

inline size_t bytes_per_frame(int fmt) { return (size_t)frame_bytes(fmt); }   // (kernels.hpp; size_t for the buffer arithmetic of the call sites)

// ---- diagnostic switches (iqgpu_debug_set; parse rules: abi.cpp kSwitches): one chain's snapshot, with the defaults ----
struct DebugSwitches {
    bool force_generic = false;   // "force_generic": always use the workgroup-tiled k_front
    uint32_t dbg = 0;             // kDbg* kernel-selection switches (kernels.hpp), carried in the launch arguments
    int tap_fold = -1;            // "tap_fold" 0 | 1: arm placement in the tap planes of k_front_mid / k_front_fat (-1: front_tap_fold)
    // run stealing in k_front_mid (kernels.hpp, FrontArgs::w_steal): "steal" turns it on, "steal_min" / "_rounds" / "_stride" /
    // "_lanes" tune it.  (off by default: measured neutral, profiles/r04_steal.md -- the launch tail it removes turned out to be free)
    bool steal = false; int steal_min = 6, steal_rounds = 6, steal_stride = 544, steal_lanes = 16;   // stride in 8-byte words: 4352 B
    // weights of the runs of the first / second / third wave of a SIMD in k_front_mid ("run_weights" = "a,b,c"; 0 = equal runs)
    int32_t run_wt[4] = {1300, 1000, 700, 0};
    bool nco_hold = true;         // "nco_hold" = "0": k_front_mid looks its phasors up on every tile, as before the hold
    int cus = 0;                  // "cus": plan every launch for this many CUs (applies in [8, the device's CU count]; 0 = all)
    int fft_log2n = 0;            // "fft_log2n": overlap-save transform size (applies when it holds the taps; 0 = chosen)
    int fft_threads = 0;          // "fft_threads": k_fftconv16's workgroup size (0 = chosen)
    bool fft_keep_geometry = false;   // "fft_geometry" = "keep": the two filter kernels on k_p0fft16's transform size and windows
    int measure_route = -1;       // "measure_route" = "unfused" | "s1": the route of iqgpu_chain_measure (-1: the faster one measured for the shape, measure_route() in seek.cpp)
    int casc2_min_run = 0;        // "casc2_min_run": shortest streaming run (tiles) that takes k_cascade2 (0 = the built-in bound)
    // "dc_range_slice_frames": frames per staging slice of the host variants of iqgpu_chain_*_dc_measure_range (0 = kDcRangeSliceFrames;
    // a slice is whole calls, at least one).  No part of a saved state's fingerprint: it decides no routing
    long long dc_range_slice_frames = 0;
};
DebugSwitches debug_switches();                        // abi.cpp: the table as it stands, under one lock
std::string debug_value(const char *name);             // ... one raw value ("" when unset): process-level switches only (sysfs_root)

// ------------------------------------------------------------------------------------------------
// the chain object
// ------------------------------------------------------------------------------------------------
// Owners of device resources (host only: psd.hip and sgram.hip see this header through psd.hpp and use none of it).  A member of one
// of these types is freed with the object that holds it, in reverse order of declaration: there is no list of releases to keep.  All
// are move-only -- a move leaves the source empty -- and none creates anything in a constructor.
// (IQGPU_LOCAL: the library is not built with -fvisibility=hidden, so without it every inline member of the owners would enter the
//  dynamic symbol table as a weak symbol; with it the table stays as it was)
#define IQGPU_LOCAL __attribute__((visibility("hidden")))
// a device buffer that grows on demand
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    IQGPU_LOCAL DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    IQGPU_LOCAL DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    IQGPU_LOCAL ~DevBuf() { release(); }
    int ensure(size_t bytes)
    {
        if (bytes <= cap) return IQGPU_OK;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = bytes + bytes / 8 + 256;
        if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; return fail(IQGPU_ENOMEM, "hipMalloc(%zu) failed", want); }
        cap = want;
        return IQGPU_OK;
    }
    // grow, keeping the first keep_bytes (synchronises the stream once per growth)
    int ensure_keep(size_t bytes, size_t keep_bytes, hipStream_t s)
    {
        if (bytes <= cap) return IQGPU_OK;
        DevBuf nb;
        int rc = nb.ensure(bytes); if (rc) return rc;
        if (p && keep_bytes) {
            if (hipMemcpyAsync(nb.p, p, keep_bytes, hipMemcpyDeviceToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
                return fail(IQGPU_EHIP, "device copy failed while growing a stream buffer");
        }
        *this = std::move(nb);
        return IQGPU_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// n elements of device memory, allocated once: empty, or uploaded from the host (n == 0 leaves it empty)
template <typename T> struct IQGPU_LOCAL DevMem {
    T *p = nullptr;
    DevMem() = default;
    DevMem(DevMem &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevMem &operator=(DevMem &&o) noexcept { if (this != &o) { release(); p = o.p; o.p = nullptr; } return *this; }
    ~DevMem() { release(); }
    operator T *() const { return p; }
    hipError_t alloc(size_t n)
    {
        release();
        const hipError_t e = n ? hipMalloc((void **)&p, n * sizeof(T)) : hipSuccess;
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    int upload(const T *src, size_t n)
    {
        if (alloc(n) != hipSuccess) return fail(IQGPU_ENOMEM, "hipMalloc(%zu) failed", n * sizeof(T));
        if (n) HIP_TRY(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
        return IQGPU_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
};

// n elements of pinned host memory (flags: hipHostMalloc's)
template <typename T> struct IQGPU_LOCAL HostMem {
    T *p = nullptr;
    HostMem() = default;
    HostMem(HostMem &&o) noexcept : p(o.p) { o.p = nullptr; }
    HostMem &operator=(HostMem &&o) noexcept { if (this != &o) { release(); p = o.p; o.p = nullptr; } return *this; }
    ~HostMem() { release(); }
    operator T *() const { return p; }
    hipError_t alloc(size_t n, unsigned flags)
    {
        release();
        const hipError_t e = hipHostMalloc((void **)&p, n * sizeof(T), flags);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    void release() { if (p) (void)hipHostFree((void *)p); p = nullptr; }
};

// an event and a stream.  create() on a live owner is a no-op: a lazy set-up that failed half way and runs again keeps what it has
struct IQGPU_LOCAL Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    Event &operator=(Event &&o) noexcept { if (this != &o) { release(); e = o.e; o.e = nullptr; } return *this; }
    ~Event() { release(); }
    operator hipEvent_t() const { return e; }
    hipError_t create(unsigned flags) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    void release() { if (e) (void)hipEventDestroy(e); e = nullptr; }
};
struct IQGPU_LOCAL Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream &&o) noexcept : s(o.s) { o.s = nullptr; }
    Stream &operator=(Stream &&o) noexcept { if (this != &o) { release(); s = o.s; o.s = nullptr; } return *this; }
    ~Stream() { release(); }
    operator hipStream_t() const { return s; }
    hipError_t create() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    void release() { if (s) (void)hipStreamDestroy(s); s = nullptr; }
};
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "DevBuf owns its memory");
static_assert(!std::is_copy_constructible<DevMem<float>>::value && !std::is_copy_constructible<HostMem<float>>::value, "owners do not copy");
static_assert(!std::is_copy_constructible<Event>::value && !std::is_copy_constructible<Stream>::value, "owners do not copy");

struct iqgpu_chain {
    static constexpr int kPipeSlots = 8;
    iqgpu_chain_desc desc;
    int device = 0;
    float ratio = 1.0f;
    double target_rate = 0.0;
    bool resample = false;
    bool decim = false;          // resampler fused into the front kernel (r < 1, filter after it or none)
    bool late = false;           // resampler behind the front stage / pre filter: k_interp (r >= 1)
    ResamplePlan rp;
    FilterPlan fp;
    DebugSwitches sw;            // the diagnostic switches as the table stood when the chain was designed
    // operator constants
    bool dc = false; float dc_alpha = 0.0f, dc_c = 1.0f; double dc_logc = 0.0;
    float iq_mag = 0.0f, iq_phase = 0.0f;
    int nco_mode = 0, pnco_mode = 0; uint32_t nco_dtheta = 0;
    // geometry
    int S = 0, D = 1, TG = kTile;
    int warm_tiles = 0, hist_cap = 0, tiles_per_block = 128;
    bool auto_block = true;      // block_samples == 0: size the per-wave runs from the call and the CU count
    int n_cu = 256;
    uint32_t n_est = 0;
    int lvl_off[kMaxS + 2] = {0};
    int tap_off[kMaxS] = {0};
    int n_hb_taps = 0;
    // stream position (since the last reset)
    int rem = 0;                 // samples of the open group
    uint64_t phi = 0;            // phase of the next output relative to the next group
    uint32_t nco_theta = 0;      // pre-NCO phase of the next input sample
    uint32_t pnco_theta = 0;     // post-NCO phase of the next output sample
    uint64_t fpending = 0;       // FFT-mode filter input samples not yet emitted
    // input frames consumed and output frames emitted since the last reset (a seek: since frame 0 of the stream it seeks in);
    // iqgpu_chain_tell, the header of a saved state
    uint64_t total_in = 0, total_out = 0;
    // device state
    // (own_stream in front of every buffer and event: it is destroyed behind them.  stream: the one in use, not owned -- iqgpu_chain_set_stream)
    Stream own_stream; hipStream_t stream = nullptr;
    DevMem<cf2> d_nco_tab; DevMem<float> d_arb, d_hb; DevMem<cf2> d_ftaps;
    DevMem<cf2> d_hfreq, d_twiddle; int fft_log2n = 0;   // overlap-save path of FFT-kind filters
    DevMem<cf2> d_hist[2]; int hist_cur = 0;
    // S >= 2 without a dc blocker: k_cascade (stages 0 .. S-2) -> mid -> k_front_s1 (last stage + polyphase)
    bool cascade = false; int hist2_cap = 0, casc_warm = 1;
    DevMem<cf2> d_hist2[2]; int hist2_cur = 0;
    DevBuf mid;
    DevMem<cd2> d_dc_state;
    DevMem<unsigned char> d_sink;     // diagnostic scratch of k_front_s1 (iqgpu_chain_debug_read_scratch)
    // run descriptors of k_front_mid (kernels.hpp, FrontArgs::w_steal; sw.steal*): one per wave of a launch; all exhausted between
    // launches (zeroed when the array is (re)allocated)
    DevBuf steal_buf;
    DevBuf dc_agg, dc_carry;
    // exact seamless sharding of DC-blocker chains (seek.cpp): the map of a measured call, the state and the tables of iqgpu_chain_dc_advance
    DevBuf dc_walk;
    // ... and the measure pass over a whole range (iqgpu_chain_*_dc_measure_range): the entry table and the maps of all its pieces;
    // the host variants' two staging slices, their copy stream and, per slice, "copy landed" / "kernels done" (created on first use)
    DevBuf dc_range_tab, dc_range_map, dc_range_in[2];
    Stream dc_range_h2d; Event dc_range_in_done[2], dc_range_k_done[2];
    DevBuf fbuf[2]; int fcur = 0;
    // output AGC (digital profile)
    bool agc = false; float agc_target = 0.9f; int64_t agc_chunk = 16384;
    DevMem<AgcState> d_agc_state; AgcState agc_init{};
    float agc_rms_alpha = 0.0f;     // > 0: profile dx / local (liquid agc_crcf), AgcState.gain = g, .peak_memory = y2_prime
    DevBuf abuf, agc_peak, agc_gain, agc_peak_b;
    // dx / local: the chunk grid of the parallel scheme belongs to the stream -- its position since the last reset, and the last
    // `agc_rms_warm` samples of the AGC's input (what a chunk that begins early in the next call warms up on), agc.hip
    DevBuf agc_hist; int64_t agc_rms_warm = 0; uint64_t agc_rms_pos = 0;
    // agc_peak is all zero: what a fused front launch needs (k_agc_classify hands it back zeroed, agc_peak_b too; the unfused kernels do not)
    bool agc_peak_clean = false;
    // seamless sharding of digital-AGC chains (ABI v8, seek.cpp; AgcMode): the rows of a measure pass, the tables and the scratch
    // state of iqgpu_chain_agc_advance, the scratch AGC state of the measure pass on k_front_s1
    DevBuf agc_rows, agc_walk, agc_scratch;
    // fused AGC of the locked phase (k_front_s1<.., AGC> + k_agc_verify): which chains qualify, the host's mirror of
    // "has the stream locked" (a closed form: the first chunk that starts after AGC_DIGITAL_LOCK_TIME of output), the
    // flag the verifier leaves for the fallback launches
    bool agc_fusable = false, agc_locked_host = false; uint64_t agc_seen_host = 0;
    DevMem<int32_t> d_agc_flag;
    // The verdict on the HOST (round 5).  On the paths where the host waits for a call's output anyway -- iqgpu_chain_process, and
    // submit / collect, whose host moves every batch from stage to stage -- the fallback kernels are not queued behind a fused
    // launch as four launches that normally return at once (~19 us of a 400 us step): k_agc_classify's verdict also lands in a
    // word of pinned host memory, the prepared fallback launches wait here, and whoever next needs the stream to be final
    // (the next call into the chain, the batch's D2H copy, reset / synchronize / get_agc_state) reads the word and launches them
    // only when it is set.  iqgpu_chain_process_device keeps the queued scheme: its caller owns the stream and its synchronisation.
    // h_agc_verdict[0]: -1 = a verdict is awaited, 0 / 1 = k_agc_classify's answer
    HostMem<volatile int32_t> h_agc_verdict; int32_t *d_agc_verdict = nullptr;   // the same word, host and device address (the second: not owned)
    struct PendingVerdict { bool valid = false; bool filter = false; FrontArgs fb; FftConvArgs fc; AgcArgs ga; } pend;
    // ... and the AGC fused into the user filter's epilogue (k_fftconv16) where a filter stands between the resampler and the AGC:
    // the shipped -usb / -lsb presets
    bool agc_fusable_filter = false;
    // round 6: resampler -> post-resample overlap-save filter in ONE kernel (k_p0fft16, fftconv.hip): the chain's shape allows it,
    // with the window geometry it runs (fuse_win stream samples per block, fuse_vout outputs)
    bool fuse_filter = false; int fuse_win = 0, fuse_vout = 0;
    DevBuf ibuf[2]; int icur = 0;  // k_interp input: [ihist history][new samples]
    InterpArgs ia{};              // geometry of the r >= 1 path
    int ihist = 0;
    DevMem<float> d_ihb;
    DevBuf stage_in, stage_out;
    DevBuf seek_sink;             // where iqgpu_chain_seek's warm-up run writes what it emits (dropped)
    DevBuf seek_win;              // iqgpu_chain_dcrms_seek: the cf32 output of all its preroll calls, contiguous, for k_agc_rms_seek
    // pipelined host entry point (iqgpu_chain_submit / _measure_submit / _collect): kPipeSlots batches in flight.  H2D copies,
    // kernels (the chain's stream) and D2H copies each have their own stream; a batch moves to the next stage inside a later
    // submit / collect, once the host has seen the previous stage finish (no device-side event waits: see pipe_advance)
    struct IQGPU_LOCAL PipeSlot {
        Event in_done, k_done, all_done;
        DevBuf d_in, d_out; uint64_t ticket = 0; bool busy = false;
        size_t frames_in = 0, n_emit = 0; void *out = nullptr;
        float iq_mag = 0.0f, iq_phase = 0.0f;          // correction factors as of submit()
        // a batch of the measure pass (iqgpu_chain_measure_submit): nothing of its n_emit frames is copied back; its n_rows rows go
        // from the slot's own table (the chain's agc_rows would be overwritten by the next batch before the copy has run) to `rows`
        bool measure = false; DevBuf d_rows; size_t n_rows = 0; iqgpu_agc_chunk *rows = nullptr;
    };
    PipeSlot pipe[kPipeSlots];
    static constexpr int kCopyStreams = 4;                // small copies rotate over them, large ones keep to the first
    Stream pipe_h2d[kCopyStreams], pipe_d2h[kCopyStreams];
    bool pipe_ready = false;
    uint64_t pipe_seq = 0;        // tickets handed out
    uint64_t pipe_launched = 0;   // tickets whose kernels have been queued (<= pipe_seq)
    uint64_t pipe_copied = 0;     // tickets whose D2H copy has been queued (<= pipe_launched)
    // stream position behind the last ticket (valid while pipe_launched < pipe_seq)
    int pipe_rem = 0; uint64_t pipe_phi = 0, pipe_fpending = 0, pipe_total_in = 0, pipe_total_out = 0;
    // I/Q optimiser probe: first 1024 pre-processed samples of a call (device -> pinned host), src/pipeline.c:468-476
    // (the optimiser runs on ITS OWN thread beside the stage thread: aux_mu guards the factors and the probe state;
    //  a block in flight or not yet read is never overwritten -- the optimiser takes at most two a second)
    std::mutex aux_mu;
    bool probe_on = false, probe_pending = false, probe_valid = false;
    uint64_t probe_gen = 0;       // counts probe_drop calls: a reader that waited for a copy meanwhile dropped does not publish it
    DevMem<cf2> d_probe; HostMem<cf2> h_probe; Event probe_done;
    cf2 probe_last[1024];
    // I/Q calibration (iq_calib.cpp; buffers of its own, so that a call touches nothing the stream carries): window + twiddle table
    // (uploaded when allocated), the host form's raw blocks, the gathered cf32 blocks, candidates + metrics + power statistics
    DevBuf iq_cal_tab, iq_cal_in, iq_cal_blocks, iq_cal_work;
    char front_kernel[48] = "";   // which front kernel the last call launched (iqgpu_chain_front_kernel)
    bool poisoned = false;        // a call failed after device state had been touched: reset() clears it
    // placement of the arms in the tap planes of k_front_mid / k_front_fat for this chain's step (front_tap_fold, or sw.tap_fold)
    int tap_fold6 = 0, tap_fold8 = 0;
    // NCO phasor hold of k_front_mid for this chain's phase step at 6 / 8 outputs per lane (front_mid_nco_hold; off with sw.nco_hold)
    int nco_hold6 = 0, nco_hold8 = 0;
    int nco_hold6_all = 0;        // ... for the instantiations that hold all twelve phasors of a lane (front_mid_nco_hold_all)
    // profiling
    bool profiling = false;
    struct IQGPU_LOCAL TimedLaunch { int kind; Event a, b; };
    std::vector<TimedLaunch> pending_events;
    std::vector<Event> event_pool;
    iqgpu_profile prof{};
    // the members free themselves, in reverse order of declaration (a chain that never reached the device holds none: no HIP call)
    ~iqgpu_chain() { if (own_stream) (void)hipSetDevice(device); }
};

// ---- create-time design (abi.cpp): validation, ratio, operator constants, plans, launch geometry; touches no device ----
int design_chain(iqgpu_chain *c, const iqgpu_chain_desc *d);
// the eight words behind d_agc_flag as a chain starts (and restarts: iqgpu_chain_reset, iqgpu_chain_load_state) with them (abi.cpp)
extern const int32_t kAgcFlagInit[8];

// ------------------------------------------------------------------------------------------------
// stream-position arithmetic (closed forms; SPEC B.6)
// ------------------------------------------------------------------------------------------------
struct CallPlan {
    int64_t n_groups = 0;      // complete 2^S groups this call
    int64_t n_res = 0;         // front-kernel outputs this call (resampled, or one per input)
    int64_t n_emit = 0;        // frames written to the caller
    int64_t n_x = 0;           // r >= 1 path: samples entering k_interp (after the pre filter)
    int64_t n_arb = 0;         //              polyphase outputs; n_emit = n_arb << S
    uint64_t phi_next = 0;
    int rem_next = 0;
    uint64_t fpending_next = 0;
};

// the stream position a call starts from: what plan_call reads of the chain's host-side state
struct StreamPos { int rem = 0; uint64_t phi = 0; uint64_t fpending = 0; };
CallPlan plan_call_at(const iqgpu_chain *c, const StreamPos &at, size_t frames_in);      // plan.cpp
CallPlan plan_call(const iqgpu_chain *c, size_t frames_in);                               // ... from the chain's own position

// ---- a chain at ANY stream position (seamless range sharding, plan.cpp): all five position words of the chain after `frames` input
// frames of one stream from zero, and the outputs emitted in front of that position
constexpr uint64_t kMaxStreamFrames = (uint64_t)1 << 39;      // (groups << 24) and (outputs * step) stay inside 64 bits up to here
struct StreamAt { StreamPos pos; uint64_t n_out = 0; uint32_t nco_theta = 0, pnco_theta = 0; };
StreamAt stream_at(const iqgpu_chain *c, uint64_t frames);
// the chain's FIR memory in input frames (+ the DC blocker's warm-up): what a seek has to run in front of its position
// (with_dc = false: without that warm-up -- what iqgpu_chain_seek_dc asks for, which is handed the blocker's state)
uint64_t seek_preroll_frames(const iqgpu_chain *c, bool with_dc = true);
// what iqgpu_chain_seek_rms asks for (dx / local): that FIR memory, plus input frames that make the chain emit at least
// warm + chunk outputs wherever in the stream they lie (the closed form in iqgpu.h)
uint64_t seek_rms_preroll_frames(const iqgpu_chain *c);

// ---- profiling (process.cpp): HIP events around every launch while profiling is on ----
Event get_event(iqgpu_chain *c);
void drain_events(iqgpu_chain *c);
struct KernelTimer {
    iqgpu_chain *c; int kind; Event a, b;
    IQGPU_LOCAL KernelTimer(iqgpu_chain *c_, int kind_) : c(c_), kind(kind_)
    {
        if (c->profiling) { a = get_event(c); b = get_event(c); (void)hipEventRecord(a, c->stream); }
    }
    ~KernelTimer()
    {
        if (c->profiling) { (void)hipEventRecord(b, c->stream); c->pending_events.push_back({kind, std::move(a), std::move(b)}); }
    }
};

// ------------------------------------------------------------------------------------------------
// one process() call: per-call geometry, then the stages in stream order
//   [dc carries] -> front (one FrontRoute, below) -> [filter] -> [k_interp] -> [agc]
// ------------------------------------------------------------------------------------------------
// Which kernels the front of a call runs on: ONE value per call, chosen by Call::choose_route (plan.cpp; the order of the choice and
// the two demotions: DESIGN.md 3.0b), one enumerator per value iqgpu_chain_front_kernel reports.  What the host reads of a route it
// reads HERE -- from kRouteInfo, or from the switches below where the answer needs a launcher's function -- and nowhere else.
enum class FrontRoute { Generic, GenericLate, S1, S1S0, Fat, Mid, P0, P0Fft, Cascade, Cascade2, S2 };
struct RouteInfo {
    const char *name;      // what iqgpu_chain_front_kernel reports (k_front_mid: with the suffix of its MidSel, stage_front)
    int tile;              // input frames per tile of the plan (0: no wave plan; Mid: 128 per output of a lane -- route_tile)
    int lead;              // frames a streaming run reads in front of its first tile
    bool wave;             // wave-autonomous: cplan holds its runs, and the DC carries start where they do (dc_geom mode 1)
    bool casc;             // stages 0 .. S-2 in front of the last one: k_cascade's intermediate stream in c->mid, the last stage on d_hist2
    int fallback_tile;     // != 0: the fallback behind its fused-AGC launch is k_front_s1 on k_front_s1's OWN geometry of this tile (plan_s1)
    bool float_peaks;      // its fused-AGC epilogue keeps float peaks: the verifier tests them with a margin
};
constexpr RouteInfo kRouteInfo[] = {
    /* Generic     */ {"k_front",               0,          0,        false, false, 0,      false},   // the workgroup-tiled kernel
    /* GenericLate */ {"k_front+k_interp",      0,          0,        false, false, 0,      false},   // ... pointwise, the resampler behind it (r >= 1)
    /* S1          */ {"k_front_s1",            kWTile,     0,        true,  false, 0,      false},   // one half-band stage (m = 10)
    /* S1S0        */ {"k_front_s1",            256,        0,        true,  false, 0,      false},   // no half-band stage: k_front_s1<S0>
    /* Fat         */ {"k_front_fat",           kFatTile,   0,        true,  false, kWTile, false},   // S1's shape, 8 waves per CU (opt-in)
    /* Mid         */ {"k_front_mid",           0,          kMidLead, true,  false, kWTile, true},    // S1's shape, 12 waves per CU: long calls
    /* P0          */ {"k_front_p0",            256,        0,        true,  false, 256,    true},    // S1S0's shape, output-major: long calls
    /* P0Fft       */ {"k_p0fft16",             256,        0,        true,  false, 0,      false},   // ... and the filter behind it, in ONE kernel launched by stage_filter (opt-in)
    /* Cascade     */ {"k_cascade+k_front_s1",  kWTile,     0,        true,  true,  0,      false},   // S >= 2
    /* Cascade2    */ {"k_cascade2+k_front_s1", kWTile,     kWTile,   true,  true,  0,      false},   // ... two tiles per trip: a run of an odd number of tiles starts one tile early
    /* S2          */ {"k_front_s2",            2 * kWTile, 0,        true,  true,  0,      false},   // S == 2, both stages in one kernel: planned in tiles of the LAST stage
};
static_assert(sizeof(kRouteInfo) / sizeof(kRouteInfo[0]) == (size_t)FrontRoute::S2 + 1, "one row per route");
constexpr const RouteInfo &route_info(FrontRoute r) { return kRouteInfo[(int)r]; }
// (mid_nl: half-band outputs per lane of the call's k_front_mid instantiation, Call::mid_nl)
inline int route_tile(FrontRoute r, int mid_nl) { return r == FrontRoute::Mid ? front_mid_tile(mid_nl) : route_info(r).tile; }
// edge alignment: k_front_mid's 768-frame tiles hand their edge runs to the 512-frame tile routine -- edge runs of two tiles = three
// of its tiles, the streaming part starts and ends at an even tile
inline int route_align(FrontRoute r, int mid_nl) { return (r == FrontRoute::Mid && mid_nl == 6) ? 2 : 1; }
inline int route_edge_tpw(FrontRoute r, int mid_nl) { return r == FrontRoute::P0 ? front_p0_edge_tpw() : route_align(r, mid_nl); }
// waves per CU its launch is sized for (a: the plan's shape fields; the cascades need casc_wave_lds).  0: no wave plan of its own
inline int route_waves(FrontRoute r, const FrontArgs &a)
{
    switch (r) {
    case FrontRoute::S1: case FrontRoute::S1S0: case FrontRoute::P0Fft: return front_s1_waves(a);
    case FrontRoute::Fat: return front_fat_waves();
    case FrontRoute::Mid: return front_mid_waves();
    case FrontRoute::P0: return front_p0_waves();
    case FrontRoute::Cascade: case FrontRoute::Cascade2: return cascade_waves(a);
    case FrontRoute::S2: return front_s2_waves();
    case FrontRoute::Generic: case FrontRoute::GenericLate: break;
    }
    return 0;
}
// Seamless sharding of digital-AGC chains (ABI v8, seek.cpp).  Other than Ordinary: a call runs the chain's ordinary UNFUSED route
// -- its last stage leaves cf32 in abuf -- and the AGC itself stays out: no scan, no apply, no pack, the AGC state and its host
// mirrors untouched, nothing written to the caller's output.  Measure: k_agc_measure then writes one row per chunk into agc_rows
// (iqgpu_chain_measure); Drop: nothing reads abuf (the preroll of iqgpu_chain_seek_agc) -- or, dx / local, k_agc_rms_seek reads the
// call's samples behind abuf's lead of agc_rms_warm samples (the preroll of iqgpu_chain_seek_rms).
// MeasureS1: the other route of the measure pass, for agc_fusable chains: k_front_s1<.., AGC> -- their fallback kernel, which
// reduces the exact peak in front of the gain in its epilogue -- as it is, with the packed output into seek_sink and a scratch AGC
// state (agc_scratch); the rows are then put together from its peak array.  Half the traffic of Measure, a slower kernel.
// Shadow: exact sharding of chains with the DC blocker AND the AGC (iqgpu_chain_dcagc_*, seek.cpp).  The call is cut into the pieces
// of the ORDINARY call at its position (agc_call_cut) and every piece is planned as the ordinary piece is -- same plan_geometry, same
// dc_geom, agc_fused in the plan -- so the DC state, the histories and the position advance exactly as in the ordinary call, and so do
// the host's lock / seen mirrors.  Behind the arithmetic nothing is kept: an unfused piece leaves cf32 in abuf and k_agc_measure reads
// it (as Measure); a piece fused into the front kernel runs that launch against the scratch state with its packed output into
// seek_sink, no verdict and no fallback, and its rows come from the kernel's exact peak array (as MeasureS1, but on the ordinary
// call's plan); a piece whose gain the ordinary call applies in the FILTER's epilogue runs the same filter launch with the cf32
// epilogue -- the ordinary call's own fallback launch: same windows, same history move -- because the fused epilogue keeps float
// peaks, good for the verifier's margin test and not for a row.  The rows of a cut call are joined in chunk order.
enum class AgcMode { Ordinary, Measure, Drop, MeasureS1, Shadow };
struct CallOpts {                 // what an entry point asks of ONE call (process_device_impl).  The default: an ordinary call
    AgcMode agc = AgcMode::Ordinary;
    bool host_verdict = false;    // the host-ordered entry points: the verdict of a fused launch on the host (iqgpu_chain::h_agc_verdict)
    bool iq_fixed = false; float iq_mag = 0.0f, iq_phase = 0.0f;   // a pipelined batch: the correction factors as of its submit()
    AgcRow *rows = nullptr;       // Measure / MeasureS1 / Shadow: where the rows go on the device (a pipelined batch: its slot's table; nullptr: agc_rows)
    // the I/Q probe takes the head of ORDINARY stream calls only (iqgpu.h, iqgpu_chain_enable_iq_probe): the preroll of a seek, a
    // measuring call and every piece but the first of a call process_device_impl cuts in pieces stay out of it and leave the slot alone
    bool no_probe = false;
    size_t probe_span = 0;        // the first piece of such a cut call: frames of the WHOLE call, which the 1024-frame rule counts (0: frames_in)
};

struct Call {
    iqgpu_chain *c;
    const void *d_raw_in; size_t frames_in; void *d_out;
    CallOpts o;
    CallPlan p;
    bool filt; size_t L1; uint64_t fpending0;
    void *fin_out; int fin_fmt;              // where the LAST stage writes (d_out, or the AGC's cf32 buffer)
    int64_t total_tiles; int tpb, n_blocks;  // geometry of the workgroup-tiled k_front
    FrontRoute route;                        // which front path runs (choose_route)
    int mid_nl = 0;                          // Mid: half-band outputs per lane of its instantiation (6, or 8: its tile is 128 of them)
    int64_t s2_in_tiles = 0;                 // S2 (cplan is then the LAST stage's plan): the number of 512-frame input tiles of the call
    int wtile, casc_K, rem_k;                // input frames per tile of the plan; stages in front of the last one; open group as the first kernel sees it
    float iq_mag = 0.0f, iq_phase = 0.0f;    // the correction factors this call applies (snapshot under aux_mu)
    bool agc_fused = false;                  // this call: gain applied in the front kernel -- or, with a filter behind it, in the filter's epilogue -- and verified behind it (AgcMode::MeasureS1: that front kernel, no verdict)
    bool front_fused() const { return agc_fused && !filt; }
    // a fused front launch whose output nobody keeps: the scratch AGC state, no verdict, the rows from its peak array
    bool no_verdict() const { return o.agc == AgcMode::MeasureS1 || o.agc == AgcMode::Shadow; }
    bool verdict_on_host() const { return o.host_verdict && c->h_agc_verdict != nullptr; }   // the fallback behind a fused launch waits for the host
    FrontArgs cplan;                         // run geometry of the wave-autonomous kernel that sees the raw input
    cf2 *fcur = nullptr, *icur = nullptr;    // filter-input / k_interp-input buffers of this call

    // run rule of the wave-autonomous kernels: one run per resident wave when auto (wave slots of ONE round of
    // workgroups), else fixed-length runs from block_samples
    int64_t wave_slots(int waves) const { return (int64_t)c->n_cu * waves; }
    int fixed_tpw() const
    {
        if (c->auto_block) return 0;
        int64_t t = (int64_t)c->tiles_per_block * kTile / (16 * kWTile);
        if (t < 1) t = 1;
        if (t > (1 << 30)) t = 1 << 30;
        return (int)t;
    }
    void copy_plan(FrontArgs &dst) const
    {
        dst.w_total_tiles = cplan.w_total_tiles;
        dst.w_warm_tiles = cplan.w_warm_tiles; dst.w_edge_tpw = cplan.w_edge_tpw;
        dst.w_n_stream = cplan.w_n_stream; dst.w_run_q = cplan.w_run_q; dst.w_run_r = cplan.w_run_r;
        dst.w_edge_ta = cplan.w_edge_ta; dst.w_edge_tb = cplan.w_edge_tb;
        dst.w_n_edge1 = cplan.w_n_edge1; dst.w_n_edge = cplan.w_n_edge;
        dst.w_wpw = cplan.w_wpw; dst.w_wsum = cplan.w_wsum;
        for (int i = 0; i < 4; ++i) dst.w_wt[i] = cplan.w_wt[i];
        dst.p0_k_a = cplan.p0_k_a; dst.p0_k_b = cplan.p0_k_b; dst.p0_f_max = cplan.p0_f_max;
    }
    int raw_aligned() const { return (((uintptr_t)d_raw_in) & 15u) == 0 ? 1 : 0; }
    AgcRow *measure_rows() const { return o.rows ? o.rows : (AgcRow *)c->agc_rows.p; }   // the device table of a measuring call
    // the per-chunk peaks a fused front launch accumulates into start from zero: k_agc_classify zeroes what it has read (agc_peak
    // and agc_peak_b), so only the first fused call behind an unfused one (or behind a reallocation) pays for a fill
    hipError_t clean_agc_peaks()
    {
        if (c->agc_peak_clean) return hipSuccess;
        const hipError_t e = hipMemsetAsync(c->agc_peak.p, 0, c->agc_peak.cap, c->stream);
        if (e == hipSuccess) c->agc_peak_clean = true;
        return e;
    }
    // the fused-AGC fields of a front launch (the measure pass on that kernel: the gain of a scratch state), and its peak array zeroed
    hipError_t wire_fused_agc(FrontArgs &a)
    {
        a.agc_fused = 1; a.agc_state = no_verdict() ? (const AgcState *)c->agc_scratch.p : c->d_agc_state;
        a.agc_peak2 = (unsigned long long *)c->agc_peak.p; a.agc_chunk_frames = c->agc_chunk; a.agc_shift = c->S; a.agc_rem = c->rem;
        return clean_agc_peaks();
    }

    // the run descriptors of k_front_mid (FrontArgs::w_steal): run stealing (rounds > 0), or one round of workgroups over more
    // fixed-length runs than resident waves (run_stride > 0)
    void wire_run_descriptors(FrontArgs &a, int rounds, int64_t run_stride) const
    {
        a.w_steal = (unsigned long long *)c->steal_buf.p; a.w_steal_min = c->sw.steal_min;
        a.w_steal_stride = c->sw.steal_stride; a.w_steal_lanes = c->sw.steal_lanes; a.w_steal_rounds = rounds;
        a.w_run_stride = run_stride;
    }

    void plan_geometry();                    // plan.cpp: k_front's blocks, then choose_route and plan_route
    bool choose_route();                     // sets route; true: the choice needed the route's plan, which stands in cplan
    void plan_route();                       // cplan, wtile (and S2: rem_k, s2_in_tiles) of the route
    void plan_s1(FrontArgs &a, int tile, int warm_tiles = 0) const;   // THE k_front_s1 geometry of a.rem0 + a.frames_in frames
    int front_cascade(FrontArgs &a);         // stage_front of the routes with k_cascade's stages in front
    DcGeom dc_geom() const;
    AgcGeom agc_geom() const;
    int stage_dc_carries();
    int prepare_buffers();
    int stage_front();
    int stage_filter();
    int stage_late_resampler();
    int stage_agc();
    int stage_agc_measure();
    int stage_agc_rows_from_peaks();
    int stage_agc_verify(int peak_approx, AgcArgs *ga);
    int stage_agc_verify_and_fallback(const FrontArgs &spec);
    int stage_agc_verify_and_fallback_filter(const FftConvArgs &spec);
    AgcArgs agc_args() const;
};

// ---- entry points shared across translation units ----
int process_device_impl(iqgpu_chain *c, const void *d_raw_in, size_t frames_in, void *d_out, size_t out_capacity_bytes,
                        size_t *frames_out, const CallOpts &o = CallOpts());              // process.cpp
int stage_host_input(iqgpu_chain *c, const void *in, size_t frames, const void **d_in);   // process.cpp: host frames into stage_in, *d_in
// process.cpp: the DC blocker's map of the call process_device_impl would make of these frames at stream position `at`, into d_map[0 .. 2)
// (past_lock: the piece of an AGC chain's call behind the lock, planned with the gain in its last kernel -- iqgpu_chain_dcagc_dc_measure)
int dc_measure_call(iqgpu_chain *c, const StreamPos &at, const void *d_raw_in, size_t frames_in, cd2 *d_map, bool past_lock = false);
// ... its planning alone (host arithmetic; the chain's position is put back): the segments of that call and the alignment of its address
struct DcMeasurePlan { DcGeom geom; int raw_aligned; };
DcMeasurePlan dc_measure_plan(iqgpu_chain *c, const StreamPos &at, const void *d_raw_in, size_t frames_in, bool past_lock = false);
// agc_host.cpp: ONE definition of how a call of a chain with the digital AGC is cut -- the frames of its unfused head (0: none,
// frames_in: the whole call); the rest runs with the gain fused into its last kernel.  A function of the lock / seen mirrors, the
// stream position and the call's length alone; *locks: the locking chunk lies in this call
size_t agc_call_cut(const iqgpu_chain *c, bool locked, uint64_t seen, const StreamPos &at, size_t frames_in, bool *locks);
// ... and the mirrors in front of stream frame `frames` of a stream processed on a grid of multiples of agc_chunk_frames (closed form)
void agc_mirrors_at(const iqgpu_chain *c, uint64_t frames, bool *locked, uint64_t *seen);
// behind a fused launch whose fallback waits for the verdict on the host: waits for the word, launches the fallback when it is set
// (*ran = true then).  No-op without a pending verdict.
int agc_resolve_pending(iqgpu_chain *c, bool *ran = nullptr);                             // agc_host.cpp
// seek.cpp: what the two-pass calls ask of a chain (the digital output AGC on the sample clock), and the route of its measure pass
int agc_two_pass_check(const iqgpu_chain *c, const char *who);
AgcMode measure_route(const iqgpu_chain *c);
// seek.cpp: the six ways a chain is started mid-stream -- iqgpu_chain_seek, _seek_agc, _seek_dc, _dcagc_seek, _seek_rms, _dcrms_seek --
// and, one row per family in shard_family's table, everything its entry points do differently.  The checks themselves are in seek.cpp
enum class SeekKind { Plain, Agc, Dc, DcAgc, Rms, DcRms };
enum class ShardCheck { None, TwoPass, Rms, DcRms };          // none, two_pass_check(needs), rms_seek_check, dcrms_check
struct ShardFamily {
    ShardCheck check; unsigned needs;     // what every entry point of the family asks of a chain (needs: kNeedAgc | kNeedDc of TwoPass)
    AgcMode preroll_agc;                  // the AGC stage of the preroll's calls (Ordinary: their output goes to seek_sink, else nowhere)
    bool dc_at;                           // takes the blocker's state in front of the preroll, and the grid of calls the preroll runs in
    bool agc_entry;                       // takes the AGC state at first_frame and installs it
    bool rebuild_agc;                     // the AGC loop's state at first_frame is rebuilt from the preroll's cf32 output ...
    bool gather;                          // ... of every call, gathered in seek_win (else: of the one call, where it lies in abuf)
    uint64_t (*memory)(const iqgpu_chain *);      // the preroll the chain needs far enough into the stream
    const char *seek, *dc_measure, *dc_advance, *measure, *design_preroll, *dc_measure_range;      // its entry points (nullptr: it has none)
};
// (hidden: between seek.cpp and plan.cpp only -- the library's dynamic symbol table stays as it was)
__attribute__((visibility("hidden"))) const ShardFamily &shard_family(SeekKind k);
// the family's check under the name of the entry point that asks (description: in the words of a design_* call, where they differ)
__attribute__((visibility("hidden"))) int shard_check(const ShardFamily &f, const iqgpu_chain *c, const char *who, bool description = false);
int rms_seek_check(const iqgpu_chain *c, const char *who);      // an output AGC of profile dx / local, no DC blocker (with it: iqgpu_chain_dcrms_seek)
// abi.cpp: empties the I/Q probe's slot -- a block staged or held belongs to the stream the chain is leaving (reset, seek, load_state).
// Called behind the batches in flight; waits for a staged copy, so that it cannot land in the pinned buffer later
int probe_drop(iqgpu_chain *c);
int pipe_advance(iqgpu_chain *c, uint64_t upto);   // pipeline.cpp: queues the kernels of every submitted batch up to ticket `upto`
int pipe_drain(iqgpu_chain *c, uint64_t upto);     // ... and their D2H copies
