// seek.cpp -- seamless range sharding: a chain started mid-stream, the AGC measure pass (both: modes of process.cpp's call; its pipelined
// form is in pipeline.cpp), the AGC walk; the DC blocker's measure pass, walk and seek.  What the six seek families ask of a chain
// (two_pass_check, rms_seek_check, dcrms_check) and everything else they do differently: shard_family's table, below
#include "chain.hpp"

// ------------------------------------------------------------------------------------------------
// iqgpu_chain_seek: the chain at stream frame first_frame -- reset, the closed-form position preroll_frames earlier, and the
// preroll through the ordinary per-call path with its output dropped (seamless range sharding, iqgpu.h)
// ------------------------------------------------------------------------------------------------
// What the calls of the exact recipes ask of a chain.  kNeedAgc (the v8 / v9 calls): the digital output AGC on the sample clock.
// kNeedDc (the DC blocker's calls): the blocker -- and, alone, no output AGC.  Both: iqgpu_chain_dcagc_*
enum : unsigned { kNeedAgc = 1, kNeedDc = 2 };
static int two_pass_check(const iqgpu_chain *c, const char *who, unsigned needs)
{
    if (!c) return fail(IQGPU_EINVAL, "%s: NULL chain", who);
    if ((needs & kNeedDc) && !c->dc) return fail(IQGPU_EINVAL, "%s: the chain has no DC blocker", who);
    if (needs == kNeedDc && c->agc) return fail(IQGPU_EUNSUPPORTED, "%s: a chain with the output AGC -- its measure route may cut a call into "
        "other segments than the process route, so the two exact recipes do not combine (such chains: iqgpu_chain_dcagc_* for the "
        "digital profile, iqgpu_chain_dcrms_* for dx / local)", who);
    if (!(needs & kNeedAgc)) return IQGPU_OK;
    if (!c->agc) return fail(IQGPU_EINVAL, "%s: the chain has no output AGC", who);
    if (c->agc_rms_alpha > 0.0f) return fail(IQGPU_EUNSUPPORTED, "%s: the AGC profiles dx / local carry a per-sample loop state that no "
        "table of per-chunk figures reproduces exactly; only the digital profile is sharded seamlessly", who);
    if (c->desc.agc_clock == IQGPU_AGC_CLOCK_WALL) return fail(IQGPU_EUNSUPPORTED, "%s: IQGPU_AGC_CLOCK_WALL has no value at a stream "
        "position; use IQGPU_AGC_CLOCK_SAMPLES", who);
    return IQGPU_OK;
}
int agc_two_pass_check(const iqgpu_chain *c, const char *who) { return two_pass_check(c, who, kNeedAgc); }

// what iqgpu_chain_seek_rms asks of a chain, and iqgpu_design_preroll_frames_rms of a description (in the same words): an output AGC of
// profile dx / local, no DC blocker
int rms_seek_check(const iqgpu_chain *c, const char *who)
{
    if (!c) return fail(IQGPU_EINVAL, "%s: NULL chain", who);
    if (!c->agc) return fail(IQGPU_EINVAL, "%s: the chain has no output AGC", who);
    if (!(c->agc_rms_alpha > 0.0f)) return fail(IQGPU_EUNSUPPORTED, "%s: the digital AGC profile works chunk by chunk and is sharded by "
        "iqgpu_chain_seek_agc; this call is for the profiles dx / local", who);
    if (c->dc) return fail(IQGPU_EUNSUPPORTED, "%s: a chain with the DC blocker -- its exact route needs a call grid and a walked state "
        "(iqgpu_chain_seek_dc); iqgpu_chain_dcrms_seek composes the two", who);
    return IQGPU_OK;
}

// what iqgpu_chain_dcrms_* ask of a chain: the DC blocker and the output AGC of profile dx / local.  Such a chain never cuts a call
// (agc_fusable and agc_fusable_filter want the digital profile): every call runs whole on the unfused route, so the reason the DC
// blocker's calls have to refuse an AGC chain does not hold for it.  (description: asked by iqgpu_design_preroll_frames_dcrms, which
// names its own siblings)
static int dcrms_check(const iqgpu_chain *c, const char *who, bool description)
{
    const char *what = description ? "description" : "chain";
    if (!c) return fail(IQGPU_EINVAL, "%s: NULL chain", who);
    if (!c->dc) return fail(IQGPU_EINVAL, "%s: the %s has no DC blocker (without it: %s)", who, what,
        description ? "iqgpu_design_preroll_frames_rms" : "iqgpu_chain_seek_rms");
    if (!c->agc) return fail(IQGPU_EINVAL, "%s: the %s has no output AGC%s", who, what, description ? "" : " (without it: iqgpu_chain_seek_dc)");
    if (!(c->agc_rms_alpha > 0.0f)) return fail(IQGPU_EUNSUPPORTED, "%s: the digital AGC profile works chunk by chunk and is sharded by "
        "iqgpu_chain_dcagc_*; this call is for the profiles dx / local", who);
    return IQGPU_OK;
}

// The six families, one row each, in SeekKind's order (chain.hpp: SeekKind, ShardFamily).  How their seeks run:
//   Plain  the preroll as ordinary calls, their output into seek_sink
//   Agc    the preroll with the AGC out of the way, then *agc_entry (or the fresh state) installed
//   Dc     no warm-up of the DC blocker asked for: *dc_at (or zero) is its state in front of the preroll, which runs in calls of
//          call_frames (0: one call)
//   DcAgc  both at once: the preroll as SHADOW calls (chain.hpp, AgcMode) from the host mirrors' closed form
//   Rms    dx / local: the preroll with the AGC out of the way and its cf32 output kept on the device, then the loop's state at
//          first_frame from k_agc_rms_seek over those samples
//   DcRms  Dc and Rms at once: *dc_at in front of a preroll in calls of call_frames, the cf32 output of every one of them gathered in
//          seek_win, k_agc_rms_seek over that
static uint64_t fir_and_dc_memory(const iqgpu_chain *c) { return seek_preroll_frames(c, true); }
static uint64_t fir_memory(const iqgpu_chain *c) { return seek_preroll_frames(c, false); }
const ShardFamily &shard_family(SeekKind k)
{
    using SC = ShardCheck;
    using AM = AgcMode;
    static const ShardFamily rows[6] = {
        //        check      needs               preroll_agc   dc_at  entry  rebuild gather memory
        /*Plain*/ {SC::None,    0,                  AM::Ordinary, false, false, false, false, fir_and_dc_memory,
                   "iqgpu_chain_seek", nullptr, nullptr, nullptr, "iqgpu_design_preroll_frames", nullptr},
        /*Agc*/   {SC::TwoPass, kNeedAgc,           AM::Drop,     false, true,  false, false, fir_and_dc_memory,
                   "iqgpu_chain_seek_agc", nullptr, nullptr, "iqgpu_chain_measure", nullptr, nullptr},
        /*Dc*/    {SC::TwoPass, kNeedDc,            AM::Ordinary, true,  false, false, false, fir_memory,
                   "iqgpu_chain_seek_dc", "iqgpu_chain_dc_measure", "iqgpu_chain_dc_advance", nullptr, nullptr, "iqgpu_chain_dc_measure_range"},
        /*DcAgc*/ {SC::TwoPass, kNeedDc | kNeedAgc, AM::Shadow,   true,  true,  false, false, fir_memory,
                   "iqgpu_chain_dcagc_seek", "iqgpu_chain_dcagc_dc_measure", "iqgpu_chain_dcagc_dc_advance", "iqgpu_chain_dcagc_measure", nullptr,
                   "iqgpu_chain_dcagc_dc_measure_range"},
        /*Rms*/   {SC::Rms,     0,                  AM::Drop,     false, false, true,  false, seek_rms_preroll_frames,
                   "iqgpu_chain_seek_rms", nullptr, nullptr, nullptr, "iqgpu_design_preroll_frames_rms", nullptr},
        /*DcRms*/ {SC::DcRms,   0,                  AM::Drop,     true,  false, true,  true,  seek_rms_preroll_frames,
                   "iqgpu_chain_dcrms_seek", "iqgpu_chain_dcrms_dc_measure", "iqgpu_chain_dcrms_dc_advance", nullptr,
                   "iqgpu_design_preroll_frames_dcrms", "iqgpu_chain_dcrms_dc_measure_range"},
    };
    return rows[(int)k];
}

int shard_check(const ShardFamily &f, const iqgpu_chain *c, const char *who, bool description)
{
    switch (f.check) {
    case ShardCheck::None:    return IQGPU_OK;
    case ShardCheck::TwoPass: return two_pass_check(c, who, f.needs);
    case ShardCheck::Rms:     return rms_seek_check(c, who);
    case ShardCheck::DcRms:   return dcrms_check(c, who, description);
    }
    return IQGPU_OK;
}

// what a seek was given beyond the position and the preroll
struct SeekRequest {
    SeekKind kind = SeekKind::Plain;
    bool on_device = false;                        // the preroll is in device memory
    const iqgpu_agc_state *agc_entry = nullptr;    // families with agc_entry
    const iqgpu_dc_state *dc_at = nullptr;         // families with dc_at
    size_t call_frames = 0;                        // families with dc_at
};

static int seek_impl(iqgpu_chain *c, uint64_t first_frame, const void *preroll, size_t preroll_frames, const SeekRequest &rq)
{
    const ShardFamily &fam = shard_family(rq.kind);
    const char *who = fam.seek;
    if (!c) return fail(IQGPU_EINVAL, "%s: NULL chain", who);
    // what iqgpu_chain_reset does comes first: batches in flight and a pending verdict resolved, histories and dc state zeroed,
    // the poison cleared -- a refused argument below leaves the chain reset
    int rc = iqgpu_chain_reset(c); if (rc) return rc;
    c->fpending = 0;                                          // (reset keeps the FFT remainder queued: a seek starts a stream)
    rc = shard_check(fam, c, who); if (rc) return rc;
    if (fam.agc_entry) {
        const iqgpu_agc_state *e = rq.agc_entry;
        if (e && (e->locked != 0 && e->locked != 1)) return fail(IQGPU_EINVAL, "%s: entry state with locked = %d", who, e->locked);
    }
    cd2 dc_at{0.0, 0.0};
    if (fam.dc_at) {
        if (rq.dc_at) { dc_at.x = rq.dc_at->re; dc_at.y = rq.dc_at->im; }
        if (!std::isfinite(dc_at.x) || !std::isfinite(dc_at.y)) return fail(IQGPU_EINVAL, "%s: the state in front of the preroll is not finite", who);
        if (rq.call_frames && preroll_frames % rq.call_frames != 0) return fail(IQGPU_EINVAL, "%s: a preroll of %zu frames is not a whole number "
            "of calls of %zu frames", who, preroll_frames, rq.call_frames);
        // (the cut of a call is a closed form of the position only on the chunk grid)
        if (fam.preroll_agc == AgcMode::Shadow && (first_frame % (uint64_t)c->agc_chunk || rq.call_frames % (size_t)c->agc_chunk || preroll_frames % (size_t)c->agc_chunk))
            return fail(IQGPU_EINVAL, "%s: first_frame %llu, call_frames %zu and the preroll of %zu frames have to be multiples of "
                "agc_chunk_frames = %lld", who, (unsigned long long)first_frame, rq.call_frames, preroll_frames, (long long)c->agc_chunk);
    }
    if (first_frame > kMaxStreamFrames) return fail(IQGPU_EINVAL, "%s: frame %llu is beyond 2^39 frames", who, (unsigned long long)first_frame);
    if ((uint64_t)preroll_frames > first_frame) return fail(IQGPU_EINVAL, "%s: a preroll of %zu frames would start in front of "
        "frame 0 (first_frame %llu)", who, preroll_frames, (unsigned long long)first_frame);
    if (first_frame > 0) {
        // (a family without a check of its own has no way with the output AGC)
        if (c->agc && fam.check == ShardCheck::None) return fail(IQGPU_EUNSUPPORTED, "iqgpu_chain_seek: the output AGC depends on the whole stream in front of a position, "
            "not on a bounded warm-up");
        const uint64_t memory = fam.memory(c), need = first_frame < memory ? first_frame : memory;
        if ((uint64_t)preroll_frames < need) return fail(IQGPU_EINVAL, "%s: preroll of %zu frames is shorter than the %llu "
            "this chain needs at frame %llu", who, preroll_frames, (unsigned long long)need, (unsigned long long)first_frame);
        if (preroll_frames && !preroll) return fail(IQGPU_EINVAL, "%s: NULL preroll", who);
    }
    if (fam.dc_at) {
        // the blocker's state in front of the preroll (at frame 0: of the stream), where the reset has left zero -- behind every
        // refusal, so that a refused call leaves the chain reset
        HIP_TRY(hipMemcpyAsync(c->d_dc_state, &dc_at, sizeof(cd2), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    if (first_frame > 0) {
        const StreamAt from = stream_at(c, first_frame - (uint64_t)preroll_frames), to = stream_at(c, first_frame);
        // gather: room for the cf32 output of ALL preroll calls, sized before the first launch (a failure here leaves the chain reset)
        const size_t win_total = (size_t)(to.n_out - from.n_out);
        size_t win_at = 0;
        if (fam.gather) { rc = c->seek_win.ensure((win_total + 1) * sizeof(cf2)); if (rc) return rc; }
        if (c->fp.enabled) {
            // [L-1 history][pending]: zeros stand for the samples in front of the warm-up
            const size_t front = c->fp.taps.size() - 1 + (size_t)from.pos.fpending;
            rc = c->fbuf[c->fcur].ensure((front + 1) * sizeof(cf2)); if (rc) return rc;
            HIP_TRY(hipMemsetAsync(c->fbuf[c->fcur].p, 0, front * sizeof(cf2), c->stream));
        }
        c->rem = from.pos.rem; c->phi = from.pos.phi; c->fpending = from.pos.fpending;
        c->nco_theta = from.nco_theta; c->pnco_theta = from.pnco_theta;
        // (the preroll lies in front of the range the caller asked for: the I/Q probe takes no block from it and keeps its slot free
        //  for the head of the first call behind the seek)
        // Drop: nothing of the preroll is kept and the AGC must not see it: the unfused route into abuf, no AGC kernel behind it
        // (rebuild_agc: the call's cf32 samples stay in abuf, behind its lead of agc_rms_warm samples, for k_agc_rms_seek below; gather:
        //  every call writes there, where the single stream's call writes, and its samples are copied behind those of the calls in front).
        // Shadow: cut as the single stream's calls are, from the mirrors the single stream has in front of the preroll
        const bool shadow = fam.preroll_agc == AgcMode::Shadow, to_sink = fam.preroll_agc == AgcMode::Ordinary;
        CallOpts preroll_call; preroll_call.no_probe = true; preroll_call.agc = fam.preroll_agc;
        if (shadow) agc_mirrors_at(c, first_frame - (uint64_t)preroll_frames, &c->agc_locked_host, &c->agc_seen_host);

        // with call_frames the preroll runs in the single stream's own calls -- every one staged like a call of iqgpu_chain_process --
        // from the single stream's own state; otherwise in one call.  No frames: no call
        const size_t obps = bytes_per_frame(c->desc.out_format), ibps = bytes_per_frame(c->desc.in_format);
        const size_t per = fam.dc_at && rq.call_frames ? rq.call_frames : preroll_frames;
        for (size_t at = 0; at < preroll_frames; at += per) {
            const void *src = (const char *)preroll + at * ibps, *d_in = src;
            if (!rq.on_device) { rc = stage_host_input(c, src, per, &d_in); if (rc) return rc; }
            size_t dropped = 0;
            if (to_sink) { rc = c->seek_sink.ensure((size_t)plan_call(c, per).n_emit * obps + 16); if (rc) return rc; }
            rc = process_device_impl(c, d_in, per, to_sink ? c->seek_sink.p : nullptr, to_sink ? c->seek_sink.cap : 0, &dropped, preroll_call);
            if (rc) return rc;
            if (fam.gather) {
                const hipError_t e = win_at + dropped <= win_total
                    ? launch_copy_cf((cf2 *)c->seek_win.p + win_at, (const cf2 *)c->abuf.p + c->agc_rms_warm, (int64_t)dropped, c->stream)
                    : hipErrorInvalidValue;
                if (e != hipSuccess) { c->poisoned = true; return fail(IQGPU_EHIP, "%s: %s", who, hipGetErrorString(e)); }
                win_at += dropped;
            }
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        // the warm-up has walked the position forward call-wise: it has to stand on the closed form at first_frame
        if (c->rem != to.pos.rem || c->phi != to.pos.phi || c->fpending != to.pos.fpending || c->nco_theta != to.nco_theta ||
            c->pnco_theta != to.pnco_theta || (fam.gather && win_at != win_total)) {
            c->poisoned = true;
            return fail(IQGPU_EINVAL, "internal: the position behind the preroll is not the closed form at frame %llu", (unsigned long long)first_frame);
        }
        c->total_in = first_frame; c->total_out = to.n_out;       // (iqgpu_chain_tell: of the stream, not of the preroll)
        // (the mirrors the shadow calls have walked forward: the closed form at first_frame -- stated, so that a chain which never cuts
        //  a call, and so never moves them, carries them too)
        if (shadow) agc_mirrors_at(c, first_frame, &c->agc_locked_host, &c->agc_seen_host);
        if (fam.rebuild_agc && to.n_out > 0) {
            // The loop's state at the cut from the samples the preroll has left at abuf + W: stream positions [pos0, cut).  The
            // trajectory of the chunk that holds sample cut - 1 starts at `start`; the preroll's outputs are the single stream's from
            // `clean` on (position 0 when it began at frame 0, else the first output behind the frames that refill the FIR memory).
            const int64_t W = c->agc_rms_warm, cut = (int64_t)to.n_out, pos0 = (int64_t)from.n_out;
            AgcRmsArgs ra{};
            int32_t nch = 0;
            agc_rms_geometry(c->agc_rms_alpha, 0, 0, &ra.chunk, &ra.warm, &nch);
            const int64_t a0 = (cut - 1) / ra.chunk * ra.chunk - ra.warm, start = a0 > 0 ? a0 : 0;
            const int64_t clean = (uint64_t)preroll_frames == first_frame ? 0
                : (int64_t)stream_at(c, first_frame - (uint64_t)preroll_frames + seek_preroll_frames(c, false)).n_out;
            const bool room = fam.gather ? (int64_t)c->seek_win.cap >= (cut - pos0) * (int64_t)sizeof(cf2)
                                    : (int64_t)c->abuf.cap >= (W + cut - pos0) * (int64_t)sizeof(cf2);
            if (clean > start || pos0 > start || !room) {
                c->poisoned = true;
                return fail(IQGPU_EINVAL, "internal: the preroll's outputs [%lld, %lld) (exact from %lld) do not reach back to %lld, where the AGC "
                    "trajectory in front of frame %llu starts", (long long)pos0, (long long)cut, (long long)clean, (long long)start,
                    (unsigned long long)first_frame);
            }
            ra.x = fam.gather ? (const cf2 *)c->seek_win.p : (const cf2 *)c->abuf.p + W; ra.n = cut - pos0; ra.pos0 = pos0; ra.hist_valid = 0;
            ra.alpha = c->agc_rms_alpha; ra.state = c->d_agc_state;
            hipError_t e = launch_agc_rms_seek(ra, c->stream);
            // the warm-up window of the calls to come: the last W samples in front of the cut (a stream shorter than that: its own
            // samples, at the end)
            const int64_t keep = ra.n < W ? ra.n : W;
            if (e == hipSuccess) e = launch_copy_cf((cf2 *)c->agc_hist.p + (W - keep), ra.x + (ra.n - keep), keep, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) { c->poisoned = true; return fail(IQGPU_EHIP, "%s: %s", who, hipGetErrorString(e)); }
            c->agc_rms_pos = to.n_out;
        }
    }
    if (fam.agc_entry && rq.agc_entry) {
        // The AGC state of the stream at first_frame, everywhere the chain keeps it: the device state the kernels read, and the host's
        // mirrors of "has the stream locked" and of samples_seen, from which the fused / unfused split of every later call follows
        // (agc_unfused_head).  The reset above has left the rest as on a chain that arrived here by processing: no pending verdict,
        // the verifier's eight words at their initial values (no healthy chunk recorded for the call to come), the peak array marked
        // dirty so that the first fused launch clears it.
        static_assert(sizeof(iqgpu_agc_state) == sizeof(AgcState), "AGC state layout");
        AgcState st;
        memcpy(&st, rq.agc_entry, sizeof(st));
        st.reserved = 0;
        HIP_TRY(hipMemcpyAsync(c->d_agc_state, &st, sizeof(AgcState), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->agc_locked_host = st.locked != 0;
        c->agc_seen_host = st.seen;
    }
    return IQGPU_OK;
}

// (a request in SeekRequest's order: kind, on_device, agc_entry, dc_at, call_frames)
extern "C" int iqgpu_chain_seek(iqgpu_chain *c, uint64_t first_frame, const void *preroll, size_t preroll_frames)
{
    return seek_impl(c, first_frame, preroll, preroll_frames, {SeekKind::Plain, false});
}
extern "C" int iqgpu_chain_seek_device(iqgpu_chain *c, uint64_t first_frame, const void *d_preroll, size_t preroll_frames)
{
    return seek_impl(c, first_frame, d_preroll, preroll_frames, {SeekKind::Plain, true});
}
extern "C" int iqgpu_chain_seek_agc(iqgpu_chain *c, uint64_t first_frame, const void *preroll, size_t preroll_frames, const iqgpu_agc_state *entry)
{
    return seek_impl(c, first_frame, preroll, preroll_frames, {SeekKind::Agc, false, entry});
}
extern "C" int iqgpu_chain_seek_agc_device(iqgpu_chain *c, uint64_t first_frame, const void *d_preroll, size_t preroll_frames,
                                           const iqgpu_agc_state *entry)
{
    return seek_impl(c, first_frame, d_preroll, preroll_frames, {SeekKind::Agc, true, entry});
}
extern "C" int iqgpu_chain_seek_rms(iqgpu_chain *c, uint64_t first_frame, const void *preroll, size_t preroll_frames)
{
    return seek_impl(c, first_frame, preroll, preroll_frames, {SeekKind::Rms, false});
}
extern "C" int iqgpu_chain_seek_rms_device(iqgpu_chain *c, uint64_t first_frame, const void *d_preroll, size_t preroll_frames)
{
    return seek_impl(c, first_frame, d_preroll, preroll_frames, {SeekKind::Rms, true});
}
extern "C" int iqgpu_chain_seek_dc(iqgpu_chain *c, uint64_t first_frame, const void *preroll, size_t preroll_frames, size_t call_frames,
                                   const iqgpu_dc_state *at_preroll_start)
{
    return seek_impl(c, first_frame, preroll, preroll_frames, {SeekKind::Dc, false, nullptr, at_preroll_start, call_frames});
}
extern "C" int iqgpu_chain_seek_dc_device(iqgpu_chain *c, uint64_t first_frame, const void *d_preroll, size_t preroll_frames,
                                          size_t call_frames, const iqgpu_dc_state *at_preroll_start)
{
    return seek_impl(c, first_frame, d_preroll, preroll_frames, {SeekKind::Dc, true, nullptr, at_preroll_start, call_frames});
}
extern "C" int iqgpu_chain_dcrms_seek(iqgpu_chain *c, uint64_t first_frame, const void *preroll, size_t preroll_frames, size_t call_frames,
                                      const iqgpu_dc_state *dc_at_preroll_start)
{
    return seek_impl(c, first_frame, preroll, preroll_frames, {SeekKind::DcRms, false, nullptr, dc_at_preroll_start, call_frames});
}
extern "C" int iqgpu_chain_dcrms_seek_device(iqgpu_chain *c, uint64_t first_frame, const void *d_preroll, size_t preroll_frames,
                                             size_t call_frames, const iqgpu_dc_state *dc_at_preroll_start)
{
    return seek_impl(c, first_frame, d_preroll, preroll_frames, {SeekKind::DcRms, true, nullptr, dc_at_preroll_start, call_frames});
}
extern "C" int iqgpu_chain_dcagc_seek(iqgpu_chain *c, uint64_t first_frame, const void *preroll, size_t preroll_frames, size_t call_frames,
                                      const iqgpu_dc_state *dc_at_preroll_start, const iqgpu_agc_state *agc_entry)
{
    return seek_impl(c, first_frame, preroll, preroll_frames, {SeekKind::DcAgc, false, agc_entry, dc_at_preroll_start, call_frames});
}
extern "C" int iqgpu_chain_dcagc_seek_device(iqgpu_chain *c, uint64_t first_frame, const void *d_preroll, size_t preroll_frames,
                                             size_t call_frames, const iqgpu_dc_state *dc_at_preroll_start, const iqgpu_agc_state *agc_entry)
{
    return seek_impl(c, first_frame, d_preroll, preroll_frames, {SeekKind::DcAgc, true, agc_entry, dc_at_preroll_start, call_frames});
}

// ------------------------------------------------------------------------------------------------
// exact seamless sharding of DC-blocker chains: the map of a call (k_dc_prefix + k_dc_scan's map output), the walk over the maps
// ------------------------------------------------------------------------------------------------
// (Dc and DcRms; the call of a dx / local chain is one piece on the unfused route, which is what dc_measure_call plans for a chain with
//  the AGC: one row)
static int dc_measure_impl(iqgpu_chain *c, uint64_t first_frame, const void *in, size_t frames_in, iqgpu_dc_row *row, bool on_device, SeekKind kind)
{
    const ShardFamily &fam = shard_family(kind);
    const char *who = fam.dc_measure;
    int rc = shard_check(fam, c, who); if (rc) return rc;
    if (!row) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (first_frame > kMaxStreamFrames || (uint64_t)frames_in > kMaxStreamFrames - first_frame) return fail(IQGPU_EINVAL, "%s: stream position "
        "%llu + %zu frames is beyond 2^39 frames", who, (unsigned long long)first_frame, frames_in);
    row->f = 1.0; row->g_re = 0.0; row->g_im = 0.0; row->frames = 0;             // (no frames: the identity)
    if (frames_in == 0) return IQGPU_OK;
    if (!in) return fail(IQGPU_EINVAL, "%s: NULL buffer", who);
    if (c->poisoned) return fail(IQGPU_EHIP, "an earlier call failed half way through: the stream state is undefined until iqgpu_chain_reset()");
    HIP_TRY(hipSetDevice(c->device));
    rc = pipe_advance(c, c->pipe_seq); if (rc) return rc;         // batches submitted earlier come first (same stream)
    rc = c->dc_walk.ensure(64); if (rc) return rc;
    const void *d_in = in;
    if (!on_device) { rc = stage_host_input(c, in, frames_in, &d_in); if (rc) return rc; }
    rc = dc_measure_call(c, stream_at(c, first_frame).pos, d_in, frames_in, (cd2 *)c->dc_walk.p); if (rc) return rc;
    cd2 m[2];
    HIP_TRY(hipMemcpyAsync(m, c->dc_walk.p, sizeof(m), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    row->f = m[0].x; row->g_re = m[1].x; row->g_im = m[1].y; row->frames = (uint64_t)frames_in;
    return IQGPU_OK;
}

extern "C" int iqgpu_chain_dc_measure(iqgpu_chain *c, uint64_t first_frame, const void *raw_in, size_t frames_in, iqgpu_dc_row *row)
{
    return dc_measure_impl(c, first_frame, raw_in, frames_in, row, false, SeekKind::Dc);
}
extern "C" int iqgpu_chain_dc_measure_device(iqgpu_chain *c, uint64_t first_frame, const void *d_raw_in, size_t frames_in, iqgpu_dc_row *row)
{
    return dc_measure_impl(c, first_frame, d_raw_in, frames_in, row, true, SeekKind::Dc);
}
extern "C" int iqgpu_chain_dcrms_dc_measure(iqgpu_chain *c, uint64_t first_frame, const void *raw_in, size_t frames_in, iqgpu_dc_row *row)
{
    return dc_measure_impl(c, first_frame, raw_in, frames_in, row, false, SeekKind::DcRms);
}
extern "C" int iqgpu_chain_dcrms_dc_measure_device(iqgpu_chain *c, uint64_t first_frame, const void *d_raw_in, size_t frames_in, iqgpu_dc_row *row)
{
    return dc_measure_impl(c, first_frame, d_raw_in, frames_in, row, true, SeekKind::DcRms);
}

// One definition of the walk: k_dc_walk applies the helper behind k_dc_scan's state update, in the translation unit of k_dc_scan, a
// batch of 2^16 rows per launch from a scratch copy of *st
static int dc_advance_impl(iqgpu_chain *c, iqgpu_dc_state *st, const iqgpu_dc_row *rows, size_t n, iqgpu_dc_state *before, SeekKind kind)
{
    static_assert(sizeof(iqgpu_dc_row) == sizeof(DcMapRow) && sizeof(DcMapRow) == 32 && sizeof(iqgpu_dc_state) == sizeof(cd2), "DC row layout");
    const ShardFamily &fam = shard_family(kind);
    const char *who = fam.dc_advance;
    int rc = shard_check(fam, c, who); if (rc) return rc;
    if (!st || (n && !rows)) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (!std::isfinite(st->re) || !std::isfinite(st->im)) return fail(IQGPU_EINVAL, "%s: the state is not finite", who);
    for (size_t i = 0; i < n; ++i)
        if (!(rows[i].f > 0.0 && rows[i].f <= 1.0) || !std::isfinite(rows[i].g_re) || !std::isfinite(rows[i].g_im))
            return fail(IQGPU_EINVAL, "%s: row %zu is not a row of iqgpu_chain_dc_measure (f %g, g %g %+gi)", who, i, rows[i].f, rows[i].g_re,
                rows[i].g_im);
    if (n == 0) return IQGPU_OK;
    HIP_TRY(hipSetDevice(c->device));
    constexpr size_t kBatch = (size_t)1 << 16;
    const size_t nb_max = n < kBatch ? n : kBatch;
    // [state][rows x nb_max][before x nb_max]
    rc = c->dc_walk.ensure(64 + nb_max * (sizeof(DcMapRow) + sizeof(cd2))); if (rc) return rc;
    cd2 *d_st = (cd2 *)c->dc_walk.p;
    DcMapRow *d_rows = (DcMapRow *)((char *)c->dc_walk.p + 64);
    cd2 *d_before = (cd2 *)(d_rows + nb_max);
    HIP_TRY(hipMemcpyAsync(d_st, st, sizeof(cd2), hipMemcpyHostToDevice, c->stream));
    for (size_t done = 0; done < n; done += kBatch) {
        const size_t nb = n - done < kBatch ? n - done : kBatch;
        HIP_TRY(hipMemcpyAsync(d_rows, rows + done, nb * sizeof(DcMapRow), hipMemcpyHostToDevice, c->stream));
        DcWalkArgs a{};
        a.rows = d_rows; a.n = (int64_t)nb; a.state = d_st; a.before = before ? d_before : nullptr;
        HIP_TRY(launch_dc_walk(a, c->stream));
        if (before) HIP_TRY(hipMemcpyAsync(before + done, d_before, nb * sizeof(cd2), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    HIP_TRY(hipMemcpy(st, d_st, sizeof(cd2), hipMemcpyDeviceToHost));
    return IQGPU_OK;
}

extern "C" int iqgpu_chain_dc_advance(iqgpu_chain *c, iqgpu_dc_state *st, const iqgpu_dc_row *rows, size_t n, iqgpu_dc_state *before)
{
    return dc_advance_impl(c, st, rows, n, before, SeekKind::Dc);
}
extern "C" int iqgpu_chain_dcagc_dc_advance(iqgpu_chain *c, iqgpu_dc_state *st, const iqgpu_dc_row *rows, size_t n, iqgpu_dc_state *before)
{
    return dc_advance_impl(c, st, rows, n, before, SeekKind::DcAgc);
}
extern "C" int iqgpu_chain_dcrms_dc_advance(iqgpu_chain *c, iqgpu_dc_state *st, const iqgpu_dc_row *rows, size_t n, iqgpu_dc_state *before)
{
    return dc_advance_impl(c, st, rows, n, before, SeekKind::DcRms);
}

// iqgpu_chain_dcagc_dc_measure: the maps of the ordinary call at first_frame, ONE ROW PER PIECE -- the call is cut as
// process_device_impl cuts it there (agc_call_cut with the mirrors' closed form at first_frame), and the single stream rounds its
// state behind each piece, so the two maps of a cut call are not merged
static int dcagc_dc_measure_impl(iqgpu_chain *c, uint64_t first_frame, const void *in, size_t frames_in, iqgpu_dc_row *rows, size_t cap,
                                 size_t *n_rows, bool on_device)
{
    const ShardFamily &fam = shard_family(SeekKind::DcAgc);
    const char *who = fam.dc_measure;
    int rc = shard_check(fam, c, who); if (rc) return rc;
    if (!rows || !n_rows) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    *n_rows = 0;
    if (cap < 2) return fail(IQGPU_EINVAL, "%s: the table holds %zu rows, a call can be two pieces", who, cap);
    if (first_frame > kMaxStreamFrames || (uint64_t)frames_in > kMaxStreamFrames - first_frame) return fail(IQGPU_EINVAL, "%s: stream position "
        "%llu + %zu frames is beyond 2^39 frames", who, (unsigned long long)first_frame, frames_in);
    if (first_frame % (uint64_t)c->agc_chunk) return fail(IQGPU_EINVAL, "%s: first_frame %llu is not a multiple of agc_chunk_frames = %lld",
        who, (unsigned long long)first_frame, (long long)c->agc_chunk);
    if (frames_in == 0) return IQGPU_OK;
    if (!in) return fail(IQGPU_EINVAL, "%s: NULL buffer", who);
    if (c->poisoned) return fail(IQGPU_EHIP, "an earlier call failed half way through: the stream state is undefined until iqgpu_chain_reset()");
    HIP_TRY(hipSetDevice(c->device));
    rc = pipe_advance(c, c->pipe_seq); if (rc) return rc;         // batches submitted earlier come first (same stream)
    rc = c->dc_walk.ensure(64); if (rc) return rc;
    const void *d_in = in;
    if (!on_device) { rc = stage_host_input(c, in, frames_in, &d_in); if (rc) return rc; }
    // the pieces: [0, head) in front of the lock, [head, frames_in) behind it; a chain that never cuts runs the call whole, unfused
    size_t head = frames_in;
    if (c->agc_fusable || c->agc_fusable_filter) {
        bool locked = false, locks = false; uint64_t seen = 0;
        agc_mirrors_at(c, first_frame, &locked, &seen);
        head = agc_call_cut(c, locked, seen, stream_at(c, first_frame).pos, frames_in, &locks);
    }
    const size_t ibps = bytes_per_frame(c->desc.in_format);
    const size_t len[2] = {head, frames_in - head};
    size_t n = 0;
    for (int k = 0; k < 2; ++k) {
        if (len[k] == 0) continue;
        const size_t off = k ? head : 0;
        rc = dc_measure_call(c, stream_at(c, first_frame + off).pos, (const char *)d_in + off * ibps, len[k], (cd2 *)c->dc_walk.p + 2 * n, k == 1);
        if (rc) return rc;
        rows[n].frames = (uint64_t)len[k];
        ++n;
    }
    cd2 m[4];
    HIP_TRY(hipMemcpyAsync(m, c->dc_walk.p, sizeof(cd2) * 2 * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; ++i) { rows[i].f = m[2 * i].x; rows[i].g_re = m[2 * i + 1].x; rows[i].g_im = m[2 * i + 1].y; }
    *n_rows = n;
    return IQGPU_OK;
}

extern "C" int iqgpu_chain_dcagc_dc_measure(iqgpu_chain *c, uint64_t first_frame, const void *raw_in, size_t frames_in, iqgpu_dc_row *rows,
                                            size_t cap, size_t *n_rows)
{
    return dcagc_dc_measure_impl(c, first_frame, raw_in, frames_in, rows, cap, n_rows, false);
}
extern "C" int iqgpu_chain_dcagc_dc_measure_device(iqgpu_chain *c, uint64_t first_frame, const void *d_raw_in, size_t frames_in,
                                                   iqgpu_dc_row *rows, size_t cap, size_t *n_rows)
{
    return dcagc_dc_measure_impl(c, first_frame, d_raw_in, frames_in, rows, cap, n_rows, true);
}

// ------------------------------------------------------------------------------------------------
// iqgpu_chain_*_dc_measure_range: pass 1 of the three exact recipes over a whole range in ONE submission.  Every piece of every grid
// call is planned up front by the planning of the per-call form (dc_measure_plan: host arithmetic), the plans go to the device as one
// table, k_dc_prefix_batch / k_dc_scan_batch run the per-call kernels' device functions over kDcBatchEntries entries per launch, the
// maps of all pieces come back in one copy behind one synchronisation.  The handle is read, never moved.
// ------------------------------------------------------------------------------------------------
constexpr size_t kDcRangeSliceFrames = (size_t)1 << 24;     // the host variants' staging slice (whole calls, at least one): 64 MiB of cs16
constexpr int64_t kDcBatchSegments = (int64_t)1 << 22;      // aggregates of one launch (dc_agg: 32 MiB); an entry beyond it starts the next launch

extern "C" size_t iqgpu_dc_measure_range_launch_entries(void) { return (size_t)kDcBatchEntries; }

namespace {
struct RangePiece { size_t off, len; bool past_lock; };                     // frames from the range's first frame
struct RangeLaunch { size_t e0, n; int max_seg; size_t slice; };            // entries [e0, e0 + n) of the table, all of one slice
struct RangeSlice { size_t off, len; };                                     // host variants: the frames of one staging slice
}

static int dc_measure_range_run(iqgpu_chain *c, const char *who, uint64_t first_frame, const void *in, bool on_device,
                                const std::vector<RangePiece> &pieces, const std::vector<RangeSlice> &slices, iqgpu_dc_row *rows)
{
    const size_t ibps = bytes_per_frame(c->desc.in_format), n_ent = pieces.size();
    int rc;
    if (!on_device) {
        size_t most = 0;
        for (const RangeSlice &sl : slices) most = sl.len > most ? sl.len : most;
        for (size_t b = 0; b < 2 && b < slices.size(); ++b) { rc = c->dc_range_in[b].ensure(most * ibps); if (rc) return rc; }
        HIP_TRY(c->dc_range_h2d.create());                               // (on first use: create() keeps a handle it holds)
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(c->dc_range_in_done[b].create(hipEventDisableTiming));
            HIP_TRY(c->dc_range_k_done[b].create(hipEventDisableTiming));
        }
    }
    // where slice s lies on the device, and the table: every piece planned from the address its frames will have
    auto slice_base = [&](size_t s) { return on_device ? (const char *)in : (const char *)c->dc_range_in[s & 1].p; };
    std::vector<DcBatchEntry> tab(n_ent);
    std::vector<RangeLaunch> launches;
    int64_t most_agg = 0, agg = 0;
    size_t s = 0;
    for (size_t e = 0; e < n_ent; ++e) {
        const RangePiece &pc = pieces[e];
        while (pc.off >= slices[s].off + slices[s].len) ++s;
        const size_t raw_off = (pc.off - slices[s].off) * ibps;
        const DcMeasurePlan mp = dc_measure_plan(c, stream_at(c, first_frame + (uint64_t)pc.off).pos, slice_base(s) + raw_off, pc.len, pc.past_lock);
        if (launches.empty() || launches.back().slice != s || launches.back().n == (size_t)kDcBatchEntries || agg + mp.geom.n_seg > kDcBatchSegments) {
            launches.push_back(RangeLaunch{e, 0, 1, s});
            agg = 0;
        }
        tab[e].geom = mp.geom; tab[e].raw_off = (int64_t)raw_off; tab[e].raw_aligned = mp.raw_aligned; tab[e].agg_off = (int32_t)agg;
        agg += mp.geom.n_seg;
        if (agg > most_agg) most_agg = agg;
        RangeLaunch &l = launches.back();
        ++l.n;
        if (mp.geom.n_seg > l.max_seg) l.max_seg = mp.geom.n_seg;
    }
    rc = c->dc_agg.ensure((size_t)most_agg * sizeof(cf2)); if (rc) return rc;
    rc = c->dc_range_tab.ensure(n_ent * sizeof(DcBatchEntry)); if (rc) return rc;
    rc = c->dc_range_map.ensure(n_ent * 2 * sizeof(cd2)); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->dc_range_tab.p, tab.data(), n_ent * sizeof(DcBatchEntry), hipMemcpyHostToDevice, c->stream));

    auto copy_slice = [&](size_t k) {
        const hipError_t e = hipMemcpyAsync(c->dc_range_in[k & 1].p, (const char *)in + slices[k].off * ibps, slices[k].len * ibps,
                                            hipMemcpyHostToDevice, c->dc_range_h2d);
        return e != hipSuccess ? e : hipEventRecord(c->dc_range_in_done[k & 1], c->dc_range_h2d);
    };
    // the host variants: the copy of slice k + 1 is queued -- once the kernels of slice k - 1, which read its buffer, are done -- before
    // the host waits for slice k's copy and queues its kernels (host-ordered, as the pipeline is: no stream waits on another)
    if (!on_device) HIP_TRY(copy_slice(0));
    size_t li = 0;
    for (size_t k = 0; k < slices.size(); ++k) {
        if (!on_device) {
            if (k + 1 < slices.size()) {
                if (k >= 1) HIP_TRY(hipEventSynchronize(c->dc_range_k_done[(k + 1) & 1]));
                HIP_TRY(copy_slice(k + 1));
            }
            HIP_TRY(hipEventSynchronize(c->dc_range_in_done[k & 1]));
        }
        for (; li < launches.size() && launches[li].slice == k; ++li) {
            const RangeLaunch &l = launches[li];
            const DcBatchEntry *d_tab = (const DcBatchEntry *)c->dc_range_tab.p + l.e0;
            DcPrefixBatchArgs pa{};
            pa.raw = slice_base(k); pa.in_fmt = c->desc.in_format; pa.gain = c->desc.gain; pa.c = c->dc_c; pa.logc = c->dc_logc;
            pa.entries = d_tab; pa.agg = (cf2 *)c->dc_agg.p;
            HIP_TRY(launch_dc_prefix_batch(pa, (int)l.n, l.max_seg, c->stream));
            DcScanBatchArgs sa{};
            sa.entries = d_tab; sa.agg = (const cf2 *)c->dc_agg.p; sa.logc = c->dc_logc; sa.map = (cd2 *)c->dc_range_map.p + 2 * l.e0;
            HIP_TRY(launch_dc_scan_batch(sa, (int)l.n, c->stream));
        }
        if (!on_device) HIP_TRY(hipEventRecord(c->dc_range_k_done[k & 1], c->stream));
    }
    if (li != launches.size()) return fail(IQGPU_EINVAL, "internal: %s planned %zu launches and queued %zu", who, launches.size(), li);
    std::vector<cd2> m(2 * n_ent);
    HIP_TRY(hipMemcpyAsync(m.data(), c->dc_range_map.p, m.size() * sizeof(cd2), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t e = 0; e < n_ent; ++e) {
        rows[e].f = m[2 * e].x; rows[e].g_re = m[2 * e + 1].x; rows[e].g_im = m[2 * e + 1].y; rows[e].frames = (uint64_t)pieces[e].len;
    }
    return IQGPU_OK;
}

// (all three families: Dc and DcRms give one row per call; DcAgc -- the family whose preroll runs as shadow calls -- cuts every call as
//  iqgpu_chain_dcagc_dc_measure cuts it, one row per piece)
static int dc_measure_range_impl(iqgpu_chain *c, uint64_t first_frame, const void *in, size_t frames_in, size_t call_frames, iqgpu_dc_row *rows,
                                 size_t cap, size_t *n_rows, uint32_t *first_row, bool on_device, SeekKind kind)
{
    const ShardFamily &fam = shard_family(kind);
    const char *who = fam.dc_measure_range;
    int rc = shard_check(fam, c, who); if (rc) return rc;
    if (!rows || !n_rows) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    *n_rows = 0;
    const bool cuts = fam.preroll_agc == AgcMode::Shadow;
    if (call_frames == 0 || call_frames % 4096) return fail(IQGPU_EINVAL, "%s: call_frames %zu is not a non-zero multiple of 4096", who, call_frames);
    if (cuts && (call_frames % (size_t)c->agc_chunk || first_frame % (uint64_t)c->agc_chunk)) return fail(IQGPU_EINVAL, "%s: first_frame %llu and "
        "call_frames %zu have to be multiples of agc_chunk_frames = %lld", who, (unsigned long long)first_frame, call_frames, (long long)c->agc_chunk);
    if (first_frame % (uint64_t)call_frames) return fail(IQGPU_EINVAL, "%s: first_frame %llu is not on the grid of calls of %zu frames", who,
        (unsigned long long)first_frame, call_frames);
    if (first_frame > kMaxStreamFrames || (uint64_t)frames_in > kMaxStreamFrames - first_frame) return fail(IQGPU_EINVAL, "%s: stream position "
        "%llu + %zu frames is beyond 2^39 frames", who, (unsigned long long)first_frame, frames_in);
    if (frames_in == 0) return IQGPU_OK;
    // the pieces of every grid call, in stream order
    const size_t n_calls = (frames_in + call_frames - 1) / call_frames;
    const bool may_cut = cuts && (c->agc_fusable || c->agc_fusable_filter);
    std::vector<RangePiece> pieces;
    std::vector<uint32_t> first(n_calls);
    pieces.reserve(n_calls + 1);
    for (size_t k = 0; k < n_calls; ++k) {
        const size_t off = k * call_frames, len = frames_in - off < call_frames ? frames_in - off : call_frames;
        size_t head = len;
        if (may_cut) {
            bool locked = false, locks = false; uint64_t seen = 0;
            agc_mirrors_at(c, first_frame + (uint64_t)off, &locked, &seen);
            head = agc_call_cut(c, locked, seen, stream_at(c, first_frame + (uint64_t)off).pos, len, &locks);
        }
        first[k] = (uint32_t)pieces.size();
        if (head > 0) pieces.push_back(RangePiece{off, head, false});
        if (head < len) pieces.push_back(RangePiece{off + head, len - head, true});
    }
    *n_rows = pieces.size();
    if (cap < pieces.size()) return fail(IQGPU_ECAPACITY, "%s: %zu calls are %zu rows, the table holds %zu", who, n_calls, pieces.size(), cap);
    *n_rows = 0;
    if (!in) return fail(IQGPU_EINVAL, "%s: NULL buffer", who);
    if (c->poisoned) return fail(IQGPU_EHIP, "an earlier call failed half way through: the stream state is undefined until iqgpu_chain_reset()");
    HIP_TRY(hipSetDevice(c->device));
    rc = pipe_advance(c, c->pipe_seq); if (rc) return rc;         // batches submitted earlier come first (same stream)
    // the host variants' slices: whole calls; the _device variants read the range where it lies (one "slice")
    std::vector<RangeSlice> slices;
    if (on_device) slices.push_back(RangeSlice{0, frames_in});
    else {
        const size_t want = c->sw.dc_range_slice_frames > 0 ? (size_t)c->sw.dc_range_slice_frames : kDcRangeSliceFrames;
        const size_t per = (want / call_frames ? want / call_frames : 1) * call_frames;
        for (size_t off = 0; off < frames_in; off += per) slices.push_back(RangeSlice{off, frames_in - off < per ? frames_in - off : per});
    }
    rc = dc_measure_range_run(c, who, first_frame, in, on_device, pieces, slices, rows);
    if (rc) {
        // (whatever was queued reads host vectors of this call and the caller's buffer: nothing of it outlives the call)
        (void)hipStreamSynchronize(c->stream);
        if (c->dc_range_h2d) (void)hipStreamSynchronize(c->dc_range_h2d);
        return rc;
    }
    if (first_row) memcpy(first_row, first.data(), n_calls * sizeof(uint32_t));
    *n_rows = pieces.size();
    return IQGPU_OK;
}

extern "C" int iqgpu_chain_dc_measure_range(iqgpu_chain *c, uint64_t first_frame, const void *raw_in, size_t frames_in, size_t call_frames,
                                            iqgpu_dc_row *rows, size_t cap, size_t *n_rows, uint32_t *first_row)
{
    return dc_measure_range_impl(c, first_frame, raw_in, frames_in, call_frames, rows, cap, n_rows, first_row, false, SeekKind::Dc);
}
extern "C" int iqgpu_chain_dc_measure_range_device(iqgpu_chain *c, uint64_t first_frame, const void *d_raw_in, size_t frames_in, size_t call_frames,
                                                   iqgpu_dc_row *rows, size_t cap, size_t *n_rows, uint32_t *first_row)
{
    return dc_measure_range_impl(c, first_frame, d_raw_in, frames_in, call_frames, rows, cap, n_rows, first_row, true, SeekKind::Dc);
}
extern "C" int iqgpu_chain_dcagc_dc_measure_range(iqgpu_chain *c, uint64_t first_frame, const void *raw_in, size_t frames_in, size_t call_frames,
                                                  iqgpu_dc_row *rows, size_t cap, size_t *n_rows, uint32_t *first_row)
{
    return dc_measure_range_impl(c, first_frame, raw_in, frames_in, call_frames, rows, cap, n_rows, first_row, false, SeekKind::DcAgc);
}
extern "C" int iqgpu_chain_dcagc_dc_measure_range_device(iqgpu_chain *c, uint64_t first_frame, const void *d_raw_in, size_t frames_in, size_t call_frames,
                                                         iqgpu_dc_row *rows, size_t cap, size_t *n_rows, uint32_t *first_row)
{
    return dc_measure_range_impl(c, first_frame, d_raw_in, frames_in, call_frames, rows, cap, n_rows, first_row, true, SeekKind::DcAgc);
}
extern "C" int iqgpu_chain_dcrms_dc_measure_range(iqgpu_chain *c, uint64_t first_frame, const void *raw_in, size_t frames_in, size_t call_frames,
                                                  iqgpu_dc_row *rows, size_t cap, size_t *n_rows, uint32_t *first_row)
{
    return dc_measure_range_impl(c, first_frame, raw_in, frames_in, call_frames, rows, cap, n_rows, first_row, false, SeekKind::DcRms);
}
extern "C" int iqgpu_chain_dcrms_dc_measure_range_device(iqgpu_chain *c, uint64_t first_frame, const void *d_raw_in, size_t frames_in, size_t call_frames,
                                                         iqgpu_dc_row *rows, size_t cap, size_t *n_rows, uint32_t *first_row)
{
    return dc_measure_range_impl(c, first_frame, d_raw_in, frames_in, call_frames, rows, cap, n_rows, first_row, true, SeekKind::DcRms);
}

// ------------------------------------------------------------------------------------------------
// seamless sharding of digital-AGC chains (ABI v8): the measure pass, and the walk over its tables
// ------------------------------------------------------------------------------------------------
// Which route a measuring call takes (chain.hpp, AgcMode): the faster one measured per shape (tools/bench_measure.py, DESIGN 5.1,
// 2^28 frames).  Chains without a half-band stage (the cu8-nrsc5 presets: one output per 1.6 input frames, so the cf32 stream of the
// unfused route is its largest) take k_front_s1<.., AGC>: 0.665 ms against 0.747.  With a half-band stage the unfused route wins
// (NRSC-5 cs16: 0.576 against 0.655); cascades were not timed and keep it.  The "measure_route" switch overrides.
AgcMode measure_route(const iqgpu_chain *c)
{
    const bool s1 = c->agc_fusable && (c->sw.measure_route == 1 || (c->sw.measure_route < 0 && c->S == 0 && !c->cascade));
    return s1 ? AgcMode::MeasureS1 : AgcMode::Measure;
}

// (Agc and DcAgc; the family whose preroll runs as shadow calls measures as one: the call cut and planned as the ordinary call at the
//  chain's position, chain.hpp AgcMode::Shadow)
static int measure_impl(iqgpu_chain *c, const void *in, size_t frames_in, iqgpu_agc_chunk *rows, size_t cap, size_t *n_rows, bool on_device,
                        SeekKind kind)
{
    static_assert(sizeof(iqgpu_agc_chunk) == sizeof(AgcRow) && sizeof(AgcRow) == 16, "AGC row layout");
    const ShardFamily &fam = shard_family(kind);
    const char *who = fam.measure;
    int rc = shard_check(fam, c, who); if (rc) return rc;
    if (!n_rows) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    *n_rows = 0;
    if (frames_in == 0) return IQGPU_OK;
    if (!in || !rows) return fail(IQGPU_EINVAL, "%s: NULL buffer", who);
    const size_t n = (frames_in + (size_t)c->agc_chunk - 1) / (size_t)c->agc_chunk;
    if (cap < n) return fail(IQGPU_ECAPACITY, "%s: %zu frames are %zu chunks, the table holds %zu rows", who, frames_in, n, cap);
    HIP_TRY(hipSetDevice(c->device));
    rc = pipe_advance(c, c->pipe_seq); if (rc) return rc;         // batches submitted earlier come first (same stream)
    rc = agc_resolve_pending(c); if (rc) return rc;
    const void *d_in = in;
    if (!on_device) { rc = stage_host_input(c, in, frames_in, &d_in); if (rc) return rc; }
    size_t dropped = 0;
    CallOpts mo; mo.agc = fam.preroll_agc == AgcMode::Shadow ? AgcMode::Shadow : measure_route(c); mo.no_probe = true;      // (a pass whose output nobody keeps: nothing for the I/Q optimiser)
    rc = process_device_impl(c, d_in, frames_in, nullptr, 0, &dropped, mo);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(rows, c->agc_rows.p, n * sizeof(AgcRow), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *n_rows = n;
    return IQGPU_OK;
}

extern "C" int iqgpu_chain_measure(iqgpu_chain *c, const void *raw_in, size_t frames_in, iqgpu_agc_chunk *rows, size_t cap, size_t *n_rows)
{
    return measure_impl(c, raw_in, frames_in, rows, cap, n_rows, false, SeekKind::Agc);
}
extern "C" int iqgpu_chain_measure_device(iqgpu_chain *c, const void *d_raw_in, size_t frames_in, iqgpu_agc_chunk *rows, size_t cap,
                                          size_t *n_rows)
{
    return measure_impl(c, d_raw_in, frames_in, rows, cap, n_rows, true, SeekKind::Agc);
}

extern "C" int iqgpu_chain_dcagc_measure(iqgpu_chain *c, const void *raw_in, size_t frames_in, iqgpu_agc_chunk *rows, size_t cap, size_t *n_rows)
{
    return measure_impl(c, raw_in, frames_in, rows, cap, n_rows, false, SeekKind::DcAgc);
}
extern "C" int iqgpu_chain_dcagc_measure_device(iqgpu_chain *c, const void *d_raw_in, size_t frames_in, iqgpu_agc_chunk *rows, size_t cap,
                                                size_t *n_rows)
{
    return measure_impl(c, d_raw_in, frames_in, rows, cap, n_rows, true, SeekKind::DcAgc);
}

extern "C" int iqgpu_chain_agc_initial_state(const iqgpu_chain *c, iqgpu_agc_state *st)
{
    if (!c || !st) return fail(IQGPU_EINVAL, "iqgpu_chain_agc_initial_state: NULL argument");
    if (!c->agc) return fail(IQGPU_EINVAL, "iqgpu_chain_agc_initial_state: the chain has no output AGC");
    AgcState s0 = c->agc_init;
    if (c->desc.agc_clock != IQGPU_AGC_CLOCK_WALL) s0.last_strong = 0.0;
    memcpy(st, &s0, sizeof(s0));
    return IQGPU_OK;
}

// One definition of the walk: the tables go to device memory and k_agc_scan -- the kernel behind every unfused call -- walks them
// from a scratch copy of *st, a batch of 2^20 rows per launch (the kernel's chunk index is 32-bit; a whole stream of 2^39 frames
// can hold 2^25 rows).  The kernel carries its state from launch to launch exactly as from call to call.
extern "C" int iqgpu_chain_agc_advance(iqgpu_chain *c, iqgpu_agc_state *st, const iqgpu_agc_chunk *rows, size_t n, float *gains)
{
    int rc = two_pass_check(c, "iqgpu_chain_agc_advance", kNeedAgc); if (rc) return rc;
    if (!st || (n && !rows)) return fail(IQGPU_EINVAL, "iqgpu_chain_agc_advance: NULL argument");
    if (n == 0) return IQGPU_OK;
    // (k_agc_scan adds the lengths of the 64 rows of a batch in 32 bits: the bound chain_create puts on agc_chunk_frames, here on
    //  any 64 consecutive rows of a table the caller may have built)
    uint64_t window = 0;
    for (size_t i = 0; i < n; ++i) {
        if (rows[i].frames_out > 0x7fffffffu || !(rows[i].peak2 >= 0.0)) return fail(IQGPU_EINVAL, "iqgpu_chain_agc_advance: row %zu is "
            "not a row of iqgpu_chain_measure (frames_out %u, peak2 %g)", i, rows[i].frames_out, rows[i].peak2);
        window += rows[i].frames_out;
        if (i >= 64) window -= rows[i - 64].frames_out;
        if (window >= 0x80000000ull) return fail(IQGPU_EINVAL, "iqgpu_chain_agc_advance: the 64 rows that end at row %zu hold %llu "
            "frames (64 consecutive rows must stay below 2^31)", i, (unsigned long long)window);
    }
    HIP_TRY(hipSetDevice(c->device));
    constexpr size_t kBatch = (size_t)1 << 20;
    const size_t nb_max = n < kBatch ? n : kBatch;
    // [state][peak2 x nb_max][len x nb_max][gain x nb_max]
    rc = c->agc_walk.ensure(64 + nb_max * (sizeof(unsigned long long) + sizeof(int32_t) + sizeof(float))); if (rc) return rc;
    AgcState *d_st = (AgcState *)c->agc_walk.p;
    unsigned long long *d_p2 = (unsigned long long *)((char *)c->agc_walk.p + 64);
    int32_t *d_len = (int32_t *)(d_p2 + nb_max);
    float *d_gain = (float *)(d_len + nb_max);
    std::vector<unsigned long long> h_p2(nb_max);
    std::vector<int32_t> h_len(nb_max);
    HIP_TRY(hipMemcpyAsync(d_st, st, sizeof(AgcState), hipMemcpyHostToDevice, c->stream));
    for (size_t done = 0; done < n; done += kBatch) {
        const size_t nb = n - done < kBatch ? n - done : kBatch;
        for (size_t i = 0; i < nb; ++i) {
            memcpy(&h_p2[i], &rows[done + i].peak2, sizeof(double));
            h_len[i] = (int32_t)rows[done + i].frames_out;
        }
        HIP_TRY(hipMemcpyAsync(d_p2, h_p2.data(), nb * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_len, h_len.data(), nb * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        AgcArgs a{};
        a.geom.n_chunks = (int32_t)nb;
        a.peak2 = d_p2; a.chunk_len = d_len; a.gain = d_gain; a.state = d_st;
        a.target = c->agc_target; a.rate = c->target_rate;
        HIP_TRY(launch_agc_walk(a, c->stream));
        if (gains) HIP_TRY(hipMemcpyAsync(gains + done, d_gain, nb * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));             // (the staging vectors are reused by the next batch)
    }
    HIP_TRY(hipMemcpy(st, d_st, sizeof(AgcState), hipMemcpyDeviceToHost));
    return IQGPU_OK;
}
