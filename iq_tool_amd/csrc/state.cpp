// state.cpp -- checkpoint / resume: everything a chain carries from call to call into a caller-owned blob and back
// (iqgpu_chain_save_state / _load_state, iqgpu.h), the position counters behind it (iqgpu_chain_tell), the blob's size without a
// device (iqgpu_design_state_size).  The container -- header, checksum, iqgpu_state_inspect -- is state_blob.cpp.
#include "chain.hpp"
#include "state_blob.hpp"

// ------------------------------------------------------------------------------------------------
// layout: [StateHeader][StateWords][d_hist][d_hist2][filter front][k_interp front][agc_hist], every section rounded up to 16 bytes and
// present at its maximum length whatever the state (absent stages: zero length) -- the size is a function of the design
// ------------------------------------------------------------------------------------------------
struct StateWords {                  // what the chain keeps on the host, and the two small device states
    int32_t  rem, agc_locked;
    uint32_t nco_theta, pnco_theta;
    uint64_t phi, fpending, agc_seen, agc_rms_pos;
    float    iq_mag, iq_phase;
    uint64_t pad0;
    cd2      dc;                     // zero without the blocker
    AgcState agc;                    // zero without the AGC
    uint64_t pad1[2];
};
static_assert(sizeof(StateWords) == 128 && sizeof(AgcState) == 32 && sizeof(cd2) == 16, "state words layout");

struct StateLayout {
    size_t n_hist = 0, n_hist2 = 0, n_fbuf = 0, n_ibuf = 0, n_agc_hist = 0;           // cf2 samples, at their maximum
    size_t o_words = 0, o_hist = 0, o_hist2 = 0, o_fbuf = 0, o_ibuf = 0, o_agc_hist = 0, total = 0;
};

static int64_t agc_rms_warm_of(const iqgpu_chain *c)      // (a created chain keeps it in agc_rms_warm; a designed one has not got that far)
{
    if (!c->agc || !(c->agc_rms_alpha > 0.0f)) return 0;
    int64_t chunk = 0, warm = 0; int32_t nch = 0;
    agc_rms_geometry(c->agc_rms_alpha, 0, 0, &chunk, &warm, &nch);
    return warm;
}

static StateLayout state_layout(const iqgpu_chain *c)
{
    StateLayout l;
    if (c->decim) { l.n_hist = (size_t)c->hist_cap; if (c->cascade) l.n_hist2 = (size_t)c->hist2_cap; }
    // [L-1 history][pending], pending < block (plan_call_at; no block: none)
    if (c->fp.enabled) l.n_fbuf = c->fp.taps.size() - 1 + (size_t)c->fp.block;
    if (c->late) l.n_ibuf = (size_t)c->ihist;
    l.n_agc_hist = (size_t)agc_rms_warm_of(c);
    auto r16 = [](size_t n) { return (n + 15) & ~(size_t)15; };
    size_t o = sizeof(StateHeader);
    l.o_words = o; o += sizeof(StateWords);
    l.o_hist = o; o += r16(l.n_hist * sizeof(cf2));
    l.o_hist2 = o; o += r16(l.n_hist2 * sizeof(cf2));
    l.o_fbuf = o; o += r16(l.n_fbuf * sizeof(cf2));
    l.o_ibuf = o; o += r16(l.n_ibuf * sizeof(cf2));
    l.o_agc_hist = o; o += r16(l.n_agc_hist * sizeof(cf2));
    l.total = o;
    return l;
}

// Everything the layout and the meaning of the contents depend on: the description's fields that shape the design, what the design
// derived from them, the chain's switch snapshot (routing decides the history layouts and the roundings behind them).  Not the I/Q
// factors (they travel in the blob), not the device, the stream or profiling.
static uint64_t state_fingerprint(const iqgpu_chain *c)
{
    Hash64 k;
    const iqgpu_chain_desc &d = c->desc;
    k.word((uint64_t)IQGPU_STATE_FORMAT_VERSION);
    k.word((uint64_t)(uint32_t)d.in_format); k.word((uint64_t)(uint32_t)d.out_format); k.f32(d.gain);
    k.word((uint64_t)(d.dc_block_enable != 0)); k.word((uint64_t)(d.iq_correct_enable != 0)); k.word((uint64_t)(d.no_resample != 0));
    k.word((uint64_t)(d.shift_after_resample != 0)); k.word((uint64_t)d.block_samples);
    // ratio, rates and the operator constants derived from them
    k.f32(c->ratio); k.f64(c->target_rate); k.word((uint64_t)c->resample); k.word((uint64_t)c->decim); k.word((uint64_t)c->late);
    k.f32(c->dc_alpha); k.f32(c->dc_c);
    k.word((uint64_t)(uint32_t)c->nco_mode); k.word((uint64_t)(uint32_t)c->pnco_mode); k.word((uint64_t)c->nco_dtheta);
    // the half-band plan and the polyphase step
    k.word((uint64_t)c->S); k.word((uint64_t)c->rp.S); k.word((uint64_t)c->rp.interp); k.word((uint64_t)c->rp.step); k.f32(c->rp.rate_arb);
    k.word((uint64_t)c->rp.history_in);
    for (const HalfbandStage &st : c->rp.stages) { k.word((uint64_t)st.m); if (!st.branch.empty()) k.bytes(st.branch.data(), st.branch.size() * sizeof(float)); }
    k.word((uint64_t)c->cascade); k.word((uint64_t)c->casc_warm);
    // the user filter
    k.word((uint64_t)c->fp.enabled); k.word((uint64_t)c->fp.post_resample); k.word((uint64_t)c->fp.is_complex); k.word((uint64_t)c->fp.impl);
    k.word((uint64_t)c->fp.block); k.word((uint64_t)c->fp.taps.size());
    if (!c->fp.taps.empty()) k.bytes(c->fp.taps.data(), c->fp.taps.size() * sizeof(cfloat));
    // the output AGC
    k.word((uint64_t)c->agc);
    if (c->agc) { k.word((uint64_t)(uint32_t)d.agc_profile); k.word((uint64_t)(uint32_t)d.agc_clock); k.f32(c->agc_target);
                  k.word((uint64_t)c->agc_chunk); k.f32(c->agc_rms_alpha); }
    // the sizes of the blob's sections
    const StateLayout l = state_layout(c);
    k.word(l.n_hist); k.word(l.n_hist2); k.word(l.n_fbuf); k.word(l.n_ibuf); k.word(l.n_agc_hist);
    // the switch snapshot
    const DebugSwitches &s = c->sw;
    k.word((uint64_t)s.force_generic); k.word((uint64_t)s.dbg); k.word((uint64_t)(uint32_t)s.tap_fold);
    k.word((uint64_t)s.steal); k.word((uint64_t)(uint32_t)s.steal_min); k.word((uint64_t)(uint32_t)s.steal_rounds);
    k.word((uint64_t)(uint32_t)s.steal_stride); k.word((uint64_t)(uint32_t)s.steal_lanes);
    for (int i = 0; i < 4; ++i) k.word((uint64_t)(uint32_t)s.run_wt[i]);
    k.word((uint64_t)s.nco_hold); k.word((uint64_t)(uint32_t)s.cus); k.word((uint64_t)(uint32_t)s.fft_log2n); k.word((uint64_t)(uint32_t)s.fft_threads);
    k.word((uint64_t)s.fft_keep_geometry); k.word((uint64_t)(uint32_t)s.measure_route); k.word((uint64_t)(uint32_t)s.casc2_min_run);
    return k.h;
}

extern "C" int iqgpu_design_state_size(const iqgpu_chain_desc *d, size_t *bytes)
{
    if (!d || !bytes) return fail(IQGPU_EINVAL, "iqgpu_design_state_size: NULL argument");
    *bytes = 0;
    iqgpu_chain *c = new (std::nothrow) iqgpu_chain();
    if (!c) return fail(IQGPU_ENOMEM, "out of host memory");
    const int rc = design_chain(c, d);
    if (rc == IQGPU_OK) *bytes = state_layout(c).total;
    delete c;
    return rc;
}

// ------------------------------------------------------------------------------------------------
// iqgpu_chain_tell: the position behind every batch already submitted (what submit has promised: pipe_rem / pipe_phi)
// ------------------------------------------------------------------------------------------------
extern "C" int iqgpu_chain_tell(iqgpu_chain *c, uint64_t *frames_in, uint64_t *frames_out)
{
    if (!c || !frames_in || !frames_out) return fail(IQGPU_EINVAL, "iqgpu_chain_tell: NULL argument");
    const bool ahead = c->pipe_launched < c->pipe_seq;
    *frames_in = ahead ? c->pipe_total_in : c->total_in;
    *frames_out = ahead ? c->pipe_total_out : c->total_out;
    return IQGPU_OK;
}

// ------------------------------------------------------------------------------------------------
// iqgpu_chain_save_state: the stream made final as iqgpu_chain_get_agc_state makes it, then device-to-host copies of what the
// kernels keep -- logical contents only: which buffer of a pair is current (hist_cur, fcur, icur) does not reach the blob
// ------------------------------------------------------------------------------------------------
extern "C" int iqgpu_chain_save_state(iqgpu_chain *c, void *blob, size_t cap, size_t *bytes)
{
    const char *who = "iqgpu_chain_save_state";
    if (!c || !bytes) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    const StateLayout l = state_layout(c);
    *bytes = l.total;
    if (cap < l.total) return fail(IQGPU_ECAPACITY, "%s: the state of this chain is %zu bytes, the buffer holds %zu", who, l.total, cap);
    if (!blob) return fail(IQGPU_EINVAL, "%s: NULL blob", who);
    if (c->agc && c->desc.agc_clock == IQGPU_AGC_CLOCK_WALL) return fail(IQGPU_EUNSUPPORTED, "%s: the AGC state of an IQGPU_AGC_CLOCK_WALL "
        "chain holds a monotonic clock reading, which has no meaning in another process; use IQGPU_AGC_CLOCK_SAMPLES", who);
    if (c->poisoned) return fail(IQGPU_EHIP, "an earlier call failed half way through: the stream state is undefined until iqgpu_chain_reset()");
    HIP_TRY(hipSetDevice(c->device));
    { const int rc = pipe_advance(c, c->pipe_seq); if (rc) return rc; }     // batches submitted and not yet collected
    { const int rc = agc_resolve_pending(c); if (rc) return rc; }
    HIP_TRY(hipStreamSynchronize(c->stream));

    char *b = (char *)blob;
    memset(b, 0, l.total);                                     // (unused tails and every padding byte)
    StateWords w;
    memset(&w, 0, sizeof(w));
    w.rem = c->rem; w.phi = c->phi; w.nco_theta = c->nco_theta; w.pnco_theta = c->pnco_theta; w.fpending = c->fpending;
    { std::lock_guard<std::mutex> g(c->aux_mu); w.iq_mag = c->iq_mag; w.iq_phase = c->iq_phase; }
    if (c->dc) HIP_TRY(hipMemcpy(&w.dc, c->d_dc_state, sizeof(cd2), hipMemcpyDeviceToHost));
    if (c->agc) {
        HIP_TRY(hipMemcpy(&w.agc, c->d_agc_state, sizeof(AgcState), hipMemcpyDeviceToHost));
        w.agc_locked = c->agc_locked_host ? 1 : 0; w.agc_seen = c->agc_seen_host; w.agc_rms_pos = c->agc_rms_pos;
    }
    memcpy(b + l.o_words, &w, sizeof(w));
    if (l.n_hist) HIP_TRY(hipMemcpy(b + l.o_hist, c->d_hist[c->hist_cur], l.n_hist * sizeof(cf2), hipMemcpyDeviceToHost));
    if (l.n_hist2) HIP_TRY(hipMemcpy(b + l.o_hist2, c->d_hist2[c->hist2_cur], l.n_hist2 * sizeof(cf2), hipMemcpyDeviceToHost));
    if (l.n_fbuf) {
        const size_t front = c->fp.taps.size() - 1 + (size_t)c->fpending;
        if (front > l.n_fbuf) return fail(IQGPU_EINVAL, "internal: %llu pending filter samples with a block of %u", (unsigned long long)c->fpending, c->fp.block);
        if (front) HIP_TRY(hipMemcpy(b + l.o_fbuf, c->fbuf[c->fcur].p, front * sizeof(cf2), hipMemcpyDeviceToHost));
    }
    if (l.n_ibuf) HIP_TRY(hipMemcpy(b + l.o_ibuf, c->ibuf[c->icur].p, l.n_ibuf * sizeof(cf2), hipMemcpyDeviceToHost));
    if (l.n_agc_hist) {
        // the last n_agc_hist samples of the AGC's input; while the stream is shorter than that only its own samples, at the end, are
        // ever read (AgcRmsArgs::hist_valid): what stands in front of them is left over from before a reset and stays out of the blob
        HIP_TRY(hipMemcpy(b + l.o_agc_hist, c->agc_hist.p, l.n_agc_hist * sizeof(cf2), hipMemcpyDeviceToHost));
        const size_t valid = c->agc_rms_pos < (uint64_t)l.n_agc_hist ? (size_t)c->agc_rms_pos : l.n_agc_hist;
        memset(b + l.o_agc_hist, 0, (l.n_agc_hist - valid) * sizeof(cf2));
    }
    StateHeader h;
    memset(&h, 0, sizeof(h));
    h.magic = kStateMagic; h.format_version = IQGPU_STATE_FORMAT_VERSION; h.bytes = (uint64_t)l.total;
    h.fingerprint = state_fingerprint(c); h.frames_in = c->total_in; h.frames_out = c->total_out;
    memcpy(b, &h, sizeof(h));
    h.checksum = state_checksum(b, l.total);
    memcpy(b, &h, sizeof(h));
    return IQGPU_OK;
}

// ------------------------------------------------------------------------------------------------
// iqgpu_chain_load_state: every check first -- a refused blob leaves the chain exactly as it was --, then what iqgpu_chain_reset does,
// then the state, everywhere the chain keeps it
// ------------------------------------------------------------------------------------------------
extern "C" int iqgpu_chain_load_state(iqgpu_chain *c, const void *blob, size_t bytes)
{
    const char *who = "iqgpu_chain_load_state";
    if (!c) return fail(IQGPU_EINVAL, "%s: NULL chain", who);
    StateHeader h;
    int rc = state_blob_check(who, blob, bytes, &h); if (rc) return rc;
    const StateLayout l = state_layout(c);
    const uint64_t mine = state_fingerprint(c);
    if (h.fingerprint != mine) return fail(IQGPU_EINVAL, "%s: fingerprint %016llx, this chain's is %016llx: the state was saved by a chain of "
        "another description or under other diagnostic switches", who, (unsigned long long)h.fingerprint, (unsigned long long)mine);
    if (h.bytes != (uint64_t)l.total) return fail(IQGPU_EINVAL, "%s: %llu bytes, the state of this chain is %zu", who, (unsigned long long)h.bytes,
        l.total);
    const char *b = (const char *)blob;
    StateWords w;
    memcpy(&w, b + l.o_words, sizeof(w));
    // the position words index the histories: inside what a chain of this design can reach
    if (w.rem < 0 || w.rem >= (c->decim ? c->D : 1)) return fail(IQGPU_EINVAL, "%s: open group of %d samples, the chain decimates by %d", who,
        w.rem, c->decim ? c->D : 1);
    if (w.fpending > 0 && w.fpending >= (uint64_t)(c->fp.enabled ? c->fp.block : 0)) return fail(IQGPU_EINVAL, "%s: %llu pending filter samples, "
        "the block is %u", who, (unsigned long long)w.fpending, c->fp.enabled ? c->fp.block : 0u);
    if (w.phi >= ((uint64_t)1 << 24) + (uint64_t)c->rp.step) return fail(IQGPU_EINVAL, "%s: resampler phase %llu out of range", who,
        (unsigned long long)w.phi);
    if (w.agc_locked != 0 && w.agc_locked != 1) return fail(IQGPU_EINVAL, "%s: AGC lock mirror %d", who, w.agc_locked);
    if (c->agc && w.agc.locked != 0 && w.agc.locked != 1) return fail(IQGPU_EINVAL, "%s: AGC state with locked = %d", who, w.agc.locked);

    HIP_TRY(hipSetDevice(c->device));
    // what iqgpu_chain_reset does first: batches in flight and what their last fused launch owes
    { const int prc = pipe_advance(c, c->pipe_seq); if (prc && !c->poisoned) return prc; }
    { const int prc = agc_resolve_pending(c); if (prc && !c->poisoned) return prc; }
    const size_t front = l.n_fbuf ? c->fp.taps.size() - 1 + (size_t)w.fpending : 0;
    if (l.n_fbuf) { rc = c->fbuf[c->fcur].ensure((front + 1) * sizeof(cf2)); if (rc) { c->poisoned = true; return rc; } }
    { const int prc = probe_drop(c); if (prc && !c->poisoned) return prc; }              // the I/Q probe's block is of the stream this chain leaves
    // from here on a failure leaves the device state half installed: the handle is poisoned, as by a failed call
#define LOAD_TRY(expr)                                                                                                  \
    do {                                                                                                                \
        hipError_t e_ = (expr);                                                                                         \
        if (e_ != hipSuccess) { c->poisoned = true; return fail(IQGPU_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); }  \
    } while (0)
    c->pend.valid = false;
    c->poisoned = false;
    c->rem = w.rem; c->phi = w.phi; c->nco_theta = w.nco_theta; c->pnco_theta = w.pnco_theta; c->fpending = w.fpending;
    c->total_in = h.frames_in; c->total_out = h.frames_out;
    { std::lock_guard<std::mutex> g(c->aux_mu); c->iq_mag = w.iq_mag; c->iq_phase = w.iq_phase; }
    const cd2 dc0 = c->dc ? w.dc : cd2{0.0, 0.0};
    LOAD_TRY(hipMemcpyAsync(c->d_dc_state, &dc0, sizeof(cd2), hipMemcpyHostToDevice, c->stream));
    c->agc_locked_host = false; c->agc_seen_host = 0; c->agc_peak_clean = false; c->agc_rms_pos = 0;
    if (c->agc) {
        // the AGC state everywhere the chain keeps it (as seek_impl does with an agc_entry): the device state, the host's mirrors; the
        // verifier's words at their initial values, no pending verdict, the peak array marked dirty
        LOAD_TRY(hipMemcpyAsync(c->d_agc_state, &w.agc, sizeof(AgcState), hipMemcpyHostToDevice, c->stream));
        LOAD_TRY(hipMemcpyAsync(c->d_agc_flag, kAgcFlagInit, sizeof(kAgcFlagInit), hipMemcpyHostToDevice, c->stream));
        c->agc_locked_host = w.agc_locked != 0; c->agc_seen_host = w.agc_seen; c->agc_rms_pos = w.agc_rms_pos;
        if (l.n_agc_hist) LOAD_TRY(hipMemcpyAsync(c->agc_hist.p, b + l.o_agc_hist, l.n_agc_hist * sizeof(cf2), hipMemcpyHostToDevice, c->stream));
    }
    if (l.n_ibuf) LOAD_TRY(hipMemcpyAsync(c->ibuf[c->icur].p, b + l.o_ibuf, l.n_ibuf * sizeof(cf2), hipMemcpyHostToDevice, c->stream));
    if (l.n_hist) {
        // the current buffer of each pair takes the history; the other one is zeroed, as a reset leaves it
        LOAD_TRY(hipMemcpyAsync(c->d_hist[c->hist_cur], b + l.o_hist, l.n_hist * sizeof(cf2), hipMemcpyHostToDevice, c->stream));
        LOAD_TRY(hipMemsetAsync(c->d_hist[c->hist_cur ^ 1], 0, l.n_hist * sizeof(cf2), c->stream));
    }
    if (l.n_hist2) {
        LOAD_TRY(hipMemcpyAsync(c->d_hist2[c->hist2_cur], b + l.o_hist2, l.n_hist2 * sizeof(cf2), hipMemcpyHostToDevice, c->stream));
        LOAD_TRY(hipMemsetAsync(c->d_hist2[c->hist2_cur ^ 1], 0, l.n_hist2 * sizeof(cf2), c->stream));
    }
    if (front) LOAD_TRY(hipMemcpyAsync(c->fbuf[c->fcur].p, b + l.o_fbuf, front * sizeof(cf2), hipMemcpyHostToDevice, c->stream));
    LOAD_TRY(hipStreamSynchronize(c->stream));               // (the copies read the caller's blob: done before it gets it back)
#undef LOAD_TRY
    return IQGPU_OK;
}
