// plan.cpp -- where a call starts and ends in the stream (closed forms, SPEC B.6) and how its tiles are dealt out to the
// wave-autonomous kernels.
#include "chain.hpp"

CallPlan plan_call_at(const iqgpu_chain *c, const StreamPos &at, size_t frames_in)
{
    CallPlan p;
    if (c->late) {
        p.n_res = (int64_t)frames_in;
        p.n_x = p.n_res;
        if (c->fp.enabled && c->fp.block) { // src/filter.c:503-525
            const uint64_t total = at.fpending + (uint64_t)p.n_res;
            p.n_x = (int64_t)((total / c->fp.block) * c->fp.block);
            p.fpending_next = total - (uint64_t)p.n_x;
        }
        const uint64_t span = (uint64_t)p.n_x << 24;
        const uint64_t step = c->rp.step;
        if (span > at.phi) { p.n_arb = (int64_t)((span - at.phi + step - 1) / step); p.phi_next
            = at.phi + (uint64_t)p.n_arb * step - span; }
        else { p.n_arb = 0; p.phi_next = at.phi - span; }
        p.n_emit = p.n_arb << c->ia.S;
        return p;
    }
    if (c->decim) {
        const uint64_t avail = (uint64_t)at.rem + frames_in;
        p.n_groups = (int64_t)(avail >> c->S);
        p.rem_next = (int)(avail & (uint64_t)(c->D - 1));
        const uint64_t span = (uint64_t)p.n_groups << 24;
        const uint64_t step = c->rp.step;
        if (span > at.phi) { p.n_res = (int64_t)((span - at.phi + step - 1) / step); p.phi_next
            = at.phi + (uint64_t)p.n_res * step - span; }
        else { p.n_res = 0; p.phi_next = at.phi - span; }
    } else {
        p.n_res = (int64_t)frames_in;
    }
    if (c->fp.enabled && c->fp.block) { // src/filter.c:503-525
        const uint64_t total = at.fpending + (uint64_t)p.n_res;
        p.n_emit = (int64_t)((total / c->fp.block) * c->fp.block);
        p.fpending_next = total - (uint64_t)p.n_emit;
    } else {
        p.n_emit = p.n_res;
    }
    return p;
}

CallPlan plan_call(const iqgpu_chain *c, size_t frames_in)
{
    StreamPos at; at.rem = c->rem; at.phi = c->phi; at.fpending = c->fpending;
    return plan_call_at(c, at, frames_in);
}

extern "C" size_t iqgpu_chain_next_out_frames(const iqgpu_chain *c, size_t frames_in)
{
    if (!c) return 0;
    if (c->pipe_launched < c->pipe_seq) {      // behind the batches submitted and not yet launched
        StreamPos at; at.rem = c->pipe_rem; at.phi = c->pipe_phi; at.fpending = c->pipe_fpending;
        return (size_t)plan_call_at(c, at, frames_in).n_emit;
    }
    return (size_t)plan_call(c, frames_in).n_emit;
}

// What the design_* calls below share: a throw-away chain designed from the description (create's validation), `ask` put to it --
// its refusals, then its answer -- and the chain gone again.  No device
template <class Ask> static int ask_design(const iqgpu_chain_desc *d, Ask ask)
{
    iqgpu_chain *c = new (std::nothrow) iqgpu_chain();
    if (!c) return fail(IQGPU_ENOMEM, "out of host memory");
    int rc = design_chain(c, d);
    if (rc == IQGPU_OK) rc = ask(c);
    delete c;
    return rc;
}

// frames a FRESH chain of this description emits for frames_in input frames in one stream: the same closed form
// the calls use (resampler law either way round, FFT-block quantisation in front of or behind the resampler),
// without a device -- what a sharding writer needs to place shard outputs (BASELINE configs[4])
extern "C" int iqgpu_design_out_frames(const iqgpu_chain_desc *d, size_t frames_in, size_t *frames_out)
{
    if (!d || !frames_out) return fail(IQGPU_EINVAL, "iqgpu_design_out_frames: NULL argument");
    *frames_out = 0;
    return ask_design(d, [&](const iqgpu_chain *c) { *frames_out = (size_t)plan_call(c, frames_in).n_emit; return (int)IQGPU_OK; });
}

// ------------------------------------------------------------------------------------------------
// seamless range sharding: the stream position as a closed form of the frames consumed, and the chain's memory in input frames
// ------------------------------------------------------------------------------------------------
StreamAt stream_at(const iqgpu_chain *c, uint64_t frames)
{
    StreamAt at;
    const CallPlan p = plan_call_at(c, StreamPos{}, (size_t)frames);
    at.pos.rem = p.rem_next; at.pos.phi = p.phi_next;
    at.pos.fpending = (c->fp.enabled && c->fp.block) ? p.fpending_next : 0;
    at.n_out = (uint64_t)p.n_emit;
    at.nco_theta = (uint32_t)frames * c->nco_dtheta;              // (mod 2^32, as the calls advance it)
    at.pnco_theta = (uint32_t)at.n_out * c->nco_dtheta;
    return at;
}

// Input frames a chain has to have seen for every history it keeps to hold stream data only.  Derived from the plans:
//   decimating front    d_hist holds the last hist_cap processed input frames (the warm-up tiles of every half-band level and of
//                       the polyphase window, plus the open group); behind k_cascade d_hist2 holds hist2_cap samples at rate / 2^(S-1),
//                       each of which needs the casc_warm warm-up tiles of the first S-1 stages in front of it
//   r >= 1              the front is pointwise; k_interp keeps ihist samples at the input rate
//   user filter         L - 1 taps of history, and for the FFT kind one block more (the samples pending at the position are then
//                       resampler outputs made from stream data) -- at the input rate in front of the resampler or without one, in
//                       resampler outputs behind it: n outputs span ceil(n step / 2^24) + 1 groups of 2^S frames
//   dc blocker          ceil(ln(1e6) / alpha) frames in front of all that: the state error decays as (1 - alpha)^n and reaches the
//                       output as alpha * e with |e| <= max|x| / alpha -- 1e-6 of full scale after that many frames (iqgpu.h)
uint64_t seek_preroll_frames(const iqgpu_chain *c, bool with_dc)
{
    uint64_t n = 0;
    if (c->decim) {
        n = (uint64_t)c->hist_cap;
        if (c->cascade) {
            const uint64_t via_mid = ((uint64_t)c->hist2_cap << (c->S - 1)) + (uint64_t)c->casc_warm * kWTile + (uint64_t)c->D;
            if (via_mid > n) n = via_mid;
        }
    }
    if (c->late) n = (uint64_t)c->ihist;
    if (c->fp.enabled) {
        uint64_t f = (uint64_t)(c->fp.taps.size() - 1) + (uint64_t)c->fp.block;
        if (c->decim) f = (((f * (uint64_t)c->rp.step + (((uint64_t)1 << 24) - 1)) >> 24) + 1) << c->S;
        n += f;
    }
    if (c->dc && with_dc) n += (uint64_t)std::ceil(std::log(1e6) / (double)c->dc_alpha);
    return n;
}

// Input frames E such that ANY E consecutive frames of the stream make the chain emit at least n outputs: plan_call_at's laws read
// from their worst position.  With B the FFT block of the user filter (0: FIR or none) and q(B) = B - 1 outputs a block boundary can
// hold back (0 without a block):
//   a call of E frames at an open group of rem frames closes (rem + E) >> S >= E >> S groups; g groups at phase phi < step give
//   ceil((g 2^24 - phi) / step) >= floor(g 2^24 / step) resampler outputs; n samples into the block filter with fpending >= 0 pending
//   leave floor((fpending + n) / B) B >= n - (B - 1).
//   no resampler          E = n + q
//   r < 1 (filter behind) E = ceil((n + q) step / 2^24) << S
//   r >= 1 (filter first) E = ceil(ceil(n / 2^S) step / 2^24) + q        (every resampler output becomes 2^S frames)
static uint64_t frames_for_outputs(const iqgpu_chain *c, uint64_t n)
{
    const uint64_t q = (c->fp.enabled && c->fp.block) ? (uint64_t)c->fp.block - 1 : 0;
    const uint64_t one = (uint64_t)1 << 24;
    if (c->late) {
        const uint64_t m = (n + (((uint64_t)1 << c->ia.S) - 1)) >> c->ia.S;
        return (m * (uint64_t)c->rp.step + one - 1) / one + q;
    }
    if (c->decim) return (((n + q) * (uint64_t)c->rp.step + one - 1) / one) << c->S;
    return n + q;
}

uint64_t seek_rms_preroll_frames(const iqgpu_chain *c)
{
    int64_t chunk = 0, warm = 0; int32_t nch = 0;
    agc_rms_geometry(c->agc_rms_alpha, 0, 0, &chunk, &warm, &nch);
    return seek_preroll_frames(c, false) + frames_for_outputs(c, (uint64_t)(warm + chunk));
}

// what seamless sharding without a recipe for the output AGC cannot do (the words of iqgpu_design_preroll_frames and _out_frames_range)
static int no_agc_check(const iqgpu_chain *c)
{
    if (c->agc) return fail(IQGPU_EUNSUPPORTED, "seamless sharding does not cover the output AGC: its state depends on the whole stream "
                                                "in front of a position, not on a bounded warm-up");
    return IQGPU_OK;
}

// P of a family's seek for a description: the family's own check (seek.cpp), put in the words of a description, then its preroll memory.
//   Plain  no check of its own: no output AGC
//   Rms    P_rms (seek_rms_preroll_frames)
//   DcRms  P_rms of the same description without the blocker (the blocker has no part in the FIR memory or in the output count:
//          seek_rms_preroll_frames does not read it).  The refusals are those of iqgpu_chain_dcrms_seek
static int design_preroll(const iqgpu_chain_desc *d, uint64_t *frames, SeekKind kind)
{
    const ShardFamily &fam = shard_family(kind);
    const char *who = fam.design_preroll;
    if (!d || !frames) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    *frames = 0;
    return ask_design(d, [&](const iqgpu_chain *c) {
        const int rc = fam.check == ShardCheck::None ? no_agc_check(c) : shard_check(fam, c, who, true);
        if (rc == IQGPU_OK) *frames = fam.memory(c);
        return rc;
    });
}

extern "C" int iqgpu_design_preroll_frames(const iqgpu_chain_desc *d, uint64_t *frames) { return design_preroll(d, frames, SeekKind::Plain); }
extern "C" int iqgpu_design_preroll_frames_rms(const iqgpu_chain_desc *d, uint64_t *frames) { return design_preroll(d, frames, SeekKind::Rms); }
extern "C" int iqgpu_design_preroll_frames_dcrms(const iqgpu_chain_desc *d, uint64_t *frames) { return design_preroll(d, frames, SeekKind::DcRms); }

extern "C" int iqgpu_design_out_frames_range(const iqgpu_chain_desc *d, uint64_t first_frame, uint64_t frames_in,
                                             uint64_t *out_first, uint64_t *frames_out)
{
    if (!d || !out_first || !frames_out) return fail(IQGPU_EINVAL, "iqgpu_design_out_frames_range: NULL argument");
    *out_first = 0; *frames_out = 0;
    return ask_design(d, [&](const iqgpu_chain *c) {
        const int rc = no_agc_check(c);
        if (rc != IQGPU_OK) return rc;
        if (first_frame > kMaxStreamFrames || frames_in > kMaxStreamFrames - first_frame)
            return fail(IQGPU_EINVAL, "stream position %llu + %llu frames is beyond 2^39 frames", (unsigned long long)first_frame,
                        (unsigned long long)frames_in);
        *out_first = stream_at(c, first_frame).n_out;
        *frames_out = stream_at(c, first_frame + frames_in).n_out - *out_first;
        return (int)IQGPU_OK;
    });
}

extern "C" size_t iqgpu_chain_max_out_frames(const iqgpu_chain *c, size_t frames_in)
{
    if (!c) return 0;
    // src/pipeline.c:246-258, generalised from PIPELINE_CHUNK_BASE_SAMPLES to frames_in
    double r = c->resample ? (double)c->ratio : 1.0;
    if (r < 1.0) r = 1.0;
    size_t cap = (size_t)std::ceil((double)frames_in * r) + 128;
    if (cap < frames_in) cap = frames_in;
    if (c->fp.enabled && c->fp.block) cap += c->fp.block;
    if (c->late) cap += ((size_t)2 << c->ia.S) + (c->fp.block ? (size_t)std::ceil((double)c->fp.block * r) : 0);
    return cap;
}

void Call::plan_geometry()
{
    const int64_t span_samples = (int64_t)c->rem + (int64_t)frames_in;
    total_tiles = (span_samples + kTile - 1) / kTile;
    // blocks of the workgroup-tiled k_front: with block_samples = 0 sized from the call -- about eight blocks
    // per CU, at least 16 tiles each when a block has to re-run a warm-up tile (decimating chains), any
    // size for pointwise chains
    tpb = c->tiles_per_block;
    if (c->auto_block) {
        int64_t t = (total_tiles + (int64_t)c->n_cu * 8 - 1) / ((int64_t)c->n_cu * 8);
        const int64_t t_min = c->decim ? 16 : 1;
        if (t < t_min) t = t_min;
        if (t > 128) t = 128;
        tpb = (int)t;
    }
    n_blocks = (int)((total_tiles + tpb - 1) / tpb);
    if (n_blocks < 1) n_blocks = 1;

    // the route, then the run geometry of a wave-autonomous one (needed by the dc carries as well)
    cplan = FrontArgs{};
    cplan.dbg = c->sw.dbg;
    if (!choose_route()) plan_route();
}

// THE k_front_s1 / k_front_s1<S0> geometry of a.rem0 + a.frames_in frames: tiles of 512 frames (256 without a half-band stage), one run
// per wave slot of the instantiation `a` selects or the fixed runs of block_samples, the warm-up the chain's history needs
// (warm_tiles != 0: the last stage behind k_cascade, whose history is one tile of the intermediate stream).  The first plan of a
// call, the plan a demoted k_front_mid falls back on and the fused-AGC fallback behind k_front_fat / _mid / _p0 are this function:
// the fallback's bytes are the first plan's because there is no second copy to drift
void Call::plan_s1(FrontArgs &a, int tile, int warm_tiles) const
{
    a.w_total_tiles = ((int64_t)a.rem0 + a.frames_in + tile - 1) / tile;
    int warm = warm_tiles ? warm_tiles : (int)((c->rp.history_in + tile - 1) / tile);
    if (warm < 1) warm = 1;
    plan_front_s1(a, wave_slots(front_s1_waves(a)), fixed_tpw(), warm, 1, tile);
}

// Which route the call takes (FrontRoute, chain.hpp): the predicates in the order that decides, each family's shape
// test from its own *_select().  Where a choice depends on the candidate's plan -- k_front_mid's edge runs, k_front_p0's streaming
// steps, k_cascade2's run length -- that plan is made here, once, and stands when the route does (returns true: cplan is planned).
bool Call::choose_route()
{
    const bool forced = (c->sw.dbg & kDbgForceFat) != 0;
    const bool casc = c->cascade && !c->sw.force_generic;
    const bool s0 = c->decim && c->S == 0 && !c->sw.force_generic;                                  // polyphase only
    const bool s1 = c->decim && c->S == 1 && c->rp.stages[0].m == 10 && !c->sw.force_generic;     // one half-band stage
    casc_K = c->S - 1;
    rem_k = casc ? (c->rem & ((1 << casc_K) - 1)) : c->rem;
    wtile = s0 ? 256 : kWTile;
    route = c->late ? FrontRoute::GenericLate : FrontRoute::Generic;
    if (!casc && !s0 && !s1) return true;                  // (the workgroup-tiled kernel: no wave plan)

    // the call and the chain's shape as the *_select() functions read them
    cplan.frames_in = (int64_t)frames_in; cplan.rem0 = rem_k; cplan.hist_cap = c->hist_cap;
    cplan.in_fmt = c->desc.in_format; cplan.out_fmt = (filt || casc) ? (int)IQGPU_FMT_CF32 : fin_fmt;
    cplan.raw_aligned = raw_aligned();
    cplan.agc_fused = front_fused() ? 1 : 0; cplan.agc_shift = c->S; cplan.agc_chunk_frames = c->agc_chunk;
    cplan.S = c->S; cplan.gain = c->desc.gain; cplan.iq_enable = c->desc.iq_correct_enable ? 1 : 0;
    cplan.dc_enable = c->dc ? 1 : 0; cplan.nco_mode = c->nco_mode;
    if (casc) {
        cplan.casc_K = casc_K;
        for (int k = 0; k < casc_K; ++k) cplan.m[k] = c->rp.stages[(size_t)k].m;
    }
    cplan.pnco_mode = (!filt && !c->late) ? c->pnco_mode : 0;
    cplan.step = c->rp.step;
    const bool s1_only = o.agc == AgcMode::MeasureS1;      // (the measure pass on k_front_s1<.., AGC>, chain.hpp)

    if (casc) {
        // S == 2: both stages in ONE kernel (k_front_s2, front_s2.hip).  Its streaming waves read the input as whole 16-byte words
        // from the start of a decimation group; calls that do not start on one, or are shorter than the histories they have to
        // leave behind, keep the two kernels (same bytes either way).
        if (casc_K == 1 && c->rem == 0 && cplan.raw_aligned && !front_fused() && !(c->sw.dbg & kDbgNoS2) && front_s2_shape(cplan) &&
            (int64_t)frames_in >= (int64_t)c->hist_cap && ((int64_t)frames_in >> 1) >= (int64_t)c->hist2_cap) {
            route = FrontRoute::S2;
            return false;
        }
        cplan.casc_wave_lds = (int)cascade_wave_lds(cplan);      // (reads the pointwise switches above: cascade2_shape)
        route = FrontRoute::Cascade;
        if (!cascade2_shape(cplan)) return false;
        // a raw cascade: k_cascade2's two-tile trips where the call's runs are long enough for them -- the evaluation of
        // cascade2_applies that decides (launch_cascade's own test is the same function of the same plan: DESIGN.md 3.0b)
        route = FrontRoute::Cascade2;
        plan_route();
        if (cascade2_applies(cplan, c->sw.casc2_min_run)) return true;
        // (too short for two-tile trips: k_cascade's own slice -- more waves per CU -- and no lead)
        cplan.casc_wave_lds = (int)cascade_wave_lds(cplan, false);
        route = FrontRoute::Cascade;
        plan_route();
        // (two stages on 8-bit frames: k_cascade's own slice holds k_cascade2's layout too, and without the lead a run can be a tile
        //  longer, so launch_cascade's test can pass on THIS plan: the route says what it will launch.  Every other shape fails it
        //  by the slice)
        if (cplan.casc_wave_lds >= cascade2_wave_lds(casc_K, cplan.in_fmt) && cascade2_applies(cplan, c->sw.casc2_min_run)) route = FrontRoute::Cascade2;
        return true;
    }
    if (s1) {
        // the preset shape on a call long enough to give every one of the 8 x CUs fat waves a run of tiles: k_front_fat
        // (shorter calls keep k_front_s1's 16 x CUs waves of 512-frame tiles: what counts for them is latency; same bytes either way)
        const bool fat_ok = !s1_only && front_fat_shape(cplan) &&
              (forced || (int64_t)frames_in >= (int64_t)kFatMinTilesPerWave * kFatTile * wave_slots(front_fat_waves()));
        const int nl = front_mid_nl(cplan);
        // (run descriptors hold tile indices in 32 bits)
        // (k_front_mid from 6 tiles per wave on: measured round 4 at 2^21 .. 2^25 frames, kernel ms k_front_s1 / k_front_mid:
        //  0.014 / 0.023, 0.017 / 0.023, 0.023 / 0.028, 0.039 / 0.036, 0.067 / 0.055 -- the crossover lies between 2^23 and 2^24 frames
        //  = 3.6 and 7.1 tiles per wave; the pipelined host path's 2^24-frame batches now run the headline kernel)
        constexpr int kMidMinTilesPerWave = 6;
        const bool mid_ok = !s1_only && nl != 0 && (int64_t)frames_in < ((int64_t)1 << 40) &&
              (forced || (int64_t)frames_in >= (int64_t)kMidMinTilesPerWave * front_mid_tile(nl) * wave_slots(front_mid_waves()));
        // (measured on one box, 2^28 frames: k_front_s1 0.437 ms, k_front_fat 0.404, k_front_mid 0.381: the 12-wave kernel is the
        //  default; iqgpu_debug_set("fat", "1") selects the 8-wave one where its step class applies)
        route = FrontRoute::S1;
        if (fat_ok && ((c->sw.dbg & kDbgUseFat) || !mid_ok)) route = FrontRoute::Fat;
        else if (mid_ok) {
            route = FrontRoute::Mid; mid_nl = nl;
            plan_route();
            if (cplan.w_n_edge <= front_mid_max_edge_waves()) return true;
            // (an unaligned buffer, a call that is all edges: k_front_mid keeps LDS for a handful of edge waves only)
            route = FrontRoute::S1; mid_nl = 0;
        }
        return false;
    }
    // S == 0 (the cu8-nrsc5 presets): k_front_p0 on calls long enough to give every one of its 8 x CUs waves a few steps of 320
    // outputs (shorter calls keep k_front_s1<S0>: same bytes).  Planned as k_front_s1's 256-frame tiles -- the edge runs are its
    // run_tiles -- with the streaming tiles' OUTPUTS dealt out as steps: it stands when its edge runs fit and it has steps to deal
    route = FrontRoute::S1S0;
    const bool long_call = (int64_t)frames_in >= ((int64_t)1 << 22) || forced;
    bool planned = false;
    if (!s1_only && !(c->sw.dbg & kDbgNoP0)) {
        cplan.phi0 = c->phi;
        if (front_p0_shape(cplan) && long_call) {
            const FrontArgs unplanned = cplan;
            route = FrontRoute::P0;
            plan_route();
            planned = cplan.w_n_stream > 0;
            if (!planned) { cplan = unplanned; route = FrontRoute::S1S0; }
        }
    }
    // ... and with a user filter behind the resampler on the overlap-save path: resampler AND filter in one kernel (k_p0fft16,
    // fftconv.hip, round 6) -- no front launch, no cf32 stream in HBM.  Long calls only (as k_front_p0); the next call's filter
    // front (history + pending samples) is recomputed by one workgroup, so it has to be short.  (Overrules k_front_p0 and keeps
    // the plan the call has by then -- k_front_p0's where that stood: of a route without a front launch only the run starts are read)
    if (c->fuse_filter && filt && p.n_emit > 0 && (int64_t)(L1 + p.fpending_next) <= kP0FftMaxKeep && long_call) route = FrontRoute::P0Fft;
    return planned;
}

// cplan and wtile of the route (S2: rem_k and s2_in_tiles too) from the shape fields choose_route has left in cplan
void Call::plan_route()
{
    wtile = route_tile(route, mid_nl);
    switch (route) {
    case FrontRoute::Generic: case FrontRoute::GenericLate: return;
    case FrontRoute::S1: case FrontRoute::S1S0: case FrontRoute::P0Fft: plan_s1(cplan, wtile); return;
    case FrontRoute::S2: {
        // planned in tiles of the LAST stage -- 512 intermediate samples = 1024 input frames -- on the intermediate stream's own
        // geometry: the run geometry everything else reads (dc carries included)
        cplan = FrontArgs{};
        cplan.dbg = c->sw.dbg; cplan.casc_K = casc_K; cplan.m[0] = c->rp.stages[0].m;
        cplan.frames_in = (int64_t)frames_in >> 1; cplan.rem0 = 0; cplan.hist_cap = c->hist2_cap;
        cplan.in_fmt = IQGPU_FMT_CF32; cplan.out_fmt = filt ? (int)IQGPU_FMT_CF32 : fin_fmt; cplan.raw_aligned = 1;
        cplan.w_total_tiles = (cplan.frames_in + kWTile - 1) / kWTile;
        plan_front_s1(cplan, wave_slots(route_waves(route, cplan)), fixed_tpw(), 1, 1);
        s2_in_tiles = ((int64_t)frames_in + kWTile - 1) / kWTile;
        rem_k = 0;
        return;
    }
    case FrontRoute::Fat: case FrontRoute::Mid: case FrontRoute::P0: case FrontRoute::Cascade: case FrontRoute::Cascade2: break;
    }
    const RouteInfo &ri = route_info(route);
    cplan.w_total_tiles = ((int64_t)rem_k + (int64_t)frames_in + wtile - 1) / wtile;
    int warm = ri.casc ? c->casc_warm : (int)((c->rp.history_in + wtile - 1) / wtile);
    if (warm < 1) warm = 1;
    // (block_samples counts k_front_s1's tiles; k_front_p0 deals its steps out itself)
    int ftpw = route == FrontRoute::P0 ? 0 : fixed_tpw();
    if (ftpw > 1) { ftpw = ftpw * kWTile / wtile; if (ftpw < 1) ftpw = 1; }
    plan_front_s1(cplan, wave_slots(route_waves(route, cplan)), ftpw, warm, route_edge_tpw(route, mid_nl), wtile, route_align(route, mid_nl), ri.lead);
    // k_front_mid: the three waves of a SIMD get runs in proportion to the speed their age buys them (kernels.hpp, weight_runs)
    if (route == FrontRoute::Mid && ftpw == 0 && cplan.w_n_edge <= front_mid_max_edge_waves() && c->sw.run_wt[0] > 0)
        weight_runs(cplan, front_mid_waves(), c->sw.run_wt);
    // k_front_p0: the streaming tiles' outputs as steps, where the edge runs fit its LDS and there are streaming tiles at all
    if (route == FrontRoute::P0) {
        if (cplan.w_n_edge <= front_p0_max_edge_waves() && cplan.w_edge_tb > cplan.w_edge_ta) plan_front_p0(cplan, wave_slots(front_p0_waves()));
        else cplan.w_n_stream = 0;
    }
}

// where every independent piece of the front kernel starts (the dc blocker needs its state there)
DcGeom Call::dc_geom() const
{
    DcGeom dg{};
    dg.frames_in = (int64_t)frames_in;
    if (route_info(route).wave) {
        dg.mode = 1;
        dg.n_edge1 = cplan.w_n_edge1; dg.n_stream = cplan.w_n_stream;
        dg.edge_tpw = cplan.w_edge_tpw; dg.run_q = cplan.w_run_q; dg.run_r = cplan.w_run_r; dg.ta = cplan.w_edge_ta; dg.tb
            = cplan.w_edge_tb;
        dg.warm = cplan.w_warm_tiles; dg.rem0 = rem_k; dg.tile = wtile;
        dg.n_seg = (int)(cplan.w_n_edge + dg.n_stream);
        if (dg.n_seg < 1) dg.n_seg = 1;
    } else {
        dg.mode = 0; dg.n_seg = n_blocks;
        dg.seg_first = ((int64_t)tpb - c->warm_tiles) * kTile - c->rem;
        dg.seg_len = (int64_t)tpb * kTile;
    }
    return dg;
}

