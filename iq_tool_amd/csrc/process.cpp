// process.cpp -- one process() call: every buffer sized first, then the stages in stream order
//   [dc carries] -> front (one FrontRoute, chain.hpp) -> [filter] -> [k_interp] -> [agc]
#include "chain.hpp"

// ------------------------------------------------------------------------------------------------
// profiling helpers
// ------------------------------------------------------------------------------------------------
Event get_event(iqgpu_chain *c)
{
    Event e;
    if (!c->event_pool.empty()) { e = std::move(c->event_pool.back()); c->event_pool.pop_back(); }
    else (void)e.create(hipEventDefault);                            // (a failure: an empty owner, and every call on it fails in turn)
    return e;
}
void drain_events(iqgpu_chain *c)
{
    for (auto &pe : c->pending_events) {
        float ms = 0.0f;
        (void)hipEventSynchronize(pe.b);
        if (hipEventElapsedTime(&ms, pe.a, pe.b) == hipSuccess) {
            c->prof.ms[pe.kind] += (double)ms;
            c->prof.launches[pe.kind] += 1;
        }
        c->event_pool.push_back(std::move(pe.a));
        c->event_pool.push_back(std::move(pe.b));
    }
    c->pending_events.clear();
}

// state of the dc blocker at the start of every independent piece of the front kernel
int Call::stage_dc_carries()
{
    const DcGeom dg = dc_geom();
    DcPrefixArgs pa{};
    pa.raw = d_raw_in; pa.in_fmt = c->desc.in_format; pa.gain = c->desc.gain;
    pa.raw_aligned = raw_aligned();
    pa.c = c->dc_c; pa.logc = c->dc_logc; pa.geom = dg; pa.agg = (cf2 *)c->dc_agg.p;
    { KernelTimer kt(c, IQGPU_K_DC_PREFIX); HIP_TRY(launch_dc_prefix(pa, c->stream)); }
    DcScanArgs sa{};
    sa.agg = (const cf2 *)c->dc_agg.p; sa.carry = (cd2 *)c->dc_carry.p; sa.state = c->d_dc_state;
    sa.geom = dg; sa.logc = c->dc_logc;
    { KernelTimer kt(c, IQGPU_K_DC_SCAN); HIP_TRY(launch_dc_scan(sa, c->stream)); }
    return IQGPU_OK;
}

// the cf32 buffers between stages: [L-1 history][pending][new] in front of the filter, [ihist][new] in front of k_interp
int Call::prepare_buffers()
{
    if (filt) {
        // (k_p0fft16 computes the resampler's outputs inside the filter kernel: only the buffer front exists)
        const size_t need = (L1 + (size_t)c->fpending + (route == FrontRoute::P0Fft ? 0 : (size_t)p.n_res) + 1) * sizeof(cf2);
        int rc = c->fbuf[c->fcur].ensure_keep(need, (L1 + (size_t)c->fpending) * sizeof(cf2), c->stream);
        if (rc) return rc;
        fcur = (cf2 *)c->fbuf[c->fcur].p;
    }
    if (c->late) {
        int rc = c->ibuf[c->icur].ensure_keep(((size_t)c->ihist + (size_t)p.n_x + 1) * sizeof(cf2), (size_t)c->ihist * sizeof(cf2),
            c->stream);
        if (rc) return rc;
        icur = (cf2 *)c->ibuf[c->icur].p;
        rc = c->ibuf[c->icur ^ 1].ensure(((size_t)c->ihist + 1) * sizeof(cf2)); if (rc) return rc;
    }
    // the buffers the later stages write: sized here, before the first launch touches the stream state
    if (filt) {
        int rc = c->fbuf[c->fcur ^ 1].ensure((L1 + (size_t)p.fpending_next + 1) * sizeof(cf2)); if (rc) return rc;
    }
    if (c->dc) {
        const DcGeom dg = dc_geom();
        int rc = c->dc_agg.ensure((size_t)dg.n_seg * sizeof(cf2)); if (rc) return rc;
        rc = c->dc_carry.ensure((size_t)dg.n_seg * sizeof(cd2)); if (rc) return rc;
    }
    if (route_info(route).casc) {
        // the intermediate stream between k_cascade and the last stage -- or, with both in k_front_s2, a few KB per edge wave
        const int64_t n_mid = route == FrontRoute::S2 ? front_s2_mid_samples(cplan) : ((int64_t)rem_k + (int64_t)frames_in) >> casc_K;
        int rc = c->mid.ensure(((size_t)n_mid + 8) * sizeof(cf2)); if (rc) return rc;
    }
    // run descriptors of k_front_mid: a fresh array starts exhausted (all zero), a used one is left exhausted by every launch
    if (route == FrontRoute::Mid && (c->sw.steal || fixed_tpw() != 0)) {
        const void *was = c->steal_buf.p;
        const size_t slots = (size_t)(fixed_tpw() != 0 ? wave_slots(front_mid_waves()) + cplan.w_n_edge : cplan.w_n_edge + cplan.w_n_stream) + 64;
        int rc = c->steal_buf.ensure(slots * (size_t)c->sw.steal_stride * sizeof(unsigned long long)); if (rc) return rc;
        if (c->steal_buf.p != was && hipMemsetAsync(c->steal_buf.p, 0, c->steal_buf.cap, c->stream) != hipSuccess)
            return fail(IQGPU_EHIP, "hipMemsetAsync failed");
    }
    if (c->agc && c->agc_rms_alpha > 0.0f) {
        int64_t chunk, warm; int32_t n_chunks;
        agc_rms_geometry(c->agc_rms_alpha, (int64_t)c->agc_rms_pos, p.n_emit, &chunk, &warm, &n_chunks);
        int rc = c->agc_gain.ensure((size_t)(n_chunks > 0 ? n_chunks : 1) * 4 * sizeof(float)); if (rc) return rc;
    } else if (c->agc) {
        const AgcGeom g = agc_geom();
        if (agc_out_end(g, g.n_chunks - 1) != p.n_emit) return fail(IQGPU_EINVAL, "internal: AGC chunk map disagrees with the call plan");
        { const void *was = c->agc_peak.p;
          int rc0 = c->agc_peak.ensure((size_t)g.n_chunks * sizeof(unsigned long long)); if (rc0) return rc0;
          if (c->agc_peak.p != was) c->agc_peak_clean = false; }
        int rc = c->agc_gain.ensure((size_t)g.n_chunks * (sizeof(float) + sizeof(int32_t) + sizeof(int64_t)) + 2 * ((size_t)g.n_chunks / 256 + 2) * sizeof(int32_t)); if (rc) return rc;
        if (agc_fused) {   // what the fallback launches need, should the verifier reject the fused pass
            rc = c->agc_peak_b.ensure((size_t)g.n_chunks * sizeof(unsigned long long)); if (rc) return rc;
            rc = c->abuf.ensure(((size_t)p.n_emit + 1) * sizeof(cf2)); if (rc) return rc;
        }
    }
    return IQGPU_OK;
}

// the routes with k_cascade's stages in front (a: the launch arguments every route shares): stages 0 .. S-2 raw -> mid, then the
// last stage + polyphase as a one-stage chain on the intermediate stream -- or both in k_front_s2
int Call::front_cascade(FrontArgs &a)
{
    const bool s2 = route == FrontRoute::S2;
    // ---- stages 0 .. S-2: raw -> mid (cf32 at rate / 2^K) ----
    const int K = casc_K;
    const int rem_1 = c->rem >> K;
    const int64_t n_mid = ((int64_t)rem_k + (int64_t)frames_in) >> K;
    FrontArgs a1 = a;
    a1.rem0 = rem_k;
    a1.nco_theta0 = c->nco_theta - (uint32_t)rem_k * c->nco_dtheta;
    a1.casc_K = K;
    for (int k = 0; k < K; ++k) {
        const std::vector<float> &br = c->rp.stages[(size_t)k].branch;
        for (size_t q = 0; q < 12; ++q) a1.casc_taps[k][q] = q < br.size() ? 0.5f * br[q] : 0.0f;
    }
    a1.casc_out = (cf2 *)c->mid.p; a1.casc_n_out = n_mid;
    a1.casc_wave_lds = s2 ? (int)cascade_wave_lds(a1) : cplan.casc_wave_lds;      // (the plan's: sized for k_cascade2 where the call takes it)
    a1.out_fmt = IQGPU_FMT_CF32; a1.pnco_mode = 0;
    if (s2) a1.w_total_tiles = s2_in_tiles;          // (the fused kernel is planned in the last stage's tiles: cplan is a2's)
    else {
        copy_plan(a1);
        // (k_cascade2 where launch_cascade's own test says so: the plan's test on the same plan -- the route says which)
        KernelTimer kt(c, IQGPU_K_CASCADE); HIP_TRY(launch_cascade(a1, c->sw.casc2_min_run, c->stream));
    }
    if (n_mid <= 0) return IQGPU_OK;
    // ---- last stage + polyphase: a one-stage chain on the intermediate stream ----
    FrontArgs a2{};
    a2.dbg = c->sw.dbg;
    a2.raw = c->mid.p; a2.hist_in = c->d_hist2[c->hist2_cur]; a2.hist_out = c->d_hist2[c->hist2_cur ^ 1];
    a2.frames_in = n_mid; a2.hist_cap = c->hist2_cap; a2.rem0 = rem_1;
    a2.in_fmt = IQGPU_FMT_CF32; a2.gain = 1.0f; a2.raw_aligned = 1;
    a2.nco_tab = c->d_nco_tab;
    a2.mode = 1; a2.S = 1; a2.m[0] = c->rp.stages[(size_t)K].m;
    a2.arb_table = c->d_arb; a2.step = c->rp.step; a2.phi0 = c->phi;
    a2.n_groups = p.n_groups; a2.n_out = p.n_res;
    a2.pnco_mode = a.pnco_mode; a2.pnco_theta0 = a.pnco_theta0; a2.pnco_dtheta = a.pnco_dtheta;
    a2.out_fmt = a.out_fmt; a2.out = a.out;
    a2.agc_fused = front_fused() ? 1 : 0;
    if (s2) copy_plan(a2);
    else plan_s1(a2, kWTile, 1);                     // (one warm-up tile: the last stage keeps 66 samples of history)
    for (int q = 0; q < 20; ++q) a2.hb0[q] = 0.5f * c->rp.stages[(size_t)K].branch[(size_t)q];
    a2.sink = c->d_sink;
    if (front_fused()) HIP_TRY(wire_fused_agc(a2));
    { KernelTimer kt(c, IQGPU_K_FRONT); HIP_TRY(s2 ? launch_front_s2(a1, a2, c->stream) : launch_front_s1(a2, c->stream)); }
    if (front_fused() && !no_verdict()) { const int rc = stage_agc_verify_and_fallback(a2); if (rc) return rc; }
    c->hist2_cur ^= 1;
    return IQGPU_OK;
}

int Call::stage_front()
{
    const RouteInfo &ri = route_info(route);
    if (route == FrontRoute::P0Fft) {
        // resampler and filter run as ONE kernel, launched by stage_filter (which also turns the history buffers over)
        snprintf(c->front_kernel, sizeof(c->front_kernel), "%s", ri.name);
        return IQGPU_OK;
    }
    FrontArgs a{};
    a.dbg = c->sw.dbg;
    a.raw = d_raw_in;
    a.hist_in = c->d_hist[c->hist_cur]; a.hist_out = c->d_hist[c->hist_cur ^ 1];
    a.frames_in = (int64_t)frames_in; a.hist_cap = c->hist_cap; a.rem0 = c->rem;
    a.in_fmt = c->desc.in_format; a.gain = c->desc.gain;
    a.raw_aligned = raw_aligned();
    a.dc_enable = c->dc ? 1 : 0;
    if (c->dc) {
        a.dc_c = c->dc_c; a.dc_a = 1.0f - c->dc_c; a.dc_logc = c->dc_logc;
        for (int k = 0; k < 6; ++k) a.dc_cpow[k] = (float)std::exp((double)(4 << k) * c->dc_logc);
        a.dc_cpow[6] = (float)std::exp(256.0 * c->dc_logc);
        a.dc_cpow[7] = (float)std::exp(1024.0 * c->dc_logc);
        a.dc_carry = (const cd2 *)c->dc_carry.p;
    }
    a.iq_enable = c->desc.iq_correct_enable ? 1 : 0;
    a.iq_magp1 = 1.0f + iq_mag; a.iq_phase = iq_phase;
    a.nco_mode = c->nco_mode;
    a.nco_dtheta = c->nco_dtheta;
    // phase of i_rel = 0, i.e. rem samples before the first new sample
    a.nco_theta0 = c->nco_theta - (uint32_t)c->rem * c->nco_dtheta;
    a.nco_tab = c->d_nco_tab;
    a.mode = c->decim ? 1 : 0;
    a.S = c->S;
    for (int i = 0; i < c->S; ++i) { a.m[i] = c->rp.stages[(size_t)i].m; a.tap_off[i] = c->tap_off[i]; }
    for (int i = 0; i <= c->S + 1; ++i) a.lvl_off[i] = c->lvl_off[i];
    a.n_hb_taps = c->n_hb_taps; a.hb_taps = c->d_hb; a.arb_table = c->d_arb;
    a.step = c->rp.step; a.n_est = c->n_est; a.phi0 = c->phi;
    a.n_groups = p.n_groups; a.n_out = p.n_res;
    a.total_tiles = total_tiles; a.tiles_per_block = tpb; a.warm_tiles = c->warm_tiles;
    a.pnco_theta0 = c->pnco_theta; a.pnco_dtheta = c->nco_dtheta;
    const bool nco_in_front = !filt && !c->late;     // otherwise the post NCO runs in the last stage
    a.pnco_mode = nco_in_front ? c->pnco_mode : 0;
    if (filt)         { a.out_fmt = IQGPU_FMT_CF32; a.out = fcur + L1 + c->fpending; }
    else if (c->late) { a.out_fmt = IQGPU_FMT_CF32; a.out = icur + c->ihist; }
    else              { a.out_fmt = fin_fmt; a.out = fin_out; }
    a.sink = c->d_sink;
    // one wave-autonomous kernel on the raw input: the plan and the fused-AGC fields first (what k_front_mid's selection reads)
    const bool one_kernel = ri.wave && !ri.casc;
    if (one_kernel) {
        copy_plan(a);
        if (front_fused()) HIP_TRY(wire_fused_agc(a));
    }
    const auto wire_hb0 = [&] { for (int q = 0; q < 20; ++q) a.hb0[q] = 0.5f * c->rp.stages[0].branch[(size_t)q]; };
    char mid_name[48];
    const char *name = ri.name;
    hipError_t (*launch)(const FrontArgs &, hipStream_t) = nullptr;      // of a one-kernel route: wired here, launched below

    switch (route) {
    case FrontRoute::Generic: case FrontRoute::GenericLate: {
        KernelTimer kt(c, IQGPU_K_FRONT);
        HIP_TRY(launch_front(a, n_blocks, c->stream));
        break;
    }
    case FrontRoute::Cascade: case FrontRoute::Cascade2: case FrontRoute::S2: {
        const int rc = front_cascade(a); if (rc) return rc;
        break;
    }
    case FrontRoute::S1: wire_hb0(); launch = launch_front_s1; break;      // one half-band stage (m = 10)
    case FrontRoute::S1S0: launch = launch_front_s1; break;                // none
    case FrontRoute::P0Fft: break;                                         // (no front launch: returned above)
    case FrontRoute::Fat: wire_hb0(); a.tap_fold = (uint32_t)c->tap_fold8; launch = launch_front_fat; break;
    // (k_front_p0: consecutive lanes are five outputs apart -- for the NRSC-5 step 16 arms -- so the lanes that re-read a slot in
    //  the same step would meet in two bank pairs of a linear plane: always the folded placement)
    case FrontRoute::P0: a.tap_fold = 1u; launch = launch_front_p0; break;
    case FrontRoute::Mid: {
        wire_hb0();
        // "steal" on, one run per resident wave: every wave claims its tiles through its run descriptor and waves that finish
        // early split the runs of those that are behind (front_mid.hip; off by default, profiles/r04_steal.md)
        if (c->sw.steal && fixed_tpw() == 0 && a.w_n_stream >= 64 * (int64_t)front_mid_waves()) wire_run_descriptors(a, c->sw.steal_rounds, 0);
        // (the multi-run instantiation exists for six outputs per lane only: the 8-per-lane experiment, "mid8", keeps one
        //  static run per wave over as many rounds of workgroups as the runs need -- ADVICE r4)
        // block_samples != 0 (BASELINE configs[1] as worded: "256 k-sample blocks"): more fixed-length runs than resident waves --
        // one round of workgroups, every streaming wave takes runs s, s + stride, ... through the multi-run instantiation
        else if (front_mid_nl(a) == 6 && fixed_tpw() != 0 && a.w_n_stream > wave_slots(front_mid_waves()) - a.w_n_edge)
            wire_run_descriptors(a, 0, wave_slots(front_mid_waves()) - a.w_n_edge);
        const MidSel msel = front_mid_select(a);
        a.tap_fold = (uint32_t)(msel.NL == 8 ? c->tap_fold8 : c->tap_fold6);
        a.nco_hold = (uint32_t)(msel.NL == 8 ? c->nco_hold8 : front_mid_holds_all(msel) ? c->nco_hold6_all : c->nco_hold6);
        const bool b8 = msel.INF == IQGPU_FMT_CU8 || msel.INF == IQGPU_FMT_CS8 || msel.O8 != 0;
        snprintf(mid_name, sizeof(mid_name), "%s<%d,%s%s%s%s>", ri.name, msel.NL, msel.NONCO ? "nonco" : "nco", msel.CF ? ",cf32" : "",
                 b8 ? ",8bit" : "", msel.INF == kMidN16 ? ",gain" : "");
        name = mid_name;
        launch = launch_front_mid;
        break;
    }
    }
    if (launch) {
        { KernelTimer kt(c, IQGPU_K_FRONT); HIP_TRY(launch(a, c->stream)); }
        // (the measure pass on k_front_s1<.., AGC>, a fused piece of a shadow call: the gain of a scratch state, no verdict -- only
        //  the kernel's peak array is wanted)
        if (front_fused() && !no_verdict()) { const int rc = stage_agc_verify_and_fallback(a); if (rc) return rc; }
    }
    if (c->decim) c->hist_cur ^= 1;
    snprintf(c->front_kernel, sizeof(c->front_kernel), "%s", name);
    return IQGPU_OK;
}

int Call::stage_filter()
{
    FirArgs fa{};
    fa.fbuf = fcur; fa.taps = c->d_ftaps; fa.ntaps = (int)c->fp.taps.size(); fa.is_complex = c->fp.is_complex ? 1 : 0;
    const int64_t n_filt = c->late ? p.n_x : p.n_emit;
    fa.n_emit = n_filt;
    fa.pnco_mode = c->late ? 0 : c->pnco_mode; fa.pnco_theta0 = c->pnco_theta; fa.pnco_dtheta = c->nco_dtheta; fa.nco_tab = c->d_nco_tab;
    if (c->late) { fa.out_fmt = IQGPU_FMT_CF32; fa.out = icur + c->ihist; }
    else         { fa.out_fmt = fin_fmt; fa.out = fin_out; }
    // next call's buffer front: history (L-1) + still-pending samples, into the other buffer of the pair -- by the filter kernel's
    // last workgroup when one is launched (nobody reads that buffer meanwhile), else by a copy kernel
    const size_t keep = L1 + (size_t)p.fpending_next;
    const bool fused_move = n_filt > 0 && !(c->sw.dbg & kDbgNoFusedMove);
    if (fused_move) { fa.move_dst = (cf2 *)c->fbuf[c->fcur ^ 1].p; fa.move_src = fcur + n_filt; fa.move_n = (int64_t)keep; }
    if (c->d_hfreq) {
        FftConvArgs ca{};
        ca.dbg = c->sw.dbg;
        ca.fbuf = fcur; ca.fbuf_len = (int64_t)(L1 + (size_t)c->fpending + (size_t)p.n_res);
        ca.hfreq = c->d_hfreq; ca.twiddle = c->d_twiddle; ca.ntaps = fa.ntaps;
        ca.log2n = c->fft_log2n; ca.threads = c->sw.fft_threads; ca.n_emit = n_filt;
        ca.pnco_mode = fa.pnco_mode; ca.pnco_theta0 = fa.pnco_theta0; ca.pnco_dtheta = fa.pnco_dtheta; ca.nco_tab = fa.nco_tab;
        ca.out_fmt = fa.out_fmt; ca.out = fa.out;
        ca.move_dst = fa.move_dst; ca.move_src = fa.move_src; ca.move_n = fa.move_n;
        if (route == FrontRoute::P0Fft) {
            // k_p0fft16: the window fill needs what the front kernel would have been given
            if (!fused_move) return fail(IQGPU_EINVAL, "internal: the fused filter path needs the history move in the kernel");
            P0Feed &f = ca.feed;
            f.raw = d_raw_in; f.hist_in = c->d_hist[c->hist_cur]; f.hist_out = c->d_hist[c->hist_cur ^ 1];
            f.frames_in = (int64_t)frames_in; f.hist_cap = c->hist_cap; f.in_fmt = c->desc.in_format;
            f.arb_table = c->d_arb; f.step = c->rp.step; f.tap_fold = 1u; f.phi0 = c->phi;
            f.n_res = p.n_res; f.pre = (int64_t)(L1 + (size_t)c->fpending);
            // outputs whose 24-frame window load lies inside this call's input: q_k = (phi0 + k step) >> 24 in [13, frames_in - 11]
            f.k_a = first_k(c->phi, c->rp.step, 13); f.k_b = first_k(c->phi, c->rp.step, (int64_t)frames_in - 10);
            if (f.k_b > f.n_res) f.k_b = f.n_res;
            if (f.k_a > f.k_b) f.k_a = f.k_b;
            f.write_state = 1;
            f.grid = c->n_cu * (c->fft_log2n <= 12 ? 2 : 1);
            ca.win = c->fuse_win; ca.vout = c->fuse_vout;
        } else if (c->fuse_win > 0) {
            // the calls of such a chain that stay on the two kernels (short ones) run the fused kernel's windows: the
            // chain's bytes do not depend on which kernel a call took
            ca.win = c->fuse_win; ca.vout = c->fuse_vout;
        }
        if (agc_fused) {       // (past the lock, the filter between the resampler and the AGC: gain and per-chunk peaks in its epilogue)
            ca.agc_fused = 1; ca.agc_state = c->d_agc_state; ca.agc_peak2 = (unsigned long long *)c->agc_peak.p; ca.agc_geom = agc_geom();
            HIP_TRY(clean_agc_peaks());
        }
        { KernelTimer kt(c, IQGPU_K_FILTER); HIP_TRY(launch_fftconv(ca, c->stream)); }
        if (agc_fused) { const int rc = stage_agc_verify_and_fallback_filter(ca); if (rc) return rc; }
    } else {
        KernelTimer kt(c, IQGPU_K_FILTER);
        HIP_TRY(launch_fir(fa, c->stream));
    }
    if (!fused_move) {
        KernelTimer kt(c, IQGPU_K_MOVE);
        HIP_TRY(launch_copy_cf((cf2 *)c->fbuf[c->fcur ^ 1].p, fcur + n_filt, (int64_t)keep, c->stream));
    }
    c->fcur ^= 1;
    c->fpending = p.fpending_next;
    if (route == FrontRoute::P0Fft && c->decim) c->hist_cur ^= 1;               // (what stage_front does behind its launch)
    return IQGPU_OK;
}

// r >= 1: the resampler behind the front stage / pre filter
int Call::stage_late_resampler()
{
    InterpArgs ia = c->ia;
    ia.xbuf = icur; ia.hist = c->ihist; ia.n_in = p.n_x;
    ia.phi0 = c->phi; ia.n_arb = p.n_arb; ia.n_emit = p.n_emit;
    ia.n_tiles = (p.n_emit + kInterpTile - 1) / kInterpTile;
    ia.hb_taps = c->d_ihb; ia.arb_table = c->d_arb;
    ia.pnco_mode = c->pnco_mode; ia.pnco_theta0 = c->pnco_theta; ia.pnco_dtheta = c->nco_dtheta; ia.nco_tab = c->d_nco_tab;
    ia.out_fmt = fin_fmt; ia.out = fin_out;
    // the next call's history (the last ihist resampler inputs) into the other buffer of the pair: by k_interp's last workgroup
    // when it is launched, else by a copy kernel
    const bool fused_move = p.n_emit > 0 && !(c->sw.dbg & kDbgNoFusedMove);
    ia.move_dst = nullptr; ia.move_src = nullptr; ia.move_n = 0;
    if (fused_move) { ia.move_dst = (cf2 *)c->ibuf[c->icur ^ 1].p; ia.move_src = icur + p.n_x; ia.move_n = (int64_t)c->ihist; }
    { KernelTimer kt(c, IQGPU_K_FRONT); HIP_TRY(launch_interp(ia, c->n_cu, c->stream)); }
    if (!fused_move) {
        KernelTimer kt(c, IQGPU_K_MOVE);
        HIP_TRY(launch_copy_cf((cf2 *)c->ibuf[c->icur ^ 1].p, icur + p.n_x, (int64_t)c->ihist, c->stream));
    }
    c->icur ^= 1;
    return IQGPU_OK;
}

// what every call starts from: the plan at the chain's position and where the last stage writes without an AGC behind it
static Call begin_call(iqgpu_chain *c, const void *d_raw_in, size_t frames_in, void *d_out, const CallOpts &o)
{
    Call k{};
    k.c = c; k.d_raw_in = d_raw_in; k.frames_in = frames_in; k.d_out = d_out; k.o = o;
    k.p = plan_call(c, frames_in);
    k.filt = c->fp.enabled;
    k.L1 = k.filt ? c->fp.taps.size() - 1 : 0;
    k.fpending0 = c->fpending;
    k.fin_out = d_out; k.fin_fmt = c->desc.out_format;
    return k;
}

// iqgpu_chain_dc_measure: the DC blocker's map of ONE call -- the call an ordinary process of frames_in frames at stream position `at`
// would be, planned by the code that plans it (begin_call, plan_geometry, dc_geom), of which only k_dc_prefix and the scan are
// launched; the scan writes the map to d_map and leaves the chain's DC state and carries alone.  The chain's position is put back.
// (a chain with the AGC: the piece in front of the lock leaves cf32 for the AGC kernels, the piece behind it -- past_lock -- has the
//  gain in its last kernel; both enter the plan as in process_one)
// (the planning alone, host arithmetic: shared with the range form, seek.cpp, which plans every piece of a range up front)
DcMeasurePlan dc_measure_plan(iqgpu_chain *c, const StreamPos &at, const void *d_raw_in, size_t frames_in, bool past_lock)
{
    const StreamPos was{c->rem, c->phi, c->fpending};
    c->rem = at.rem; c->phi = at.phi; c->fpending = at.fpending;
    Call k = begin_call(c, d_raw_in, frames_in, nullptr, CallOpts());
    k.agc_fused = past_lock;
    if (c->agc && !past_lock) k.fin_fmt = IQGPU_FMT_CF32;
    k.plan_geometry();
    const DcMeasurePlan mp{k.dc_geom(), k.raw_aligned()};
    c->rem = was.rem; c->phi = was.phi; c->fpending = was.fpending;
    return mp;
}

int dc_measure_call(iqgpu_chain *c, const StreamPos &at, const void *d_raw_in, size_t frames_in, cd2 *d_map, bool past_lock)
{
    const DcMeasurePlan mp = dc_measure_plan(c, at, d_raw_in, frames_in, past_lock);
    const DcGeom &dg = mp.geom;
    int rc = c->dc_agg.ensure((size_t)dg.n_seg * sizeof(cf2)); if (rc) return rc;
    DcPrefixArgs pa{};
    pa.raw = d_raw_in; pa.in_fmt = c->desc.in_format; pa.gain = c->desc.gain;
    pa.raw_aligned = mp.raw_aligned;
    pa.c = c->dc_c; pa.logc = c->dc_logc; pa.geom = dg; pa.agg = (cf2 *)c->dc_agg.p;
    HIP_TRY(launch_dc_prefix(pa, c->stream));
    DcScanArgs sa{};
    sa.agg = (const cf2 *)c->dc_agg.p; sa.geom = dg; sa.logc = c->dc_logc; sa.map = d_map;
    HIP_TRY(launch_dc_scan(sa, c->stream));
    return IQGPU_OK;
}

static int process_one(iqgpu_chain *c, const void *d_raw_in, size_t frames_in,
                       void *d_out, size_t out_capacity_bytes, size_t *frames_out, const CallOpts &o, bool past_lock)
{   // past_lock: the part of an ordinary call behind the AGC's lock, on a chain whose last kernel applies the gain itself
    *frames_out = 0;
    if (frames_in == 0) return IQGPU_OK;
    const bool bypass = c->agc && o.agc != AgcMode::Ordinary;      // nothing of such a call reaches d_out
    if (!d_raw_in || (!d_out && !bypass)) return fail(IQGPU_EINVAL, "iqgpu_chain_process_device: NULL buffer");
    if (frames_in > ((size_t)1 << 40)) return fail(IQGPU_EINVAL, "frames_in too large");
    if (c->poisoned) return fail(IQGPU_EHIP,
        "an earlier call failed half way through: the stream state is undefined until iqgpu_chain_reset()");
    HIP_TRY(hipSetDevice(c->device));
    // a fused launch of an earlier call may still owe its fallback: before anything of this call is queued behind it
    { const int prc = agc_resolve_pending(c); if (prc) return prc; }

    Call k = begin_call(c, d_raw_in, frames_in, d_out, o);
    const size_t obps = bytes_per_frame(c->desc.out_format);
    if (!bypass && (size_t)k.p.n_emit * obps > out_capacity_bytes)
        return fail(IQGPU_ECAPACITY, "output buffer too small: need %zu bytes, have %zu", (size_t)k.p.n_emit * obps, out_capacity_bytes);
    // with the AGC on, the last stage leaves cf32 in abuf and k_agc_apply packs -- unless the call is past the lock
    // on a chain whose front kernel applies the gain itself (fused: packed output straight to the caller)
    // (the measure pass on k_front_s1<.., AGC>: the fused front launch as it is, against a scratch state and with no verdict -- stage_front)
    // (a shadow call, chain.hpp: the piece behind a filter keeps the filter's cf32 epilogue -- the plan of a chain with a filter does
    //  not read agc_fused -- and is measured like a piece in front of the lock)
    const bool shadow = o.agc == AgcMode::Shadow;
    const bool agc_fused = (past_lock && !(shadow && c->fp.enabled)) || o.agc == AgcMode::MeasureS1;
    const bool scratch_fused = o.agc == AgcMode::MeasureS1 || (shadow && agc_fused);      // the fused front launch against the scratch state
    const bool measure_unfused = o.agc == AgcMode::Measure || (shadow && !agc_fused);    // k_agc_measure over abuf
    k.agc_fused = agc_fused;
    if (c->agc && !agc_fused) {
        // (dx / local: the AGC's input of earlier calls stands in front of this call's, see stage_agc)
        const size_t lead = c->agc_rms_alpha > 0.0f ? (size_t)c->agc_rms_warm : 0;
        int rc = c->abuf.ensure((lead + (size_t)k.p.n_emit + 1) * sizeof(cf2)); if (rc) return rc;
        k.fin_out = (cf2 *)c->abuf.p + lead; k.fin_fmt = IQGPU_FMT_CF32;
        if (measure_unfused && !o.rows) {
            rc = c->agc_rows.ensure((((size_t)frames_in + (size_t)c->agc_chunk - 1) / (size_t)c->agc_chunk) * sizeof(AgcRow)); if (rc) return rc;
        }
    }
    if (scratch_fused) {
        // the packed output nobody keeps, the scratch state (the fresh one: gain 1) and the table
        int rc = c->seek_sink.ensure((size_t)k.p.n_emit * obps + 16); if (rc) return rc;
        k.fin_out = c->seek_sink.p;
        const void *was = c->agc_scratch.p;
        rc = c->agc_scratch.ensure(sizeof(AgcState)); if (rc) return rc;
        if (c->agc_scratch.p != was) HIP_TRY(hipMemcpyAsync(c->agc_scratch.p, &c->agc_init, sizeof(AgcState), hipMemcpyHostToDevice, c->stream));
        if (!o.rows) { rc = c->agc_rows.ensure((((size_t)frames_in + (size_t)c->agc_chunk - 1) / (size_t)c->agc_chunk) * sizeof(AgcRow)); if (rc) return rc; }
    }
    k.plan_geometry();
    if (o.iq_fixed) { k.iq_mag = o.iq_mag; k.iq_phase = o.iq_phase; }                              // a pipelined batch: as of its submit()
    else { std::lock_guard<std::mutex> g(c->aux_mu); k.iq_mag = c->iq_mag; k.iq_phase = c->iq_phase; }   // read once per call

    // every buffer the stages need is sized before the first launch, so that an allocation failure leaves the
    // stream state untouched; a failure after that (a launch error) leaves the device state half advanced:
    // the handle is poisoned and every later call fails until iqgpu_chain_reset()
    int rc;
    if ((rc = k.prepare_buffers()) != IQGPU_OK) return rc;
    // the I/Q probe: the head of an ordinary stream call of at least 1024 frames, while the slot is free (CallOpts::no_probe, probe_span)
    bool want_probe = false;
    if (!o.no_probe) {
        std::lock_guard<std::mutex> g(c->aux_mu);
        want_probe = c->probe_on && (o.probe_span ? o.probe_span : frames_in) >= 1024 && !c->probe_pending;
    }
    if (want_probe) {
        // before k_dc_scan moves the dc state to the end of this call
        IqProbeArgs pa{};
        pa.raw = d_raw_in; pa.in_fmt = c->desc.in_format; pa.gain = c->desc.gain;
        pa.dc_enable = c->dc ? 1 : 0; pa.dc_c = c->dc_c; pa.dc_state = c->d_dc_state;
        pa.iq_enable = c->desc.iq_correct_enable ? 1 : 0; pa.iq_magp1 = 1.0f + k.iq_mag; pa.iq_phase = k.iq_phase;
        pa.nco_mode = c->nco_mode; pa.nco_theta0 = c->nco_theta; pa.nco_dtheta = c->nco_dtheta; pa.nco_tab = c->d_nco_tab;
        pa.out = c->d_probe;
        HIP_TRY(launch_iq_probe(pa, c->stream));
        HIP_TRY(hipMemcpyAsync(c->h_probe, c->d_probe, 1024 * sizeof(cf2), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipEventRecord(c->probe_done, c->stream));
        std::lock_guard<std::mutex> g(c->aux_mu);
        c->probe_pending = true;
    }
    if (c->dc && (rc = k.stage_dc_carries()) != IQGPU_OK) { c->poisoned = true; return rc; }
    if ((rc = k.stage_front()) != IQGPU_OK) { c->poisoned = true; return rc; }
    if (k.filt && (rc = k.stage_filter()) != IQGPU_OK) { c->poisoned = true; return rc; }
    if (c->late && (rc = k.stage_late_resampler()) != IQGPU_OK) { c->poisoned = true; return rc; }
    if (c->agc && !agc_fused && o.agc != AgcMode::Drop &&
        (rc = measure_unfused ? k.stage_agc_measure() : k.stage_agc()) != IQGPU_OK) { c->poisoned = true; return rc; }
    if (scratch_fused && (rc = k.stage_agc_rows_from_peaks()) != IQGPU_OK) { c->poisoned = true; return rc; }

    // ---- advance the stream position ----
    c->nco_theta += (uint32_t)frames_in * c->nco_dtheta;
    c->pnco_theta += (uint32_t)(uint64_t)k.p.n_emit * c->nco_dtheta;
    c->rem = k.p.rem_next;
    c->phi = k.p.phi_next;
    c->total_in += (uint64_t)frames_in; c->total_out += (uint64_t)k.p.n_emit;
    *frames_out = (size_t)k.p.n_emit;
    return IQGPU_OK;
}

int process_device_impl(iqgpu_chain *c, const void *d_raw_in, size_t frames_in,
                               void *d_out, size_t out_capacity_bytes, size_t *frames_out, const CallOpts &o)
{
    // (a measuring or seeking call keeps the AGC out: the whole call in one piece, process_one -- but for a shadow call, which is cut
    //  as the ordinary call at its position is)
    const bool shadow = o.agc == AgcMode::Shadow;
    if (!(c->agc_fusable || c->agc_fusable_filter) || frames_in == 0 || (o.agc != AgcMode::Ordinary && !shadow))
        return process_one(c, d_raw_in, frames_in, d_out, out_capacity_bytes, frames_out, o, false);
    // output AGC on the specialised front kernel: the scanning phase (and the chunk that locks) through the unfused
    // kernels, everything behind it fused
    *frames_out = 0;
    bool locks = false;
    const size_t head = agc_call_cut(c, c->agc_locked_host, c->agc_seen_host, StreamPos{c->rem, c->phi, c->fpending}, frames_in, &locks);
    const size_t ibps = bytes_per_frame(c->desc.in_format), obps = bytes_per_frame(c->desc.out_format);
    if (!shadow && (size_t)plan_call(c, frames_in).n_emit * obps > out_capacity_bytes)
        return fail(IQGPU_ECAPACITY, "output buffer too small: need %zu bytes, have %zu", (size_t)plan_call(c, frames_in).n_emit * obps,
            out_capacity_bytes);
    size_t n1 = 0, n2 = 0;
    // (the I/Q probe's block is the head of the WHOLE call: the first piece stages it, counting the call's frames -- the kernel reads
    //  the 1024 frames at d_raw_in, whichever piece they fall into -- and the piece behind it stays out)
    CallOpts o1 = o, o2 = o;
    o1.probe_span = frames_in;
    if (head > 0) o2.no_probe = true;
    if (shadow) {
        // the rows of the call in chunk order: the head is a whole number of chunks, the second piece's rows stand behind them
        if (!o.rows) {
            const int rc = c->agc_rows.ensure((((size_t)frames_in + (size_t)c->agc_chunk - 1) / (size_t)c->agc_chunk) * sizeof(AgcRow));
            if (rc) return rc;
            o1.rows = (AgcRow *)c->agc_rows.p;
        }
        o2.rows = o1.rows + head / (size_t)c->agc_chunk;
    }
    if (head > 0) {
        const int rc = process_one(c, d_raw_in, head, d_out, out_capacity_bytes, &n1, o1, false);
        if (rc) return rc;
        c->agc_seen_host += n1;
        if (locks) c->agc_locked_host = true;
    }
    if (head < frames_in) {
        const int rc = process_one(c, (const char *)d_raw_in + head * ibps, frames_in - head, shadow ? nullptr : (char *)d_out + n1 * obps,
                                   shadow ? 0 : out_capacity_bytes - n1 * obps, &n2, o2, true);
        if (rc) return rc;
        c->agc_seen_host += n2;
    }
    *frames_out = n1 + n2;
    return IQGPU_OK;
}

extern "C" int iqgpu_chain_process_device(iqgpu_chain *c, const void *d_raw_in, size_t frames_in,
                                          void *d_out, size_t out_capacity_bytes, size_t *frames_out)
{
    if (!c || !frames_out) return fail(IQGPU_EINVAL, "iqgpu_chain_process_device: NULL argument");
    int rc = pipe_advance(c, c->pipe_seq); if (rc) return rc;     // batches submitted earlier come first (same stream)
    rc = agc_resolve_pending(c); if (rc) return rc;               // ... with whatever their last fused launch still owes
    return process_device_impl(c, d_raw_in, frames_in, d_out, out_capacity_bytes, frames_out);
}

int stage_host_input(iqgpu_chain *c, const void *in, size_t frames, const void **d_in)
{
    const size_t bytes = frames * bytes_per_frame(c->desc.in_format);
    const int rc = c->stage_in.ensure(bytes); if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(c->stage_in.p, in, bytes, hipMemcpyHostToDevice, c->stream));
    *d_in = c->stage_in.p;
    return IQGPU_OK;
}

extern "C" int iqgpu_chain_process(iqgpu_chain *c, const void *raw_in, size_t frames_in,
                                   void *out, size_t out_capacity_bytes, size_t *frames_out)
{
    if (!c || !frames_out) return fail(IQGPU_EINVAL, "iqgpu_chain_process: NULL argument");
    *frames_out = 0;
    if (frames_in == 0) return IQGPU_OK;
    if (!raw_in || !out) return fail(IQGPU_EINVAL, "iqgpu_chain_process: NULL buffer");
    HIP_TRY(hipSetDevice(c->device));
    int rc = pipe_advance(c, c->pipe_seq); if (rc) return rc;     // batches submitted earlier come first
    const size_t obps = bytes_per_frame(c->desc.out_format);
    const size_t n_emit = (size_t)plan_call(c, frames_in).n_emit;
    if (n_emit * obps > out_capacity_bytes)
        return fail(IQGPU_ECAPACITY, "output buffer too small: need %zu bytes, have %zu", n_emit * obps, out_capacity_bytes);
    rc = c->stage_out.ensure(n_emit * obps + 16); if (rc) return rc;         // (both buffers sized before anything is queued)
    const void *d_in = nullptr;
    rc = stage_host_input(c, raw_in, frames_in, &d_in); if (rc) return rc;
    size_t produced = 0;
    // the host waits for this call's bytes anyway: the AGC verdict is read here and the fallback launched only when it is set
    CallOpts o; o.host_verdict = true;
    rc = process_device_impl(c, d_in, frames_in, c->stage_out.p, c->stage_out.cap, &produced, o);
    if (rc) return rc;
    rc = agc_resolve_pending(c); if (rc) return rc;
    if (produced) HIP_TRY(hipMemcpyAsync(out, c->stage_out.p, produced * obps, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *frames_out = produced;
    return IQGPU_OK;
}
