// front_route_dump.cpp -- every plan of a grid of calls, one line each: the route and the run geometry Call::plan_geometry gives
// (chain.hpp, plan.cpp), the DC blocker's segments (dc_geom) and, behind a fused-AGC launch on one kernel, the fallback's plan.
// Host arithmetic only: no device, no HIP call (the chains are designed, never created).  Two commits that print the same lines
// route and plan every call of the grid alike (profiles/front_route.md).  Build against the library's objects:
//   hipcc -std=c++17 -O1 -c tools/front_route_dump.cpp -o front_route_dump.o
//   hipcc front_route_dump.o iq_tool_amd/lib/obj/*.o -o tools/front_route_dump
//   tools/front_route_dump > plans.txt        (the counts per route: the '#' lines at the end)
#include "../iq_tool_amd/csrc/chain.hpp"

// ---- what this tool reads of a planned call beyond its public fields ----
static const char *route_name(const Call &k) { return route_info(k.route).name; }
static int n_routes() { return (int)(sizeof(kRouteInfo) / sizeof(kRouteInfo[0])); }
static int route_index(const Call &k) { return (int)k.route; }
static const char *route_label(int i)
{
    static const char *const l[] = {"Generic", "GenericLate", "S1", "S1S0", "Fat", "Mid", "P0", "P0Fft", "Cascade", "Cascade2", "S2"};
    return l[i];
}
// the plan of the fallback behind a fused-AGC launch of a one-kernel route (stage_agc_verify_and_fallback), false: the route has none to show
static bool fallback_plan(const Call &k, FrontArgs &fb)
{
    const RouteInfo &ri = route_info(k.route);
    if (!ri.wave || ri.casc || k.route == FrontRoute::P0Fft) return false;
    fb = k.cplan; fb.agc_fused = 0; fb.out_fmt = IQGPU_FMT_CF32;
    if (ri.fallback_tile) k.plan_s1(fb, ri.fallback_tile);
    return true;
}
// ---- end of that section ----

struct Sw { const char *name, *value; };
struct Case { const char *name; iqgpu_chain_desc d; std::vector<Sw> sw; };

static iqgpu_chain_desc desc(int in_fmt, int out_fmt, double in_rate, double target, double shift = 0.0)
{
    iqgpu_chain_desc d;
    iqgpu_chain_desc_init(&d);
    d.in_format = in_fmt; d.out_format = out_fmt; d.input_rate_hz = in_rate; d.target_rate_hz = target; d.shift_hz = shift;
    return d;
}
static iqgpu_chain_desc with_filter(iqgpu_chain_desc d, int type, float f1, float f2, int taps = 0, int impl = IQGPU_FILTER_IMPL_AUTO)
{
    d.n_filters = 1; d.filters[0] = iqgpu_filter_req{type, f1, f2};
    d.filter_taps = (taps != 0 && taps % 2 == 0) ? taps + 1 : taps; d.filter_impl = impl;
    return d;
}
static iqgpu_chain_desc with(iqgpu_chain_desc d, bool dc, bool agc, size_t block = 0, float gain = 1.0f)
{
    d.dc_block_enable = dc; d.agc_enable = agc; d.agc_profile = IQGPU_AGC_DIGITAL; d.block_samples = block; d.gain = gain;
    return d;
}

// What iqgpu_chain_create derives BEHIND its device calls and the plan reads: which chains fuse the AGC into their last kernel, and
// whether resampler and filter run as k_p0fft16.  The same host predicates in the same order (abi.cpp), none of the uploads
static void derive_create_flags(iqgpu_chain *c)
{
    const size_t Lt = c->fp.taps.size();
    bool overlap_save = false;
    if (c->fp.enabled && !c->sw.force_generic && Lt >= 2 && 2 * (Lt - 1) <= (size_t)kMaxFftN && (c->fp.block > 0 || Lt >= (size_t)kFftMinTaps)) {
        overlap_save = true;
        int lg = (c->sw.dbg & kDbgFftNoR16) ? 8 : 10;
        while ((size_t)(1 << lg) < 4 * (Lt - 1) && (1 << lg) < 4096) ++lg;
        while ((size_t)(1 << lg) < 2 * (Lt - 1)) ++lg;
        if (c->decim && c->S == 0 && !c->late && c->fp.post_resample && !(c->sw.dbg & (kDbgFftNoR16 | kDbgNoP0 | kDbgNoFusedMove)) &&
            ((c->sw.dbg & kDbgFuseFilter) || c->sw.fft_keep_geometry)) {
            FrontArgs ff{};
            ff.dbg = c->sw.dbg; ff.S = 0; ff.in_fmt = c->desc.in_format; ff.gain = c->desc.gain;
            ff.iq_enable = c->desc.iq_correct_enable ? 1 : 0; ff.dc_enable = c->dc ? 1 : 0; ff.nco_mode = c->nco_mode; ff.step = c->rp.step;
            const int lgf = lg < 12 ? 12 : lg;
            if (p0fft_shape(ff, lgf, (int)Lt) && p0fft_geometry(lgf, (int)Lt, &c->fuse_win, &c->fuse_vout)) { c->fuse_filter = (c->sw.dbg & kDbgFuseFilter) != 0; lg = lgf; }
        }
        if (c->sw.fft_log2n && (size_t)(1 << c->sw.fft_log2n) >= 2 * (Lt - 1)) lg = c->sw.fft_log2n;
        if (c->fuse_win > 0 && !p0fft_geometry(lg, (int)Lt, &c->fuse_win, &c->fuse_vout)) { c->fuse_filter = false; c->fuse_win = c->fuse_vout = 0; }
        c->fft_log2n = lg;
    }
    if (!c->agc) return;
    FrontArgs fa{};
    fa.dbg = c->sw.dbg; fa.S = c->S; fa.in_fmt = c->desc.in_format; fa.out_fmt = c->desc.out_format; fa.gain = c->desc.gain;
    fa.iq_enable = c->desc.iq_correct_enable ? 1 : 0; fa.dc_enable = c->dc ? 1 : 0;
    fa.nco_mode = c->nco_mode; fa.pnco_mode = c->pnco_mode; fa.agc_chunk_frames = c->agc_chunk; fa.agc_shift = c->S;
    if (c->cascade) { fa.S = 1; fa.in_fmt = IQGPU_FMT_CF32; }
    c->agc_fusable = c->agc_rms_alpha == 0.0f && c->decim && !c->late && !c->sw.force_generic && !c->fp.enabled &&
                     (c->cascade || c->S == 0 || (c->S == 1 && c->rp.stages[0].m == 10)) && front_s1_agc_fusable(fa);
    if (c->agc_rms_alpha == 0.0f && c->decim && !c->late && !c->sw.force_generic && c->fp.enabled && c->fp.post_resample && overlap_save &&
        fftconv_agc_fusable(c->fft_log2n, (int)Lt, c->sw.dbg))
        c->agc_fusable_filter = (double)c->agc_chunk * (double)c->ratio - (double)c->fp.block - 2.0 >= (double)(1 << c->fft_log2n);
}

static long g_plans = 0, g_by_route[16] = {0};

static void print_plan(const char *tag, const FrontArgs &a)
{
    printf(" %s[tt=%lld warm=%d etpw=%d ns=%lld q=%lld r=%lld wpw=%d wt=%d,%d,%d,%d wsum=%lld ta=%lld tb=%lld e1=%lld e=%lld p0=%lld,%lld,%lld lds=%d]", tag,
           (long long)a.w_total_tiles, a.w_warm_tiles, a.w_edge_tpw, (long long)a.w_n_stream, (long long)a.w_run_q, (long long)a.w_run_r, a.w_wpw,
           a.w_wt[0], a.w_wt[1], a.w_wt[2], a.w_wt[3], (long long)a.w_wsum, (long long)a.w_edge_ta, (long long)a.w_edge_tb, (long long)a.w_n_edge1,
           (long long)a.w_n_edge, (long long)a.p0_k_a, (long long)a.p0_k_b, (long long)a.p0_f_max, a.casc_wave_lds);
}

// one call as process_one sets it up (begin_call, the AGC's part of it), planned
static void plan_one(iqgpu_chain *c, const char *label, const char *mode, AgcMode agc, bool agc_fused, const StreamPos &at, size_t frames, uintptr_t addr)
{
    c->rem = at.rem; c->phi = at.phi; c->fpending = at.fpending;
    Call k{};
    k.c = c; k.d_raw_in = (const void *)addr; k.frames_in = frames; k.o.agc = agc;
    k.p = plan_call(c, frames);
    k.filt = c->fp.enabled; k.L1 = k.filt ? c->fp.taps.size() - 1 : 0; k.fpending0 = c->fpending;
    k.fin_fmt = c->desc.out_format;
    k.agc_fused = agc_fused;
    if (c->agc && !agc_fused) k.fin_fmt = IQGPU_FMT_CF32;
    k.plan_geometry();
    const DcGeom g = k.dc_geom();
    printf("%s cu=%d %s rem=%d phi=%llu fp=%llu n=%zu al=%d | %s wtile=%d rem_k=%d K=%d tpb=%d nb=%d s2t=%lld", label, c->n_cu, mode, at.rem,
           (unsigned long long)at.phi, (unsigned long long)at.fpending, frames, (int)(addr & 15), route_name(k), k.wtile, k.rem_k, k.casc_K, k.tpb,
           k.n_blocks, (long long)k.s2_in_tiles);
    print_plan("plan", k.cplan);
    printf(" dc[%d %d %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %d %d %d]", g.mode, g.n_seg, (long long)g.frames_in, (long long)g.seg_first,
           (long long)g.seg_len, (long long)g.n_edge1, (long long)g.n_stream, (long long)g.edge_tpw, (long long)g.run_q, (long long)g.run_r, (long long)g.ta,
           (long long)g.tb, g.warm, g.rem0, g.tile);
    FrontArgs fb;
    if (k.front_fused() && fallback_plan(k, fb)) print_plan("fallback", fb);
    printf("\n");
    ++g_plans; ++g_by_route[route_index(k)];
}

static void run_case(const Case &cs, int n_cu, size_t block, bool steal)
{
    iqgpu_debug_set(nullptr, nullptr);
    for (const Sw &s : cs.sw) if (iqgpu_debug_set(s.name, s.value) != IQGPU_OK) { fprintf(stderr, "%s: %s\n", cs.name, iqgpu_last_error()); exit(1); }
    if (steal) iqgpu_debug_set("steal", "1");
    iqgpu_chain_desc d = cs.d;
    if (block != (size_t)-1) d.block_samples = block;
    iqgpu_chain *c = new iqgpu_chain();
    if (design_chain(c, &d) != IQGPU_OK) { fprintf(stderr, "%s: %s\n", cs.name, iqgpu_last_error()); exit(1); }
    c->n_cu = n_cu;
    derive_create_flags(c);
    char label[160];
    snprintf(label, sizeof(label), "%s bs=%zu steal=%d", cs.name, (size_t)d.block_samples, steal ? 1 : 0);

    std::vector<size_t> lens = {1, 255, 256, 4095, ((size_t)1 << 16) + 1, (size_t)1 << 20};
    const size_t thr[] = {(size_t)kFatMinTilesPerWave * kFatTile * (size_t)n_cu * (size_t)front_fat_waves(),      // k_front_fat
                          (size_t)6 * (size_t)front_mid_tile(6) * (size_t)n_cu * (size_t)front_mid_waves(),       // k_front_mid, six per lane
                          (size_t)6 * (size_t)front_mid_tile(8) * (size_t)n_cu * (size_t)front_mid_waves(),       // ... eight
                          (size_t)1 << 22};                                                                        // k_front_p0, k_p0fft16
    for (size_t t : thr) { lens.push_back(t - 1); lens.push_back(t); lens.push_back(t + 1); }
    lens.push_back((size_t)1 << 24); lens.push_back((size_t)1 << 28); lens.push_back((size_t)1 << 31);

    std::vector<StreamPos> pos = {StreamPos{}};
    const int rem = c->decim && c->D > 1 ? c->D - 1 : 0;
    const uint64_t phi = c->resample ? c->rp.step / 3 : 0, fp = (c->fp.enabled && c->fp.block) ? c->fp.block / 2 : 0;
    if (phi) pos.push_back(StreamPos{0, phi, 0});
    if (rem || phi || fp) pos.push_back(StreamPos{rem, phi, fp});
    if (rem) pos.push_back(StreamPos{1, 0, fp});

    const bool fusable = c->agc_fusable || c->agc_fusable_filter;
    for (const StreamPos &at : pos)
        for (size_t n : lens)
            for (uintptr_t addr : {(uintptr_t)0x10000, (uintptr_t)0x10004}) {
                plan_one(c, label, "ordinary", AgcMode::Ordinary, false, at, n, addr);
                if (!fusable) continue;
                plan_one(c, label, "past_lock", AgcMode::Ordinary, true, at, n, addr);
                // (a shadow call: its pieces, planned as the ordinary call's -- but behind a filter, whose piece keeps the cf32 epilogue)
                plan_one(c, label, "shadow_head", AgcMode::Shadow, false, at, n, addr);
                plan_one(c, label, "shadow_past_lock", AgcMode::Shadow, !c->fp.enabled, at, n, addr);
                if (c->agc_fusable) plan_one(c, label, "measure_s1", AgcMode::MeasureS1, true, at, n, addr);
            }
    delete c;
}

int main()
{
    const int CU8 = IQGPU_FMT_CU8, CS8 = IQGPU_FMT_CS8, CS16 = IQGPU_FMT_CS16, CF32 = IQGPU_FMT_CF32, Q11 = IQGPU_FMT_SC16Q11;
    const int LP = IQGPU_FILTER_LOWPASS, BP = IQGPU_FILTER_PASSBAND;
    const double R = 2.4e6;
    auto hz = [&](double s, int S = 0) { return R / (s * (double)(1 << S)); };
    const std::vector<Sw> FF = {{"force_fat", "1"}}, FAT = {{"force_fat", "1"}, {"fat", "1"}}, S1 = {{"no_fat", "1"}}, C2 = {{"casc2_min_run", "2"}};
    std::vector<Case> cases = {
        // ---- tests/test_gpu_dispatch.py, CASES ----
        {"mid6-l3=4-nco", desc(CS16, CS16, R, hz(1.6, 1), 200e3), FF}, {"mid6-l3=5-nonco", desc(CS16, CS16, R, hz(1.8, 1)), FF},
        {"mid6-agc-unlocked", with(desc(CS16, CS16, R, hz(1.6125, 1), 200e3), false, true), FF},
        {"mid6-cf32", with_filter(desc(CS16, CF32, R, hz(1.7, 1)), LP, 200e3, 0), FF},
        {"mid6-cu8-cs8", desc(CU8, CS8, R, hz(1.55, 1), -150e3), FF}, {"mid6-cs8-cu8", desc(CS8, CU8, R, hz(1.9, 1)), FF},
        {"mid6-cs16-cu8", desc(CS16, CU8, R, hz(1.6, 1)), FF}, {"mid6-sc16q11", desc(Q11, CS16, R, hz(1.7, 1), 100e3), FF},
        {"mid6-gain", with(desc(CS16, CS16, R, hz(1.6, 1)), false, false, 0, 0.5f), FF},
        {"fat-4-6", desc(CS16, CS16, R, hz(1.63, 1), 200e3), FAT}, {"fat-5-6", desc(CS16, CS16, R, hz(1.7, 1)), FAT},
        {"fat-5-7", desc(CS16, CS16, R, hz(1.85, 1), 200e3), FAT},
        {"p0-2-3-4-cs8-cs16", desc(CS8, CS16, R, hz(1.1)), FF}, {"p0-2-3-5-cs16-cs16", desc(CS16, CS16, R, hz(1.29)), FF},
        {"p0-2-4-5-cu8-cu8", desc(CU8, CU8, R, hz(1.4)), FF}, {"p0-3-4-6-cu8-cs8", desc(CU8, CS8, R, hz(1.62)), FF},
        {"p0-3-5-6-cs16-cu8", desc(CS16, CU8, R, hz(1.7)), FF}, {"p0-3-5-7-cf32", with_filter(desc(CU8, CF32, R, hz(1.85)), LP, 300e3, 0), FF},
        {"p0-agc", with(desc(CU8, CU8, R, hz(1.6125)), false, true), FF},
        {"s1-fast", desc(CS16, CS16, R, hz(1.6125, 1), 200e3), S1}, {"s1-var1", desc(CS16, CS16, R, hz(1.6125, 1)), S1},
        {"s1-var2", desc(CU8, CU8, R, hz(1.6125)), S1}, {"s1-var3", desc(CS16, CU8, R, hz(1.6125)), S1},
        {"s1-var4", desc(CS16, CS16, R, hz(1.6125, 3), 50e3), {{"no_casc2", "1"}}},
        {"s1-var5", with(desc(CS16, CS16, R, hz(1.6125, 1), 200e3), true, false), S1}, {"s1-var6", with(desc(CS16, CS16, R, hz(1.6125, 1)), true, false), S1},
        {"s1-var7", desc(CU8, CU8, R, hz(1.6125), 200e3), S1}, {"s1-var8", with(desc(CU8, CU8, R, hz(1.6125), 200e3), true, false), S1},
        {"s1-var9", with(desc(CU8, CU8, R, hz(1.6125)), true, false), S1}, {"s1-var2-agc", with(desc(CU8, CU8, R, hz(1.6125)), false, true), S1},
        {"s2-cs8-spec0", desc(CS8, CS16, R, hz(1.6125, 2)), {}}, {"s2-cs16-spec2", desc(CS16, CS16, R, hz(1.6125, 2)), {}},
        {"s2-cs16-spec3", desc(CS16, CS16, R, hz(1.7, 2), 100e3), {}}, {"s2-cu8-spec6", desc(CU8, CU8, R, hz(1.6125, 2)), {}},
        {"s2-cu8-spec7", desc(CU8, CU8, R, hz(1.85, 2), -100e3), {}}, {"s2-cs16-spec4", with_filter(desc(CS16, CF32, R, hz(1.6125, 2)), LP, 100e3, 0), {}},
        {"s2-cf32-in", desc(CF32, CS16, R, hz(1.6125, 2)), {}},
        {"casc2-K2-cu8", with(desc(CU8, CS16, R, hz(1.6125, 3)), false, false, 65536), C2},
        {"casc2-K3-cs8", with(desc(CS8, CS16, R, hz(1.6125, 4)), false, false, 65536), C2},
        {"casc2-K4-cs16", with(desc(CS16, CS16, R, hz(1.6125, 5)), false, false, 65536), C2},
        {"fft16-N=2^10", with_filter(desc(CS16, CF32, R, hz(1.6125, 1)), LP, 200e3, 0, 301), {{"fft_log2n", "10"}}},
        {"fft16-N=2^11", with_filter(desc(CS16, CF32, R, hz(1.6125, 1)), LP, 200e3, 0, 301), {{"fft_log2n", "11"}}},
        {"fft16-N=2^12", with_filter(desc(CS16, CF32, R, hz(1.6125, 1)), LP, 200e3, 0, 301), {{"fft_log2n", "12"}}},
        {"fft16-N=2^13", with_filter(desc(CS16, CF32, R, hz(1.6125, 1)), LP, 200e3, 0, 301), {{"fft_log2n", "13"}}},
        {"fft16-N=2^14", with_filter(desc(CS16, CF32, R, hz(1.6125, 1)), LP, 200e3, 0, 301), {{"fft_log2n", "14"}}},
        // ---- tests/test_gpu_seek.py, CASES ----
        {"seek-nrsc5_s1", desc(CS16, CS16, R, 744187.5, 200e3), {}}, {"seek-nrsc5_mid", desc(CS16, CS16, R, 744187.5, 200e3), FF},
        {"seek-nrsc5_fat", desc(CS16, CS16, R, 744187.5, 200e3), FAT}, {"seek-cu8_s0_s1", desc(CU8, CU8, R, 1488375.0), {{"no_p0", "1"}}},
        {"seek-cu8_s0_p0", desc(CU8, CU8, R, 1488375.0), FF}, {"seek-s2", desc(CS16, CS16, 10e6, 2.4e6, -300e3), {}},
        {"seek-s2_two_kernels", desc(CS16, CS16, 10e6, 2.4e6, -300e3), {{"no_s2", "1"}}},
        {"seek-cascade2", with(desc(CU8, CS16, 61.44e6, 1488375.0), false, false, 40 * 8192), {}},
        {"seek-fir4097_behind", with_filter(desc(CU8, CU8, 61.44e6, 1488375.0), LP, 300e3, 0, 4097, IQGPU_FILTER_IMPL_FIR), {}},
        {"seek-fft1025_behind", with_filter(desc(CS16, CS16, 10e6, 2.4e6, -300e3), BP, 158.5e3, 113e3, 1024), {}},
        {"seek-interp", desc(CS16, CS16, 2.0e6, 2.4e6, 150e3), {}},                                      // (r >= 1)
        {"seek-generic", desc(CS16, CS16, R, 744187.5, 200e3), {{"force_generic", "1"}}},
        // ---- tests/test_gpu_seek_dcagc.py, ROUTINGS (rates of a 96 kS/s stream) ----
        {"dcagc-nrsc5_cs16_mid", with(desc(CS16, CS16, 96e3, 744187.5 * 0.04, 200e3 * 0.04), true, true), FF},
        {"dcagc-cu8_nrsc5_p0", with(desc(CU8, CU8, 96e3, 1488375.0 * 0.04), true, true), FF},
        {"dcagc-usb_filter_epilogue", with(with_filter(desc(CS16, CS16, 96e3, 744187.5 * 0.04), BP, 158.5e3f * 0.04f, 113e3f * 0.04f), true, true), FF},
        {"dcagc-am_cascade", with(desc(CS16, CS16, 96e3, 46511.71875 * 0.04), true, true), {}},
        {"dcagc-interp", with(desc(CS16, CS16, 96e3, 2.4e6 * 0.04 * 1.2, 150e3 * 0.04), true, true), {}},
        {"dcagc-agc_nofuse", with(desc(CS16, CS16, 96e3, 744187.5 * 0.04, 200e3 * 0.04), true, true), {{"agc_nofuse", "1"}}},
        // ---- beyond the tests' tables: the AGC without the blocker on every fused route, k_p0fft16, the eight-per-lane experiment ----
        {"agc-am_cascade", with(desc(CS16, CS16, R, 46511.71875), false, true), {}},
        {"agc-usb_filter_epilogue", with(with_filter(desc(CS16, CS16, R, 744187.5), BP, 158.5e3, 113e3), false, true), {}},
        {"agc-fat", with(desc(CS16, CS16, R, hz(1.63, 1), 200e3), false, true), {{"fat", "1"}}},
        {"p0fft-cu8-usb", with_filter(desc(CU8, CU8, R, 1488375.0), BP, 158.5e3, 113e3), {{"fuse_filter", "1"}}},
        {"p0fft-cu8-lsb-agc", with(with_filter(desc(CU8, CU8, R, 1488375.0), BP, -158.5e3, 113e3), false, true), {{"fuse_filter", "1"}}},
        {"mid8", desc(CS16, CS16, R, hz(1.7, 1)), {{"mid8", "1"}}},
        {"headline", desc(CS16, CS16, R, 744187.5, 200e3), {}},
    };
    // (the tables' cases with fields the helpers above do not set)
    {
        Case c{"seek-no_resample_pre_filter", with_filter(desc(CS16, CF32, R, R, -250e3), BP, -300e3, 100e3, 0, IQGPU_FILTER_IMPL_FFT), {}};   // (pointwise)
        c.d.no_resample = 1; c.d.transition_width_hz = 20e3f; c.d.attenuation_db = 70.0f; c.d.fft_size = 2048;
        cases.push_back(c);
        Case n{"seek-post_nco", desc(CS16, CS16, R, 744187.5, 200e3), {}}; n.d.shift_after_resample = 1; cases.push_back(n);
        Case f{"seek-post_nco_behind_fft", with_filter(desc(CS16, CF32, 10e6, 2.4e6, -300e3), BP, 158.5e3, 113e3, 1024), {}}; f.d.shift_after_resample = 1;
        cases.push_back(f);
        Case q{"dcagc-nrsc5_iq_correct", with(desc(CS16, CS16, 96e3, 744187.5 * 0.04, 200e3 * 0.04), true, true), FF};
        q.d.iq_correct_enable = 1; q.d.iq_mag = 0.02f; q.d.iq_phase = -0.015f; cases.push_back(q);
    }
    for (const Case &cs : cases)
        for (int n_cu : {256, 8}) {
            run_case(cs, n_cu, (size_t)-1, false);                                   // the case's own block_samples
            for (size_t block : {(size_t)0, (size_t)65536, (size_t)262144})
                for (bool steal : {false, true})
                    if (block != cs.d.block_samples || steal) run_case(cs, n_cu, block, steal);
        }
    iqgpu_debug_set(nullptr, nullptr);
    printf("# %ld plans\n", g_plans);
    for (int i = 0; i < n_routes(); ++i) printf("# %-12s %ld\n", route_label(i), g_by_route[i]);
    return 0;
}
