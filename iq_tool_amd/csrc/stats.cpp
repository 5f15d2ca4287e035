// stats.cpp -- host side of the capture-statistics accumulator (include/iqgpu.h "capture statistics"; kernels stats.hip):
// the iqgpu_stats handle -- stream position, the totals, the open page's columns in two buffers, the slab of a launch -- with
// push / push_device / read / reset under iqgpu_psd's stream rules, and the two host-only calls, merge and derive.  Independent of
// any chain.
#include "accum_core.hpp"
#include "chain.hpp"
#include "stats.hpp"

struct iqgpu_stats {
    AccumCore core;
    int open_cur = 0;                     // which of the two open-column buffers holds the open page (the page kernel writes the other)
    Event staged;                         // a host push: the slice has left the caller's memory
    // state: StatsTotals, then 2 x [5][kStatsColumns] doubles; slab: [groups][512] uint32, [groups] StatsPartial, [pages][5] doubles
    DevBuf state, slab, stage;
    StatsTotals *totals() const { return (StatsTotals *)state.p; }
    double *open_cols(int i) const { return (double *)((char *)state.p + sizeof(StatsTotals)) + (size_t)i * 5 * kStatsColumns; }
    static constexpr size_t kStateBytes = sizeof(StatsTotals) + 2 * 5 * kStatsColumns * sizeof(double);
    uint32_t *slab_hist() const { return (uint32_t *)slab.p; }
    StatsPartial *slab_part() const { return (StatsPartial *)(slab_hist() + (size_t)kStatsMaxGroups * 512); }
    double *slab_sums() const { return (double *)(slab_part() + kStatsMaxGroups); }
    static constexpr size_t kSlabBytes = (size_t)kStatsMaxGroups * (512 * sizeof(uint32_t) + sizeof(StatsPartial)) + (size_t)kStatsMaxPages * 5 * sizeof(double);
    IQGPU_LOCAL ~iqgpu_stats() { core.close(); }      // the waits first: the members free themselves behind them
};
static_assert(sizeof(StatsTotals) % sizeof(double) == 0 && sizeof(StatsPartial) % sizeof(double) == 0, "the doubles behind them stay aligned");

namespace {

constexpr size_t kPushSliceFrames = (size_t)1 << 22;     // of a host push: frames staged per slice
const char *const kReset = "iqgpu_stats_reset";

AccumCore *core(iqgpu_stats *p) { return p ? &p->core : nullptr; }

// the state of a handle without frames, queued on `own`
int zero_state(iqgpu_stats *p)
{
    StatsTotals t;
    memset(&t, 0, sizeof(t));
    t.pk = -1.0; t.pkf = 0;
    t.mn[0] = t.mn[1] = INFINITY; t.mx[0] = t.mx[1] = -INFINITY;
    HIP_TRY(hipMemsetAsync(p->state.p, 0, iqgpu_stats::kStateBytes, p->core.own));
    HIP_TRY(hipMemcpyAsync(p->state.p, &t, sizeof(t), hipMemcpyHostToDevice, p->core.own));
    HIP_TRY(hipStreamSynchronize(p->core.own));              // (t is on this stack)
    return IQGPU_OK;
}

// n frames of device memory behind everything pushed so far, on s
int push_frames(iqgpu_stats *p, const void *d_raw, size_t n, hipStream_t s)
{
    AccumCore &core = p->core;
    const int rc = core.note_stream(s); if (rc) return rc;
    const uint64_t P = kStatsPageFrames;
    core.poisoned = true;                                                          // (until the last launch of the push is queued)
    for (size_t at = 0; at < n;) {
        const uint64_t first = core.frames;
        const uint64_t room = (uint64_t)kStatsMaxPages * P - first % P;           // whole pages up to the slab's bound
        const uint64_t cnt = n - at < room ? n - at : room;
        StatsPagesArgs a{};
        a.raw = (const char *)d_raw + at * core.bps; a.first = (int64_t)first; a.n = (int64_t)cnt; a.fmt = core.format;
        int groups = 0;
        stats_grid(a.first, a.n, &groups, &a.pages_per_group);
        a.open_in = p->open_cols(p->open_cur); a.open_out = p->open_cols(p->open_cur ^ 1);
        a.hist = p->slab_hist(); a.part = p->slab_part(); a.page_sum = p->slab_sums();
        HIP_TRY(launch_stats_pages(a, s));
        StatsFoldArgs f{};
        f.hist = a.hist; f.part = a.part; f.page_sum = a.page_sum; f.groups = groups;
        f.n_pages = (int32_t)((first + cnt) / P - first / P); f.tot = p->totals();
        HIP_TRY(launch_stats_fold(f, s));
        if ((first + cnt) % P != 0) p->open_cur ^= 1;                             // the launch left an open page, in the other buffer
        core.frames = first + cnt;
        at += (size_t)cnt;
    }
    core.poisoned = false;
    return IQGPU_OK;
}

bool has_finite(const iqgpu_stats_result *r) { return r->frames > r->nonfinite_frames; }

} // namespace

extern "C" void iqgpu_stats_geometry(size_t *frames_per_page)
{
    if (frames_per_page) *frames_per_page = (size_t)kStatsPageFrames;
}

extern "C" int iqgpu_stats_create(int device, int format, iqgpu_stats **out)
{
    const char *who = "iqgpu_stats_create";
    if (out) *out = nullptr;
    if (!out) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    iqgpu_stats *p = new (std::nothrow) iqgpu_stats;
    int rc = AccumCore::open(core(p), device, format, who);
    if (rc == IQGPU_OK) {
        const hipError_t e = p->staged.create(hipEventDisableTiming);
        if (e != hipSuccess) rc = fail(IQGPU_EHIP, "%s: %s", who, hipGetErrorString(e));
    }
    if (rc == IQGPU_OK) rc = p->state.ensure(iqgpu_stats::kStateBytes);
    if (rc == IQGPU_OK) rc = p->slab.ensure(iqgpu_stats::kSlabBytes);
    if (rc == IQGPU_OK) rc = zero_state(p);
    if (rc != IQGPU_OK) { delete p; return rc; }
    *out = p;
    return IQGPU_OK;
}

extern "C" void iqgpu_stats_destroy(iqgpu_stats *p) { delete p; }

extern "C" int iqgpu_stats_reset(iqgpu_stats *p)
{
    if (!p) return fail(IQGPU_EINVAL, "iqgpu_stats_reset: NULL argument");
    int rc = p->core.begin_reset(); if (rc) return rc;
    rc = zero_state(p); if (rc) return rc;
    p->core.rewind(); p->open_cur = 0;
    return IQGPU_OK;
}

extern "C" int iqgpu_stats_push_device(iqgpu_stats *p, const void *d_raw, size_t frames, void *hip_stream)
{
    if (p && frames == 0) return IQGPU_OK;
    const int rc = AccumCore::guard(core(p), d_raw, "iqgpu_stats_push_device", kReset); if (rc) return rc;
    return push_frames(p, d_raw, frames, (hipStream_t)hip_stream);
}

extern "C" int iqgpu_stats_push(iqgpu_stats *p, const void *raw, size_t frames)
{
    if (p && frames == 0) return IQGPU_OK;
    int rc = AccumCore::guard(core(p), raw, "iqgpu_stats_push", kReset); if (rc) return rc;
    const size_t bps = p->core.bps;
    const hipStream_t own = p->core.own;
    rc = p->stage.ensure((frames < kPushSliceFrames ? frames : kPushSliceFrames) * bps); if (rc) return rc;
    for (size_t at = 0; at < frames;) {
        const size_t n = frames - at < kPushSliceFrames ? frames - at : kPushSliceFrames;
        // (the one staging buffer: the copy is ordered behind the kernels of the slice in front on the handle's stream)
        HIP_TRY(hipMemcpyAsync(p->stage.p, (const char *)raw + at * bps, n * bps, hipMemcpyHostToDevice, own));
        HIP_TRY(hipEventRecord(p->staged, own));
        rc = push_frames(p, p->stage.p, n, own); if (rc) return rc;
        HIP_TRY(hipEventSynchronize(p->staged));                     // the caller's memory is free when the call returns
        at += n;
    }
    return IQGPU_OK;
}

extern "C" int iqgpu_stats_read(iqgpu_stats *p, iqgpu_stats_result *r)
{
    int rc = AccumCore::guard(core(p), r, "iqgpu_stats_read", kReset); if (rc) return rc;
    rc = p->core.settle(); if (rc) return rc;
    StatsTotals t;
    std::vector<double> cols;
    try { cols.resize(5 * (size_t)kStatsColumns); } catch (const std::bad_alloc &) { return fail(IQGPU_ENOMEM, "iqgpu_stats_read: out of host memory"); }
    HIP_TRY(hipMemcpy(&t, p->totals(), sizeof(t), hipMemcpyDeviceToHost));
    const bool open = p->core.frames % (uint64_t)kStatsPageFrames != 0;   // else the open columns hold a page already folded, or nothing
    if (open) HIP_TRY(hipMemcpy(cols.data(), p->open_cols(p->open_cur), cols.size() * sizeof(double), hipMemcpyDeviceToHost));
    memset(r, 0, sizeof(*r));
    r->frames = p->core.frames; r->nonfinite_frames = t.nonfinite;
    for (int c = 0; c < 2; ++c) {
        r->rail_lo[c] = t.rail_lo[c]; r->rail_hi[c] = t.rail_hi[c];
        for (int b = 0; b < 256; ++b) r->hist[c][b] = t.hist[c * 256 + b];
        if (t.finite) { r->min[c] = t.mn[c]; r->max[c] = t.mx[c]; }
    }
    if (t.finite) { r->peak_power = t.pk; r->peak_frame = t.pkf; }
    double s[5];
    for (int k = 0; k < 5; ++k) s[k] = open ? t.sum[k] + stats_tree(cols.data() + (size_t)k * kStatsColumns) : t.sum[k];
    r->sum[0] = s[0]; r->sum[1] = s[1]; r->sum_sq[0] = s[2]; r->sum_sq[1] = s[3]; r->sum_iq = s[4];
    return IQGPU_OK;
}

// ---- host only ----
extern "C" int iqgpu_stats_merge(iqgpu_stats_result *into, const iqgpu_stats_result *next)
{
    if (!into || !next) return fail(IQGPU_EINVAL, "iqgpu_stats_merge: NULL argument");
    const bool a = has_finite(into), b = has_finite(next);
    if (b) {
        for (int c = 0; c < 2; ++c) {
            into->min[c] = a ? fminf(into->min[c], next->min[c]) : next->min[c];
            into->max[c] = a ? fmaxf(into->max[c], next->max[c]) : next->max[c];
        }
        if (!a || next->peak_power > into->peak_power) {             // (a tie keeps the earlier frame: into's)
            into->peak_power = next->peak_power; into->peak_frame = into->frames + next->peak_frame;
        }
    }
    into->frames += next->frames; into->nonfinite_frames += next->nonfinite_frames;
    for (int c = 0; c < 2; ++c) {
        into->rail_lo[c] += next->rail_lo[c]; into->rail_hi[c] += next->rail_hi[c];
        for (int k = 0; k < 256; ++k) into->hist[c][k] += next->hist[c][k];
        into->sum[c] += next->sum[c]; into->sum_sq[c] += next->sum_sq[c];
    }
    into->sum_iq += next->sum_iq;
    return IQGPU_OK;
}

extern "C" int iqgpu_stats_derive(const iqgpu_stats_result *r, iqgpu_stats_derived *d)
{
    if (!r || !d) return fail(IQGPU_EINVAL, "iqgpu_stats_derive: NULL argument");
    memset(d, 0, sizeof(*d));
    for (int c = 0; c < 2; ++c)
        for (int k = 0; k < 256; ++k) d->bins_used[c] += r->hist[c][k] != 0;
    d->n = r->frames - r->nonfinite_frames;
    if (d->n == 0) return IQGPU_OK;
    const double n = (double)d->n;
    d->mean_i = r->sum[0] / n; d->mean_q = r->sum[1] / n;
    d->power = (r->sum_sq[0] + r->sum_sq[1]) / n;
    if (d->power > 0.0) d->rms_dbfs = 10.0 * std::log10(d->power);
    if (r->peak_power > 0.0) d->peak_dbfs = 10.0 * std::log10(r->peak_power);
    if (d->power > 0.0 && r->peak_power > 0.0) d->crest_db = d->peak_dbfs - d->rms_dbfs;
    d->var_i = r->sum_sq[0] / n - d->mean_i * d->mean_i;
    d->var_q = r->sum_sq[1] / n - d->mean_q * d->mean_q;
    if (d->var_q > 0.0 && d->var_i >= 0.0) d->iq_gain_ratio = std::sqrt(d->var_i / d->var_q);
    if (d->var_i > 0.0 && d->var_q > 0.0) {
        double rho = (r->sum_iq / n - d->mean_i * d->mean_q) / std::sqrt(d->var_i * d->var_q);
        rho = rho < -1.0 ? -1.0 : rho > 1.0 ? 1.0 : rho;
        d->iq_phase_rad = std::asin(rho);
    }
    d->clip_fraction = (double)(r->rail_lo[0] + r->rail_lo[1] + r->rail_hi[0] + r->rail_hi[1]) / (2.0 * n);
    return IQGPU_OK;
}
