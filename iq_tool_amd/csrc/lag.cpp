// lag.cpp -- host side of the lag-product accumulator (include/iqgpu.h "lag products"; kernels lag.hip): the options,
// the iqgpu_lag handle -- the row-page core (row_pages.hpp) with LagOpen records and LagCell cells, and the history of the last max_lag
// frames in two buffers -- what a launch's arguments are, how the open row is assembled, push / push_device / read_open / reset under
// iqgpu_env's rules, and the two host-only calls on finished rows: the frequency of a lag product and the estimate over a range of
// rows.  Independent of any chain.
#include <cmath>
#include <cstddef>
#include <memory>

#include "chain.hpp"
#include "lag.hpp"
#include "row_pages.hpp"

struct iqgpu_lag {
    RowPages rp;                          // (its open_cur also says which half of hist holds the history: a launch writes the other)
    int n_lags = 0;
    int32_t lags[kLagMaxLags] = {0, 0, 0, 0};
    // hist: 2 x max_lag frames of raw bytes, frame k of a half being stream frame `frames` - max_lag + k
    DevBuf hist;
    int max_lag() const { return lags[n_lags - 1]; }
    LagOpen *open(int i) const { return (LagOpen *)rp.open_rec(i); }
    char *history(int i) const { return (char *)hist.p + (size_t)i * hist_bytes(); }
    size_t hist_bytes() const { return ((size_t)max_lag() * rp.bps + 15) & ~(size_t)15; }
    IQGPU_LOCAL ~iqgpu_lag() { rp.close(); }          // the waits first: the members free themselves behind them
};
static_assert(sizeof(LagOpen) % sizeof(double) == 0 && (kEnvMaxGroups * sizeof(uint32_t)) % sizeof(double) == 0, "what lies behind them stays aligned");
static_assert(offsetof(LagOpen, tot) + sizeof(LagOpen::tot) == sizeof(LagOpen), "the total is the record's last part");

namespace {

constexpr size_t kPushSliceFrames = (size_t)1 << 22;     // of a host push: frames staged per slice (its rows come back per slice)
constexpr double kTwoPi = 6.283185307179586476925286766559;
const char *const kReset = "iqgpu_lag_reset";
const char *const kMaxRows = "iqgpu_lag_max_rows";

RowPages *core(iqgpu_lag *p) { return p ? &p->rp : nullptr; }

int check_opts(const iqgpu_lag_opts *o, const char *who)
{
    if (!o) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    const int rc = RowPages::check_block(o->block_frames, who); if (rc) return rc;
    if (o->n_lags < 1 || o->n_lags > (uint32_t)kLagMaxLags) return fail(IQGPU_EINVAL, "%s: n_lags %u is outside 1 .. %d", who, o->n_lags, kLagMaxLags);
    for (uint32_t l = 0; l < o->n_lags; ++l) {
        if (o->lags[l] < 1 || o->lags[l] > (uint32_t)kLagMaxLag) return fail(IQGPU_EINVAL, "%s: lag %u is outside 1 .. %d", who, o->lags[l], kLagMaxLag);
        if (l && o->lags[l] <= o->lags[l - 1]) return fail(IQGPU_EINVAL, "%s: the lags must be strictly increasing", who);
    }
    return IQGPU_OK;
}

// n frames of device memory behind everything pushed so far, on s; the rows they finish into the device planes (either may be NULL)
int push_frames(iqgpu_lag *p, const void *d_raw, size_t n, float *d_lag, float *d_sum, hipStream_t s)
{
    RowPages &rp = p->rp;
    const uint64_t L = (uint64_t)p->max_lag();
    return rp.push(d_raw, n, s, [&](const RowLaunch &u) {
        LagRowsArgs a{};
        a.raw = u.raw; a.hist = p->history(rp.open_cur); a.first = (int64_t)u.first; a.n = (int64_t)u.cnt; a.fmt = rp.format; a.log2_b = rp.log2_b;
        a.pages_per_group = u.pages_per_group; a.n_lags = p->n_lags; a.max_lag = p->max_lag();
        for (int l = 0; l < p->n_lags; ++l) a.lags[l] = p->lags[l];
        a.open_in = p->open(rp.open_cur); a.open_out = p->open(rp.open_cur ^ 1);
        a.cells = (LagCell *)rp.slab_cells(); a.row_lag = d_lag; a.row_sum = d_sum; a.nonfinite = rp.slab_nonfinite();
        HIP_TRY(launch_lag_rows(a, s));
        if (u.cf32 || a.cells) {
            LagFoldArgs f{};
            rp.fill_fold(u, &f);
            f.cells = a.cells; f.n_lags = p->n_lags; f.open_in = a.open_in; f.open_out = a.open_out; f.row_lag = d_lag; f.row_sum = d_sum;
            HIP_TRY(launch_lag_fold(f, s));
        }
        // the history behind the launch, into the other half: the last max_lag frames of the stream.  A launch shorter than that
        // keeps the tail of the old history in front of its own frames
        char *h_old = p->history(rp.open_cur), *h_new = p->history(rp.open_cur ^ 1);
        if (u.cnt >= L) {
            HIP_TRY(hipMemcpyAsync(h_new, u.raw + (u.cnt - L) * rp.bps, L * rp.bps, hipMemcpyDeviceToDevice, s));
        } else {
            HIP_TRY(hipMemcpyAsync(h_new, h_old + u.cnt * rp.bps, (L - u.cnt) * rp.bps, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(h_new + (L - u.cnt) * rp.bps, u.raw, u.cnt * rp.bps, hipMemcpyDeviceToDevice, s));
        }
        if (d_lag) d_lag += u.done * 2 * (uint64_t)p->n_lags;
        if (d_sum) d_sum += u.done;
        return (int)IQGPU_OK;
    });
}

} // namespace

extern "C" void iqgpu_lag_opts_init(iqgpu_lag_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->block_frames = (uint32_t)1 << kEnvLog2BlockDefault;
    o->n_lags = 1; o->lags[0] = 1;
}

extern "C" int iqgpu_lag_rows(const iqgpu_lag_opts *o, uint64_t frames, uint64_t *rows)
{
    const int rc = check_opts(o, "iqgpu_lag_rows"); if (rc) return rc;
    if (!rows) return fail(IQGPU_EINVAL, "iqgpu_lag_rows: NULL argument");
    *rows = frames >> RowPages::log2_block(o->block_frames);
    return IQGPU_OK;
}

extern "C" int iqgpu_lag_create(int device, int format, const iqgpu_lag_opts *o, iqgpu_lag **out)
{
    const char *who = "iqgpu_lag_create";
    if (out) *out = nullptr;
    if (!out) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    int rc = check_opts(o, who); if (rc) return rc;
    iqgpu_lag *p = new (std::nothrow) iqgpu_lag;
    if (p) {
        p->n_lags = (int)o->n_lags;
        for (int l = 0; l < p->n_lags; ++l) p->lags[l] = (int32_t)o->lags[l];
    }
    rc = RowPages::open(core(p), device, format, o->block_frames, sizeof(LagOpen), sizeof(LagCell), who);
    if (rc == IQGPU_OK) rc = p->hist.ensure(2 * p->hist_bytes());
    if (rc == IQGPU_OK) rc = p->rp.zero_state();
    if (rc != IQGPU_OK) { delete p; return rc; }
    *out = p;
    return IQGPU_OK;
}

extern "C" void iqgpu_lag_destroy(iqgpu_lag *p) { delete p; }

// (frames = 0 empties the history: a frame in front of the stream's first is never a partner)
extern "C" int iqgpu_lag_reset(iqgpu_lag *p) { return RowPages::reset(core(p), "iqgpu_lag_reset"); }

extern "C" size_t iqgpu_lag_max_rows(const iqgpu_lag *p, size_t frames) { return p ? p->rp.rows_of(frames) : 0; }

extern "C" int iqgpu_lag_push_device(iqgpu_lag *p, const void *d_raw, size_t frames, float *d_row_lag, float *d_row_sum, size_t cap_rows,
                                     size_t *rows, void *hip_stream)
{
    size_t need = 0;
    const int rc = RowPages::begin_push(core(p), d_raw, frames, d_row_lag || d_row_sum, cap_rows, rows, &need, "iqgpu_lag_push_device", kReset, kMaxRows);
    if (rc) return rc;
    if (frames == 0) return IQGPU_OK;
    if (rows) *rows = need;
    return push_frames(p, d_raw, frames, d_row_lag, d_row_sum, (hipStream_t)hip_stream);
}

extern "C" int iqgpu_lag_push(iqgpu_lag *p, const void *raw, size_t frames, float *row_lag, float *row_sum, size_t cap_rows, size_t *rows)
{
    const char *who = "iqgpu_lag_push";
    size_t need = 0;
    int rc = RowPages::begin_push(core(p), raw, frames, row_lag || row_sum, cap_rows, rows, &need, who, kReset, kMaxRows); if (rc) return rc;
    if (frames == 0) return IQGPU_OK;
    RowPages &rp = p->rp;
    const size_t slice = frames < kPushSliceFrames ? frames : kPushSliceFrames;
    const size_t slice_rows = (slice >> rp.log2_b) + 1;              // rows of one slice, whatever the position
    const size_t per_row = 2 * (size_t)p->n_lags;
    rc = rp.stage.ensure(slice * rp.bps); if (rc) return rc;
    rc = rp.rows_out.ensure((per_row + 1) * slice_rows * sizeof(float)); if (rc) return rc;
    float *d_lag = row_lag ? (float *)rp.rows_out.p : nullptr, *d_sum = row_sum ? (float *)rp.rows_out.p + per_row * slice_rows : nullptr;
    if (rows) *rows = need;
    HostPlane planes[2] = {{(char *)row_lag, d_lag, per_row * sizeof(float)}, {(char *)row_sum, d_sum, sizeof(float)}};
    return push_host_slices(rp, rp.stage, raw, frames, kPushSliceFrames, slice_rows, planes, who, "finishes",
                            [&](size_t n) { return rp.rows_of(n); },
                            [&](const void *d_raw, size_t n) { return push_frames(p, d_raw, n, d_lag, d_sum, rp.own); });
}

extern "C" int iqgpu_lag_read_open(iqgpu_lag *p, double *lag, double *sum, iqgpu_lag_info *info)
{
    int rc = RowPages::guard(core(p), true, "iqgpu_lag_read_open", kReset); if (rc) return rc;
    RowPages &rp = p->rp;
    rc = rp.settle(); if (rc) return rc;
    const OpenRow r = rp.open_row();
    const int nc = 2 * p->n_lags + 1;
    if (lag || sum) {
        double v[kLagComps] = {0.0};
        if (r.has_tot || r.has_page) {
            const std::unique_ptr<LagOpen> rec(new (std::nothrow) LagOpen);
            if (!rec) return fail(IQGPU_ENOMEM, "iqgpu_lag_read_open: out of host memory");
            LagOpen &o = *rec;
            rc = rp.fetch_open(r, &o, offsetof(LagOpen, tot)); if (rc) return rc;
            for (int c = 0; c < nc; ++c) {
                if (r.has_tot) v[c] = o.tot[c];
                if (r.has_page) v[c] = v[c] + RowPages::open_tree(r, o.col[c]);
            }
        }
        if (sum) *sum = v[0];
        if (lag) for (int c = 1; c < nc; ++c) lag[c - 1] = v[c];
    }
    if (info) {
        uint64_t nonfinite = 0;
        if (rp.format == IQGPU_FMT_CF32) HIP_TRY(hipMemcpy(&nonfinite, rp.nonfinite_total(), sizeof(nonfinite), hipMemcpyDeviceToHost));
        memset(info, 0, sizeof(*info));
        info->frames = rp.frames; info->rows = rp.frames >> rp.log2_b; info->nonfinite_frames = nonfinite;
        info->open_frames = (uint32_t)r.open_frames; info->block_frames = (uint32_t)rp.B(); info->n_lags = (uint32_t)p->n_lags;
        for (int l = 0; l < p->n_lags; ++l) info->lags[l] = (uint32_t)p->lags[l];
    }
    return IQGPU_OK;
}

// ---- host only ----
extern "C" int iqgpu_lag_freq(double re, double im, uint32_t lag, double sample_rate, double *hz)
{
    const char *who = "iqgpu_lag_freq";
    if (!hz) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (!std::isfinite(re) || !std::isfinite(im) || !std::isfinite(sample_rate) || lag == 0 || !(sample_rate > 0.0))
        return fail(IQGPU_EINVAL, "%s: a non-finite value, lag 0 or a sample rate that is not positive", who);
    *hz = re == 0.0 && im == 0.0 ? 0.0 : std::atan2(im, re) / (kTwoPi * (double)lag) * sample_rate;
    return IQGPU_OK;
}

extern "C" int iqgpu_lag_estimate_rows(const float *row_lag, const float *row_sum, size_t rows, const iqgpu_lag_opts *o, uint32_t lag_index,
                                       size_t first_row, size_t n_rows, double sample_rate, iqgpu_lag_estimate *out)
{
    const char *who = "iqgpu_lag_estimate_rows";
    if (!row_lag || !out) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    const int rc = check_opts(o, who); if (rc) return rc;
    if (lag_index >= o->n_lags) return fail(IQGPU_EINVAL, "%s: lag_index %u with %u lags", who, lag_index, o->n_lags);
    if (first_row > rows || n_rows > rows - first_row) return fail(IQGPU_EINVAL, "%s: rows %zu .. + %zu of %zu", who, first_row, n_rows, rows);
    if (!std::isfinite(sample_rate) || !(sample_rate > 0.0)) return fail(IQGPU_EINVAL, "%s: a sample rate that is not positive", who);
    double re = 0.0, im = 0.0, power = 0.0;
    for (size_t r = first_row; r < first_row + n_rows; ++r) {
        const float fre = row_lag[(r * o->n_lags + lag_index) * 2], fim = row_lag[(r * o->n_lags + lag_index) * 2 + 1];
        if (fre != fre || fim != fim || (row_sum && row_sum[r] != row_sum[r])) continue;      // a row with a NaN value is skipped
        re += (double)fre; im += (double)fim;
        if (row_sum) power += (double)row_sum[r];
    }
    memset(out, 0, sizeof(*out));
    out->re = re; out->im = im; out->power = power;
    const int rf = iqgpu_lag_freq(re, im, o->lags[lag_index], sample_rate, &out->hz); if (rf) return rf;
    out->coherence = power > 0.0 ? std::hypot(re, im) / power : 0.0;
    out->span_hz = sample_rate / (double)o->lags[lag_index];
    return IQGPU_OK;
}
