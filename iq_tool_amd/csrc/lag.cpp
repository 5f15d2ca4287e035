// lag.cpp -- host side of the lag-product accumulator (include/iqgpu.h "lag products"; kernels lag.hip): the options and
// the row arithmetic (no device), the iqgpu_lag handle -- stream position, the open row in two buffers, the history of the last
// max_lag frames in two buffers, the slab of a launch -- with push / push_device / read_open / reset under iqgpu_env's rules, and the
// two host-only calls on finished rows: the frequency of a lag product and the estimate over a range of rows.  Independent of any chain.
#include <cmath>
#include <cstddef>
#include <memory>

#include "chain.hpp"
#include "lag.hpp"

struct iqgpu_lag {
    int device = 0, format = 0, log2_b = 0, n_lags = 0;
    int32_t lags[kLagMaxLags] = {0, 0, 0, 0};
    size_t bps = 0;
    uint64_t frames = 0;                  // pushed since the last reset
    int open_cur = 0;                     // which LagOpen holds the open row, which half of hist the history (a launch writes the other)
    bool poisoned = false;                // a push failed half way: reset clears it
    Stream own; hipStream_t last = nullptr; bool has_last = false;       // last: the stream of the previous push (not owned)
    // state: 2 x LagOpen, then the non-finite total (uint64); slab: [kEnvMaxGroups] uint32, then [kEnvMaxCells] LagCell (B > 65536);
    // hist: 2 x max_lag frames of raw bytes, frame k of a half being stream frame `frames` - max_lag + k
    DevBuf state, slab, hist, stage, rows_out;
    int max_lag() const { return lags[n_lags - 1]; }
    LagOpen *open(int i) const { return (LagOpen *)state.p + i; }
    char *history(int i) const { return (char *)hist.p + (size_t)i * hist_bytes(); }
    size_t hist_bytes() const { return ((size_t)max_lag() * bps + 15) & ~(size_t)15; }
    uint64_t *nonfinite_total() const { return (uint64_t *)((LagOpen *)state.p + 2); }
    static constexpr size_t kStateBytes = 2 * sizeof(LagOpen) + sizeof(uint64_t);
    uint32_t *slab_nonfinite() const { return (uint32_t *)slab.p; }
    LagCell *slab_cells() const { return log2_b > kEnvLog2CellFrames ? (LagCell *)((uint32_t *)slab.p + kEnvMaxGroups) : nullptr; }
    size_t slab_bytes() const { return (size_t)kEnvMaxGroups * sizeof(uint32_t) + (log2_b > kEnvLog2CellFrames ? (size_t)kEnvMaxCells * sizeof(LagCell) : 0); }
    uint64_t B() const { return (uint64_t)1 << log2_b; }
    size_t rows_of(size_t n) const { return (size_t)(((frames + n) >> log2_b) - (frames >> log2_b)); }
    IQGPU_LOCAL ~iqgpu_lag()
    {
        if (!own) return;                 // (create got no further than its checks: nothing is held)
        (void)hipSetDevice(device);
        if (has_last) (void)hipStreamSynchronize(last);
        (void)hipStreamSynchronize(own);  // the waits first: the members free themselves behind them
    }
};
static_assert(sizeof(LagOpen) % sizeof(double) == 0 && (kEnvMaxGroups * sizeof(uint32_t)) % sizeof(double) == 0, "what lies behind them stays aligned");

namespace {

constexpr size_t kPushSliceFrames = (size_t)1 << 22;     // of a host push: frames staged per slice (its rows come back per slice)
constexpr double kTwoPi = 6.283185307179586476925286766559;

// log2 of a valid block_frames, -1 otherwise
int log2_block(uint32_t b)
{
    if (b == 0 || (b & (b - 1)) != 0) return -1;
    int l = 0;
    while (((uint32_t)1 << l) != b) ++l;
    return l >= kEnvLog2BlockMin && l <= kEnvLog2BlockMax ? l : -1;
}

int check_opts(const iqgpu_lag_opts *o, const char *who)
{
    if (!o) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (log2_block(o->block_frames) < 0)
        return fail(IQGPU_EINVAL, "%s: block_frames %u is not a power of two in 2^%d .. 2^%d", who, o->block_frames, kEnvLog2BlockMin, kEnvLog2BlockMax);
    if (o->n_lags < 1 || o->n_lags > (uint32_t)kLagMaxLags) return fail(IQGPU_EINVAL, "%s: n_lags %u is outside 1 .. %d", who, o->n_lags, kLagMaxLags);
    for (uint32_t l = 0; l < o->n_lags; ++l) {
        if (o->lags[l] < 1 || o->lags[l] > (uint32_t)kLagMaxLag) return fail(IQGPU_EINVAL, "%s: lag %u is outside 1 .. %d", who, o->lags[l], kLagMaxLag);
        if (l && o->lags[l] <= o->lags[l - 1]) return fail(IQGPU_EINVAL, "%s: the lags must be strictly increasing", who);
    }
    return IQGPU_OK;
}

int zero_state(iqgpu_lag *p)
{
    HIP_TRY(hipMemsetAsync(p->state.p, 0, iqgpu_lag::kStateBytes, p->own));
    HIP_TRY(hipStreamSynchronize(p->own));
    return IQGPU_OK;
}

int guard(const iqgpu_lag *p, bool args_ok, const char *who)
{
    if (!p || !args_ok) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (p->poisoned) return fail(IQGPU_EHIP, "%s: an earlier push failed half way through: the accumulator is undefined until iqgpu_lag_reset()", who);
    return IQGPU_OK;
}

// n frames of device memory behind everything pushed so far, on s; the rows they finish into the device planes (either may be NULL)
int push_frames(iqgpu_lag *p, const void *d_raw, size_t n, float *d_lag, float *d_sum, hipStream_t s)
{
    if (p->has_last && p->last != s) HIP_TRY(hipStreamSynchronize(p->last));     // the previous push's work comes first
    p->has_last = true; p->last = s;
    const int lb = p->log2_b, lp = env_log2_page(lb);
    const uint64_t P = (uint64_t)1 << lp, L = (uint64_t)p->max_lag();
    p->poisoned = true;                                                           // (until the last launch of the push is queued)
    for (size_t at = 0; at < n;) {
        const uint64_t first = p->frames;
        const uint64_t room = ((uint64_t)1 << kEnvLog2LaunchFrames) - first % P;  // whole pages up to the launch's bound
        const uint64_t cnt = n - at < room ? n - at : room, end = first + cnt;
        const char *raw = (const char *)d_raw + at * p->bps;
        LagRowsArgs a{};
        a.raw = raw; a.hist = p->history(p->open_cur); a.first = (int64_t)first; a.n = (int64_t)cnt; a.fmt = p->format; a.log2_b = lb;
        a.n_lags = p->n_lags; a.max_lag = p->max_lag();
        for (int l = 0; l < p->n_lags; ++l) a.lags[l] = p->lags[l];
        int groups = 0;
        env_grid(a.first, a.n, lb, &groups, &a.pages_per_group);
        a.open_in = p->open(p->open_cur); a.open_out = p->open(p->open_cur ^ 1);
        a.cells = p->slab_cells(); a.row_lag = d_lag; a.row_sum = d_sum; a.nonfinite = p->slab_nonfinite();
        HIP_TRY(launch_lag_rows(a, s));
        const bool cf32 = p->format == IQGPU_FMT_CF32;
        if (cf32 || a.cells) {
            LagFoldArgs f{};
            f.nonfinite = a.nonfinite; f.n_groups = cf32 ? groups : 0; f.nonfinite_total = p->nonfinite_total();
            f.cells = a.cells; f.log2_cells_per_row = lb > kEnvLog2CellFrames ? lb - kEnvLog2CellFrames : 0; f.n_lags = p->n_lags;
            f.c0 = (int64_t)(first >> lp); f.n_closed = (int64_t)((end >> lp) - (first >> lp)); f.n_touched = (int64_t)(((end - 1) >> lp) - (first >> lp) + 1);
            f.rows_before = (int64_t)(first >> lb);
            f.open_in = a.open_in; f.open_out = a.open_out; f.row_lag = d_lag; f.row_sum = d_sum;
            HIP_TRY(launch_lag_fold(f, s));
        }
        // the history behind the launch, into the other half: the last max_lag frames of the stream.  A launch shorter than that
        // keeps the tail of the old history in front of its own frames
        char *h_old = p->history(p->open_cur), *h_new = p->history(p->open_cur ^ 1);
        if (cnt >= L) {
            HIP_TRY(hipMemcpyAsync(h_new, raw + (cnt - L) * p->bps, L * p->bps, hipMemcpyDeviceToDevice, s));
        } else {
            HIP_TRY(hipMemcpyAsync(h_new, h_old + cnt * p->bps, (L - cnt) * p->bps, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(h_new + (L - cnt) * p->bps, raw, cnt * p->bps, hipMemcpyDeviceToDevice, s));
        }
        p->open_cur ^= 1;                                                         // the open row and the history are in the other buffers
        const uint64_t done = (end >> lb) - (first >> lb);                        // rows the launch finished
        if (d_lag) d_lag += done * 2 * (uint64_t)p->n_lags;
        if (d_sum) d_sum += done;
        p->frames = end;
        at += (size_t)cnt;
    }
    p->poisoned = false;
    return IQGPU_OK;
}

// the checks of both pushes, in front of anything queued; *need = the rows the push finishes
int begin_push(iqgpu_lag *p, const void *raw, size_t frames, bool planes, size_t cap_rows, size_t *rows, size_t *need, const char *who)
{
    if (rows) *rows = 0;
    const int rc = guard(p, raw || !frames, who); if (rc) return rc;
    *need = p->rows_of(frames);
    if (planes && *need > cap_rows)
        return fail(IQGPU_ECAPACITY, "%s: room for %zu rows, the push finishes %zu (iqgpu_lag_max_rows)", who, cap_rows, *need);
    if (frames) HIP_TRY(hipSetDevice(p->device));
    return IQGPU_OK;
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
    *rows = frames >> log2_block(o->block_frames);
    return IQGPU_OK;
}

extern "C" int iqgpu_lag_create(int device, int format, const iqgpu_lag_opts *o, iqgpu_lag **out)
{
    const char *who = "iqgpu_lag_create";
    if (out) *out = nullptr;
    if (!out) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    int rc = check_opts(o, who); if (rc) return rc;
    if (!bytes_per_frame(format)) return fail(IQGPU_EFORMAT, "%s: unhandled sample format %d", who, format);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(IQGPU_ENODEV, "%s: no HIP device available", who);
    if (device < 0 || device >= ndev) return fail(IQGPU_ENODEV, "%s: device %d out of range (%d devices)", who, device, ndev);
    iqgpu_lag *p = new (std::nothrow) iqgpu_lag;
    if (!p) return fail(IQGPU_ENOMEM, "%s: out of host memory", who);
    p->device = device; p->format = format; p->bps = bytes_per_frame(format); p->log2_b = log2_block(o->block_frames);
    p->n_lags = (int)o->n_lags;
    for (int l = 0; l < p->n_lags; ++l) p->lags[l] = (int32_t)o->lags[l];
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = p->own.create();
    if (e != hipSuccess) rc = fail(IQGPU_EHIP, "%s: %s", who, hipGetErrorString(e));
    if (rc == IQGPU_OK) rc = p->state.ensure(iqgpu_lag::kStateBytes);
    if (rc == IQGPU_OK) rc = p->slab.ensure(p->slab_bytes());
    if (rc == IQGPU_OK) rc = p->hist.ensure(2 * p->hist_bytes());
    if (rc == IQGPU_OK) rc = zero_state(p);
    if (rc != IQGPU_OK) { delete p; return rc; }
    *out = p;
    return IQGPU_OK;
}

extern "C" void iqgpu_lag_destroy(iqgpu_lag *p) { delete p; }

extern "C" int iqgpu_lag_reset(iqgpu_lag *p)
{
    if (!p) return fail(IQGPU_EINVAL, "iqgpu_lag_reset: NULL argument");
    HIP_TRY(hipSetDevice(p->device));
    if (p->has_last) (void)hipStreamSynchronize(p->last);            // (a failed push may have left an error there: ignored)
    const int rc = zero_state(p); if (rc) return rc;
    // (frames = 0 empties the history: a frame in front of the stream's first is never a partner)
    p->frames = 0; p->open_cur = 0; p->has_last = false; p->last = nullptr; p->poisoned = false;
    return IQGPU_OK;
}

extern "C" size_t iqgpu_lag_max_rows(const iqgpu_lag *p, size_t frames) { return p ? p->rows_of(frames) : 0; }

extern "C" int iqgpu_lag_push_device(iqgpu_lag *p, const void *d_raw, size_t frames, float *d_row_lag, float *d_row_sum, size_t cap_rows,
                                     size_t *rows, void *hip_stream)
{
    size_t need = 0;
    const int rc = begin_push(p, d_raw, frames, d_row_lag || d_row_sum, cap_rows, rows, &need, "iqgpu_lag_push_device"); if (rc) return rc;
    if (frames == 0) return IQGPU_OK;
    if (rows) *rows = need;
    return push_frames(p, d_raw, frames, d_row_lag, d_row_sum, (hipStream_t)hip_stream);
}

extern "C" int iqgpu_lag_push(iqgpu_lag *p, const void *raw, size_t frames, float *row_lag, float *row_sum, size_t cap_rows, size_t *rows)
{
    size_t need = 0;
    int rc = begin_push(p, raw, frames, row_lag || row_sum, cap_rows, rows, &need, "iqgpu_lag_push"); if (rc) return rc;
    if (frames == 0) return IQGPU_OK;
    const size_t slice = frames < kPushSliceFrames ? frames : kPushSliceFrames;
    const size_t slice_rows = (slice >> p->log2_b) + 1;              // rows of one slice, whatever the position
    const size_t per_row = 2 * (size_t)p->n_lags;
    rc = p->stage.ensure(slice * p->bps); if (rc) return rc;
    rc = p->rows_out.ensure((per_row + 1) * slice_rows * sizeof(float)); if (rc) return rc;
    float *d_lag = row_lag ? (float *)p->rows_out.p : nullptr, *d_sum = row_sum ? (float *)p->rows_out.p + per_row * slice_rows : nullptr;
    if (rows) *rows = need;
    for (size_t at = 0; at < frames;) {
        const size_t n = frames - at < kPushSliceFrames ? frames - at : kPushSliceFrames;
        const size_t done = p->rows_of(n);
        if (done > slice_rows) return fail(IQGPU_EHIP, "iqgpu_lag_push: a slice finishes %zu rows, the buffer holds %zu", done, slice_rows);
        HIP_TRY(hipMemcpyAsync(p->stage.p, (const char *)raw + at * p->bps, n * p->bps, hipMemcpyHostToDevice, p->own));
        rc = push_frames(p, p->stage.p, n, d_lag, d_sum, p->own); if (rc) return rc;
        p->poisoned = true;                                              // (until the slice's rows are in the caller's memory)
        if (row_lag && done) HIP_TRY(hipMemcpyAsync(row_lag, d_lag, done * per_row * sizeof(float), hipMemcpyDeviceToHost, p->own));
        if (row_sum && done) HIP_TRY(hipMemcpyAsync(row_sum, d_sum, done * sizeof(float), hipMemcpyDeviceToHost, p->own));
        HIP_TRY(hipStreamSynchronize(p->own));                          // the one staging pair: the next slice overwrites both
        p->poisoned = false;
        if (row_lag) row_lag += done * per_row;
        if (row_sum) row_sum += done;
        at += n;
    }
    return IQGPU_OK;
}

extern "C" int iqgpu_lag_read_open(iqgpu_lag *p, double *lag, double *sum, iqgpu_lag_info *info)
{
    const int rc = guard(p, true, "iqgpu_lag_read_open"); if (rc) return rc;
    HIP_TRY(hipSetDevice(p->device));
    if (p->has_last) HIP_TRY(hipStreamSynchronize(p->last));
    p->has_last = false; p->last = nullptr;
    const uint64_t B = p->B(), P = (uint64_t)1 << env_log2_page(p->log2_b);
    const uint64_t open_frames = p->frames % B;
    const int nc = 2 * p->n_lags + 1;
    if (lag || sum) {
        // the open row's closed cells are in the total, its open page beside it; what the arithmetic says is empty is not looked at
        const bool has_tot = open_frames >= (uint64_t)kStatsPageFrames, has_page = p->frames % P != 0 && open_frames != 0;
        double v[kLagComps] = {0.0};
        if (has_tot || has_page) {
            const std::unique_ptr<LagOpen> rec(new (std::nothrow) LagOpen);
            if (!rec) return fail(IQGPU_ENOMEM, "iqgpu_lag_read_open: out of host memory");
            LagOpen &o = *rec;
            const LagOpen *d = p->open(p->open_cur);
            if (has_page) HIP_TRY(hipMemcpy(&o, d, sizeof(o), hipMemcpyDeviceToHost));
            else HIP_TRY(hipMemcpy(&o.tot, &d->tot, sizeof(o.tot), hipMemcpyDeviceToHost));       // the total alone
            // B < 1024: the open row's terms are columns [at, at + open_frames) of the step; the tree over B terms is the tree over
            // 1024 columns whose others are +0.0
            const size_t at = B < (uint64_t)kStatsColumns ? (size_t)((p->frames - open_frames) % kStatsColumns) : 0;
            const size_t cnt = B < (uint64_t)kStatsColumns ? (size_t)open_frames : (size_t)kStatsColumns;
            for (int c = 0; c < nc; ++c) {
                if (has_tot) v[c] = o.tot[c];
                if (has_page) {
                    double col[kStatsColumns] = {0.0};
                    for (size_t i = 0; i < cnt; ++i) col[i] = o.col[c][at + i];
                    v[c] = v[c] + stats_tree(col);
                }
            }
        }
        if (sum) *sum = v[0];
        if (lag) for (int c = 1; c < nc; ++c) lag[c - 1] = v[c];
    }
    if (info) {
        uint64_t nonfinite = 0;
        if (p->format == IQGPU_FMT_CF32) HIP_TRY(hipMemcpy(&nonfinite, p->nonfinite_total(), sizeof(nonfinite), hipMemcpyDeviceToHost));
        memset(info, 0, sizeof(*info));
        info->frames = p->frames; info->rows = p->frames >> p->log2_b; info->nonfinite_frames = nonfinite;
        info->open_frames = (uint32_t)open_frames; info->block_frames = (uint32_t)B; info->n_lags = (uint32_t)p->n_lags;
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
