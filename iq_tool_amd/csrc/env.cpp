// env.cpp -- host side of the envelope accumulator (include/iqgpu.h "envelope"; kernels env.hip): the options and the row
// arithmetic (no device), the iqgpu_env handle -- stream position, the open row in two buffers, the slab of a launch -- with push /
// push_device / read_open / reset under iqgpu_sgram's rules, and the two host-only calls on finished rows: the burst finder and the
// floor.  Independent of any chain.
#include <algorithm>
#include <cstddef>
#include <memory>

#include "chain.hpp"
#include "env.hpp"

struct iqgpu_env {
    int device = 0, format = 0, log2_b = 0;
    size_t bps = 0;
    uint64_t frames = 0;                  // pushed since the last reset
    int open_cur = 0;                     // which EnvOpen holds the open row (a launch writes the other)
    bool poisoned = false;                // a push failed half way: reset clears it
    Stream own; hipStream_t last = nullptr; bool has_last = false;       // last: the stream of the previous push (not owned)
    // state: 2 x EnvOpen, then the non-finite total (uint64); slab: [kEnvMaxGroups] uint32, then [kEnvMaxCells] EnvCell (B > 65536)
    DevBuf state, slab, stage, rows_out;
    EnvOpen *open(int i) const { return (EnvOpen *)state.p + i; }
    uint64_t *nonfinite_total() const { return (uint64_t *)((EnvOpen *)state.p + 2); }
    static constexpr size_t kStateBytes = 2 * sizeof(EnvOpen) + sizeof(uint64_t);
    uint32_t *slab_nonfinite() const { return (uint32_t *)slab.p; }
    EnvCell *slab_cells() const { return log2_b > kEnvLog2CellFrames ? (EnvCell *)((uint32_t *)slab.p + kEnvMaxGroups) : nullptr; }
    size_t slab_bytes() const { return (size_t)kEnvMaxGroups * sizeof(uint32_t) + (log2_b > kEnvLog2CellFrames ? (size_t)kEnvMaxCells * sizeof(EnvCell) : 0); }
    uint64_t B() const { return (uint64_t)1 << log2_b; }
    size_t rows_of(size_t n) const { return (size_t)(((frames + n) >> log2_b) - (frames >> log2_b)); }
    IQGPU_LOCAL ~iqgpu_env()
    {
        if (!own) return;                 // (create got no further than its checks: nothing is held)
        (void)hipSetDevice(device);
        if (has_last) (void)hipStreamSynchronize(last);
        (void)hipStreamSynchronize(own);  // the waits first: the members free themselves behind them
    }
};
static_assert(sizeof(EnvOpen) % sizeof(double) == 0 && (kEnvMaxGroups * sizeof(uint32_t)) % sizeof(double) == 0, "what lies behind them stays aligned");

namespace {

constexpr size_t kPushSliceFrames = (size_t)1 << 22;     // of a host push: frames staged per slice (its rows come back per slice)

// log2 of a valid block_frames, -1 otherwise
int log2_block(uint32_t b)
{
    if (b == 0 || (b & (b - 1)) != 0) return -1;
    int l = 0;
    while (((uint32_t)1 << l) != b) ++l;
    return l >= kEnvLog2BlockMin && l <= kEnvLog2BlockMax ? l : -1;
}

int check_opts(const iqgpu_env_opts *o, const char *who)
{
    if (!o) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (log2_block(o->block_frames) < 0)
        return fail(IQGPU_EINVAL, "%s: block_frames %u is not a power of two in 2^%d .. 2^%d", who, o->block_frames, kEnvLog2BlockMin, kEnvLog2BlockMax);
    return IQGPU_OK;
}

int zero_state(iqgpu_env *p)
{
    HIP_TRY(hipMemsetAsync(p->state.p, 0, iqgpu_env::kStateBytes, p->own));
    HIP_TRY(hipStreamSynchronize(p->own));
    return IQGPU_OK;
}

int guard(const iqgpu_env *p, bool args_ok, const char *who)
{
    if (!p || !args_ok) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (p->poisoned) return fail(IQGPU_EHIP, "%s: an earlier push failed half way through: the accumulator is undefined until iqgpu_env_reset()", who);
    return IQGPU_OK;
}

// n frames of device memory behind everything pushed so far, on s; the rows they finish into the device planes (any may be NULL)
int push_frames(iqgpu_env *p, const void *d_raw, size_t n, float *d_sum, float *d_pk, uint32_t *d_rail, hipStream_t s)
{
    if (p->has_last && p->last != s) HIP_TRY(hipStreamSynchronize(p->last));     // the previous push's work comes first
    p->has_last = true; p->last = s;
    const int lb = p->log2_b, lp = env_log2_page(lb);
    const uint64_t P = (uint64_t)1 << lp;
    p->poisoned = true;                                                           // (until the last launch of the push is queued)
    for (size_t at = 0; at < n;) {
        const uint64_t first = p->frames;
        const uint64_t room = ((uint64_t)1 << kEnvLog2LaunchFrames) - first % P;  // whole pages up to the launch's bound
        const uint64_t cnt = n - at < room ? n - at : room, end = first + cnt;
        EnvRowsArgs a{};
        a.raw = (const char *)d_raw + at * p->bps; a.first = (int64_t)first; a.n = (int64_t)cnt; a.fmt = p->format; a.log2_b = lb;
        int groups = 0;
        env_grid(a.first, a.n, lb, &groups, &a.pages_per_group);
        a.open_in = p->open(p->open_cur); a.open_out = p->open(p->open_cur ^ 1);
        a.cells = p->slab_cells(); a.row_sum = d_sum; a.row_peak = d_pk; a.row_rail = d_rail; a.nonfinite = p->slab_nonfinite();
        HIP_TRY(launch_env_rows(a, s));
        const bool cf32 = p->format == IQGPU_FMT_CF32;
        if (cf32 || a.cells) {
            EnvFoldArgs f{};
            f.nonfinite = a.nonfinite; f.n_groups = cf32 ? groups : 0; f.nonfinite_total = p->nonfinite_total();
            f.cells = a.cells; f.log2_cells_per_row = lb > kEnvLog2CellFrames ? lb - kEnvLog2CellFrames : 0;
            f.c0 = (int64_t)(first >> lp); f.n_closed = (int64_t)((end >> lp) - (first >> lp)); f.n_touched = (int64_t)(((end - 1) >> lp) - (first >> lp) + 1);
            f.rows_before = (int64_t)(first >> lb);
            f.open_in = a.open_in; f.open_out = a.open_out; f.row_sum = d_sum; f.row_peak = d_pk; f.row_rail = d_rail;
            HIP_TRY(launch_env_fold(f, s));
        }
        p->open_cur ^= 1;                                                         // the open row, if the launch left one, is in the other buffer
        const uint64_t done = (end >> lb) - (first >> lb);                        // rows the launch finished
        if (d_sum) d_sum += done;
        if (d_pk) d_pk += done;
        if (d_rail) d_rail += done;
        p->frames = end;
        at += (size_t)cnt;
    }
    p->poisoned = false;
    return IQGPU_OK;
}

// the checks of both pushes, in front of anything queued; *need = the rows the push finishes
int begin_push(iqgpu_env *p, const void *raw, size_t frames, bool planes, size_t cap_rows, size_t *rows, size_t *need, const char *who)
{
    if (rows) *rows = 0;
    const int rc = guard(p, raw || !frames, who); if (rc) return rc;
    *need = p->rows_of(frames);
    if (planes && *need > cap_rows)
        return fail(IQGPU_ECAPACITY, "%s: room for %zu rows, the push finishes %zu (iqgpu_env_max_rows)", who, cap_rows, *need);
    if (frames) HIP_TRY(hipSetDevice(p->device));
    return IQGPU_OK;
}

double mean_of(float row_sum, uint32_t block_frames) { return (double)row_sum / (double)block_frames; }

} // namespace

extern "C" void iqgpu_env_opts_init(iqgpu_env_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->block_frames = (uint32_t)1 << kEnvLog2BlockDefault;
}

extern "C" int iqgpu_env_rows(const iqgpu_env_opts *o, uint64_t frames, uint64_t *rows)
{
    const int rc = check_opts(o, "iqgpu_env_rows"); if (rc) return rc;
    if (!rows) return fail(IQGPU_EINVAL, "iqgpu_env_rows: NULL argument");
    *rows = frames >> log2_block(o->block_frames);
    return IQGPU_OK;
}

extern "C" int iqgpu_env_create(int device, int format, const iqgpu_env_opts *o, iqgpu_env **out)
{
    const char *who = "iqgpu_env_create";
    if (out) *out = nullptr;
    if (!out) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    int rc = check_opts(o, who); if (rc) return rc;
    if (!bytes_per_frame(format)) return fail(IQGPU_EFORMAT, "%s: unhandled sample format %d", who, format);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(IQGPU_ENODEV, "%s: no HIP device available", who);
    if (device < 0 || device >= ndev) return fail(IQGPU_ENODEV, "%s: device %d out of range (%d devices)", who, device, ndev);
    iqgpu_env *p = new (std::nothrow) iqgpu_env;
    if (!p) return fail(IQGPU_ENOMEM, "%s: out of host memory", who);
    p->device = device; p->format = format; p->bps = bytes_per_frame(format); p->log2_b = log2_block(o->block_frames);
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = p->own.create();
    if (e != hipSuccess) rc = fail(IQGPU_EHIP, "%s: %s", who, hipGetErrorString(e));
    if (rc == IQGPU_OK) rc = p->state.ensure(iqgpu_env::kStateBytes);
    if (rc == IQGPU_OK) rc = p->slab.ensure(p->slab_bytes());
    if (rc == IQGPU_OK) rc = zero_state(p);
    if (rc != IQGPU_OK) { delete p; return rc; }
    *out = p;
    return IQGPU_OK;
}

extern "C" void iqgpu_env_destroy(iqgpu_env *p) { delete p; }

extern "C" int iqgpu_env_reset(iqgpu_env *p)
{
    if (!p) return fail(IQGPU_EINVAL, "iqgpu_env_reset: NULL argument");
    HIP_TRY(hipSetDevice(p->device));
    if (p->has_last) (void)hipStreamSynchronize(p->last);            // (a failed push may have left an error there: ignored)
    const int rc = zero_state(p); if (rc) return rc;
    p->frames = 0; p->open_cur = 0; p->has_last = false; p->last = nullptr; p->poisoned = false;
    return IQGPU_OK;
}

extern "C" size_t iqgpu_env_max_rows(const iqgpu_env *p, size_t frames) { return p ? p->rows_of(frames) : 0; }

extern "C" int iqgpu_env_push_device(iqgpu_env *p, const void *d_raw, size_t frames, float *d_row_sum, float *d_row_peak, uint32_t *d_row_rail,
                                     size_t cap_rows, size_t *rows, void *hip_stream)
{
    size_t need = 0;
    const int rc = begin_push(p, d_raw, frames, d_row_sum || d_row_peak || d_row_rail, cap_rows, rows, &need, "iqgpu_env_push_device"); if (rc) return rc;
    if (frames == 0) return IQGPU_OK;
    if (rows) *rows = need;
    return push_frames(p, d_raw, frames, d_row_sum, d_row_peak, d_row_rail, (hipStream_t)hip_stream);
}

extern "C" int iqgpu_env_push(iqgpu_env *p, const void *raw, size_t frames, float *row_sum, float *row_peak, uint32_t *row_rail, size_t cap_rows,
                              size_t *rows)
{
    size_t need = 0;
    int rc = begin_push(p, raw, frames, row_sum || row_peak || row_rail, cap_rows, rows, &need, "iqgpu_env_push"); if (rc) return rc;
    if (frames == 0) return IQGPU_OK;
    const size_t slice = frames < kPushSliceFrames ? frames : kPushSliceFrames;
    const size_t slice_rows = (slice >> p->log2_b) + 1;              // rows of one slice, whatever the position
    rc = p->stage.ensure(slice * p->bps); if (rc) return rc;
    rc = p->rows_out.ensure(3 * slice_rows * sizeof(float)); if (rc) return rc;
    float *d_sum = row_sum ? (float *)p->rows_out.p : nullptr, *d_pk = row_peak ? (float *)p->rows_out.p + slice_rows : nullptr;
    uint32_t *d_rail = row_rail ? (uint32_t *)p->rows_out.p + 2 * slice_rows : nullptr;
    if (rows) *rows = need;
    for (size_t at = 0; at < frames;) {
        const size_t n = frames - at < kPushSliceFrames ? frames - at : kPushSliceFrames;
        const size_t done = p->rows_of(n);
        if (done > slice_rows) return fail(IQGPU_EHIP, "iqgpu_env_push: a slice finishes %zu rows, the buffer holds %zu", done, slice_rows);
        HIP_TRY(hipMemcpyAsync(p->stage.p, (const char *)raw + at * p->bps, n * p->bps, hipMemcpyHostToDevice, p->own));
        rc = push_frames(p, p->stage.p, n, d_sum, d_pk, d_rail, p->own); if (rc) return rc;
        p->poisoned = true;                                              // (until the slice's rows are in the caller's memory)
        if (row_sum && done) HIP_TRY(hipMemcpyAsync(row_sum, d_sum, done * sizeof(float), hipMemcpyDeviceToHost, p->own));
        if (row_peak && done) HIP_TRY(hipMemcpyAsync(row_peak, d_pk, done * sizeof(float), hipMemcpyDeviceToHost, p->own));
        if (row_rail && done) HIP_TRY(hipMemcpyAsync(row_rail, d_rail, done * sizeof(uint32_t), hipMemcpyDeviceToHost, p->own));
        HIP_TRY(hipStreamSynchronize(p->own));                          // the one staging pair: the next slice overwrites both
        p->poisoned = false;
        if (row_sum) row_sum += done;
        if (row_peak) row_peak += done;
        if (row_rail) row_rail += done;
        at += n;
    }
    return IQGPU_OK;
}

extern "C" int iqgpu_env_read_open(iqgpu_env *p, double *sum, double *peak, uint32_t *rail, iqgpu_env_info *info)
{
    const int rc = guard(p, true, "iqgpu_env_read_open"); if (rc) return rc;
    HIP_TRY(hipSetDevice(p->device));
    if (p->has_last) HIP_TRY(hipStreamSynchronize(p->last));
    p->has_last = false; p->last = nullptr;
    const uint64_t B = p->B(), P = (uint64_t)1 << env_log2_page(p->log2_b);
    const uint64_t open_frames = p->frames % B;
    if (sum || peak || rail) {
        // the open row's closed cells are in the total, its open page beside it; what the arithmetic says is empty is not looked at
        const bool has_tot = open_frames >= (uint64_t)kStatsPageFrames, has_page = p->frames % P != 0 && open_frames != 0;
        double s = 0.0, k = 0.0; uint32_t r = 0;
        if (has_tot || has_page) {
            const std::unique_ptr<EnvOpen> rec(new (std::nothrow) EnvOpen);
            if (!rec) return fail(IQGPU_ENOMEM, "iqgpu_env_read_open: out of host memory");
            EnvOpen &o = *rec;
            const EnvOpen *d = p->open(p->open_cur);
            if (has_page) HIP_TRY(hipMemcpy(&o, d, sizeof(o), hipMemcpyDeviceToHost));
            else HIP_TRY(hipMemcpy(&o.tot_sum, &d->tot_sum, sizeof(o) - offsetof(EnvOpen, tot_sum), hipMemcpyDeviceToHost));    // the total alone
            if (has_tot) { s = o.tot_sum; k = o.tot_peak; r = o.tot_rail; }
            if (has_page) {
                // B < 1024: the open row's terms are columns [at, at + open_frames) of the step; the tree over B terms is the tree
                // over 1024 columns whose others are +0.0
                const size_t at = B < (uint64_t)kStatsColumns ? (size_t)((p->frames - open_frames) % kStatsColumns) : 0;
                const size_t cnt = B < (uint64_t)kStatsColumns ? (size_t)open_frames : (size_t)kStatsColumns;
                double col[kStatsColumns] = {0.0};
                for (size_t i = 0; i < cnt; ++i) {
                    col[i] = o.col_sum[at + i];
                    k = o.col_peak[at + i] > k ? o.col_peak[at + i] : k;
                    r += o.col_rail[at + i];
                }
                s = s + stats_tree(col);
            }
        }
        if (sum) *sum = s;
        if (peak) *peak = k;
        if (rail) *rail = r;
    }
    if (info) {
        uint64_t nonfinite = 0;
        if (p->format == IQGPU_FMT_CF32) HIP_TRY(hipMemcpy(&nonfinite, p->nonfinite_total(), sizeof(nonfinite), hipMemcpyDeviceToHost));
        memset(info, 0, sizeof(*info));
        info->frames = p->frames; info->rows = p->frames >> p->log2_b; info->nonfinite_frames = nonfinite;
        info->open_frames = (uint32_t)open_frames; info->block_frames = (uint32_t)B;
    }
    return IQGPU_OK;
}

// ---- host only ----
extern "C" int iqgpu_env_bursts(const float *row_sum, size_t rows, const iqgpu_env_burst_opts *o, iqgpu_env_burst *out, size_t cap, size_t *n)
{
    const char *who = "iqgpu_env_bursts";
    if (n) *n = 0;
    if (!o || !n || (!row_sum && rows) || (!out && cap)) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (log2_block(o->block_frames) < 0) return fail(IQGPU_EINVAL, "%s: block_frames %u is not a power of two in 2^6 .. 2^24", who, o->block_frames);
    if (!(o->off <= o->on)) return fail(IQGPU_EINVAL, "%s: the thresholds must be numbers with off <= on", who);
    const uint64_t B = o->block_frames, pad = o->pad_rows;
    size_t count = 0;
    uint64_t cur_a = 0, cur_b = 0;        // the burst being joined, rows [cur_a, cur_b), padded; empty when cur_b == 0
    // one finished burst [a, b) of rows, padded already, into the output: its peak is the first largest mean of its rows
    auto emit = [&](uint64_t a, uint64_t b) {
        if (count < cap) {
            uint64_t pr = a; double pm = mean_of(row_sum[a], o->block_frames);
            for (uint64_t r = a; r < b; ++r) {
                const double m = mean_of(row_sum[r], o->block_frames);
                if (m > pm || (pm != pm && m == m)) { pm = m; pr = r; }
            }
            out[count] = iqgpu_env_burst{a * B, (b - a) * B, pr, pm};
        }
        ++count;
    };
    for (uint64_t i = 0; i < rows;) {
        if (!(mean_of(row_sum[i], o->block_frames) >= o->on)) { ++i; continue; }
        // open at i; close in front of the first run of more than hang_rows rows below `off` (a NaN mean is below), else at the end
        uint64_t e = rows, run = 0;
        for (uint64_t j = i + 1; j < rows; ++j) {
            if (mean_of(row_sum[j], o->block_frames) >= o->off) { run = 0; continue; }
            if (++run > o->hang_rows) { e = j + 1 - run; break; }
        }
        if (e - i >= o->min_rows) {
            const uint64_t a = i > pad ? i - pad : 0, b = e + pad < rows ? e + pad : rows;
            if (cur_b != 0 && a <= cur_b) cur_b = b;                  // touches or overlaps the one in front: joined
            else { if (cur_b != 0) emit(cur_a, cur_b); cur_a = a; cur_b = b; }
        }
        i = e;
    }
    if (cur_b != 0) emit(cur_a, cur_b);
    *n = count;
    if (count > cap) return fail(IQGPU_ECAPACITY, "%s: room for %zu bursts, the rows hold %zu", who, cap, count);
    return IQGPU_OK;
}

extern "C" int iqgpu_env_floor(const float *row_sum, size_t rows, uint32_t block_frames, double fraction, double *mean_power)
{
    const char *who = "iqgpu_env_floor";
    if (!row_sum || !mean_power) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (log2_block(block_frames) < 0) return fail(IQGPU_EINVAL, "%s: block_frames %u is not a power of two in 2^6 .. 2^24", who, block_frames);
    if (rows == 0 || !(fraction >= 0.0 && fraction <= 1.0)) return fail(IQGPU_EINVAL, "%s: no rows, or a fraction outside [0, 1]", who);
    std::vector<float> v;
    try { v.assign(row_sum, row_sum + rows); } catch (const std::bad_alloc &) { return fail(IQGPU_ENOMEM, "%s: out of host memory", who); }
    const size_t k = (size_t)std::floor(fraction * (double)(rows - 1));
    // ascending, a NaN behind every number
    std::nth_element(v.begin(), v.begin() + (std::ptrdiff_t)k, v.end(), [](float a, float b) { return b != b ? a == a : a < b; });
    *mean_power = mean_of(v[k], block_frames);
    return IQGPU_OK;
}
