// env.cpp -- host side of the envelope accumulator (include/iqgpu.h "envelope"; kernels env.hip): the options, the
// iqgpu_env handle -- the row-page core (row_pages.hpp) with EnvOpen records and EnvCell cells -- what a launch's arguments are, how
// the open row is assembled, push / push_device / read_open / reset under iqgpu_sgram's rules, and the two host-only calls on
// finished rows: the burst finder and the floor.  Independent of any chain.
#include <algorithm>
#include <cstddef>
#include <memory>

#include "chain.hpp"
#include "env.hpp"
#include "row_pages.hpp"

struct iqgpu_env {
    RowPages rp;
    EnvOpen *open(int i) const { return (EnvOpen *)rp.open_rec(i); }
    IQGPU_LOCAL ~iqgpu_env() { rp.close(); }          // the waits first: the members free themselves behind them
};
static_assert(sizeof(EnvOpen) % sizeof(double) == 0 && (kEnvMaxGroups * sizeof(uint32_t)) % sizeof(double) == 0, "what lies behind them stays aligned");

namespace {

constexpr size_t kPushSliceFrames = (size_t)1 << 22;     // of a host push: frames staged per slice (its rows come back per slice)
const char *const kReset = "iqgpu_env_reset";
const char *const kMaxRows = "iqgpu_env_max_rows";

RowPages *core(iqgpu_env *p) { return p ? &p->rp : nullptr; }

int check_opts(const iqgpu_env_opts *o, const char *who)
{
    if (!o) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    return RowPages::check_block(o->block_frames, who);
}

// n frames of device memory behind everything pushed so far, on s; the rows they finish into the device planes (any may be NULL)
int push_frames(iqgpu_env *p, const void *d_raw, size_t n, float *d_sum, float *d_pk, uint32_t *d_rail, hipStream_t s)
{
    RowPages &rp = p->rp;
    return rp.push(d_raw, n, s, [&](const RowLaunch &u) {
        EnvRowsArgs a{};
        a.raw = u.raw; a.first = (int64_t)u.first; a.n = (int64_t)u.cnt; a.fmt = rp.format; a.log2_b = rp.log2_b; a.pages_per_group = u.pages_per_group;
        a.open_in = p->open(rp.open_cur); a.open_out = p->open(rp.open_cur ^ 1);
        a.cells = (EnvCell *)rp.slab_cells(); a.row_sum = d_sum; a.row_peak = d_pk; a.row_rail = d_rail; a.nonfinite = rp.slab_nonfinite();
        HIP_TRY(launch_env_rows(a, s));
        if (u.cf32 || a.cells) {
            EnvFoldArgs f{};
            rp.fill_fold(u, &f);
            f.cells = a.cells; f.open_in = a.open_in; f.open_out = a.open_out; f.row_sum = d_sum; f.row_peak = d_pk; f.row_rail = d_rail;
            HIP_TRY(launch_env_fold(f, s));
        }
        if (d_sum) d_sum += u.done;
        if (d_pk) d_pk += u.done;
        if (d_rail) d_rail += u.done;
        return (int)IQGPU_OK;
    });
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
    *rows = frames >> RowPages::log2_block(o->block_frames);
    return IQGPU_OK;
}

extern "C" int iqgpu_env_create(int device, int format, const iqgpu_env_opts *o, iqgpu_env **out)
{
    const char *who = "iqgpu_env_create";
    if (out) *out = nullptr;
    if (!out) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    int rc = check_opts(o, who); if (rc) return rc;
    iqgpu_env *p = new (std::nothrow) iqgpu_env;
    rc = RowPages::open(core(p), device, format, o->block_frames, sizeof(EnvOpen), sizeof(EnvCell), who);
    if (rc == IQGPU_OK) rc = p->rp.zero_state();
    if (rc != IQGPU_OK) { delete p; return rc; }
    *out = p;
    return IQGPU_OK;
}

extern "C" void iqgpu_env_destroy(iqgpu_env *p) { delete p; }

extern "C" int iqgpu_env_reset(iqgpu_env *p) { return RowPages::reset(core(p), "iqgpu_env_reset"); }

extern "C" size_t iqgpu_env_max_rows(const iqgpu_env *p, size_t frames) { return p ? p->rp.rows_of(frames) : 0; }

extern "C" int iqgpu_env_push_device(iqgpu_env *p, const void *d_raw, size_t frames, float *d_row_sum, float *d_row_peak, uint32_t *d_row_rail,
                                     size_t cap_rows, size_t *rows, void *hip_stream)
{
    size_t need = 0;
    const int rc = RowPages::begin_push(core(p), d_raw, frames, d_row_sum || d_row_peak || d_row_rail, cap_rows, rows, &need, "iqgpu_env_push_device", kReset, kMaxRows);
    if (rc) return rc;
    if (frames == 0) return IQGPU_OK;
    if (rows) *rows = need;
    return push_frames(p, d_raw, frames, d_row_sum, d_row_peak, d_row_rail, (hipStream_t)hip_stream);
}

extern "C" int iqgpu_env_push(iqgpu_env *p, const void *raw, size_t frames, float *row_sum, float *row_peak, uint32_t *row_rail, size_t cap_rows,
                              size_t *rows)
{
    const char *who = "iqgpu_env_push";
    size_t need = 0;
    int rc = RowPages::begin_push(core(p), raw, frames, row_sum || row_peak || row_rail, cap_rows, rows, &need, who, kReset, kMaxRows); if (rc) return rc;
    if (frames == 0) return IQGPU_OK;
    RowPages &rp = p->rp;
    const size_t slice = frames < kPushSliceFrames ? frames : kPushSliceFrames;
    const size_t slice_rows = (slice >> rp.log2_b) + 1;              // rows of one slice, whatever the position
    rc = rp.stage.ensure(slice * rp.bps); if (rc) return rc;
    rc = rp.rows_out.ensure(3 * slice_rows * sizeof(float)); if (rc) return rc;
    float *d_sum = row_sum ? (float *)rp.rows_out.p : nullptr, *d_pk = row_peak ? (float *)rp.rows_out.p + slice_rows : nullptr;
    uint32_t *d_rail = row_rail ? (uint32_t *)rp.rows_out.p + 2 * slice_rows : nullptr;
    if (rows) *rows = need;
    HostPlane planes[3] = {{(char *)row_sum, d_sum, sizeof(float)}, {(char *)row_peak, d_pk, sizeof(float)}, {(char *)row_rail, d_rail, sizeof(uint32_t)}};
    return push_host_slices(rp, rp.stage, raw, frames, kPushSliceFrames, slice_rows, planes, who, "finishes",
                            [&](size_t n) { return rp.rows_of(n); },
                            [&](const void *d_raw, size_t n) { return push_frames(p, d_raw, n, d_sum, d_pk, d_rail, rp.own); });
}

extern "C" int iqgpu_env_read_open(iqgpu_env *p, double *sum, double *peak, uint32_t *rail, iqgpu_env_info *info)
{
    int rc = RowPages::guard(core(p), true, "iqgpu_env_read_open", kReset); if (rc) return rc;
    RowPages &rp = p->rp;
    rc = rp.settle(); if (rc) return rc;
    const OpenRow r = rp.open_row();
    if (sum || peak || rail) {
        double s = 0.0, k = 0.0; uint32_t n = 0;
        if (r.has_tot || r.has_page) {
            const std::unique_ptr<EnvOpen> rec(new (std::nothrow) EnvOpen);
            if (!rec) return fail(IQGPU_ENOMEM, "iqgpu_env_read_open: out of host memory");
            EnvOpen &o = *rec;
            rc = rp.fetch_open(r, &o, offsetof(EnvOpen, tot_sum)); if (rc) return rc;
            if (r.has_tot) { s = o.tot_sum; k = o.tot_peak; n = o.tot_rail; }
            if (r.has_page) {
                for (size_t i = 0; i < r.cnt; ++i) {
                    k = o.col_peak[r.at + i] > k ? o.col_peak[r.at + i] : k;
                    n += o.col_rail[r.at + i];
                }
                s = s + RowPages::open_tree(r, o.col_sum);
            }
        }
        if (sum) *sum = s;
        if (peak) *peak = k;
        if (rail) *rail = n;
    }
    if (info) {
        uint64_t nonfinite = 0;
        if (rp.format == IQGPU_FMT_CF32) HIP_TRY(hipMemcpy(&nonfinite, rp.nonfinite_total(), sizeof(nonfinite), hipMemcpyDeviceToHost));
        memset(info, 0, sizeof(*info));
        info->frames = rp.frames; info->rows = rp.frames >> rp.log2_b; info->nonfinite_frames = nonfinite;
        info->open_frames = (uint32_t)r.open_frames; info->block_frames = (uint32_t)rp.B();
    }
    return IQGPU_OK;
}

// ---- host only ----
extern "C" int iqgpu_env_bursts(const float *row_sum, size_t rows, const iqgpu_env_burst_opts *o, iqgpu_env_burst *out, size_t cap, size_t *n)
{
    const char *who = "iqgpu_env_bursts";
    if (n) *n = 0;
    if (!o || !n || (!row_sum && rows) || (!out && cap)) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (RowPages::log2_block(o->block_frames) < 0) return fail(IQGPU_EINVAL, "%s: block_frames %u is not a power of two in 2^6 .. 2^24", who, o->block_frames);
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
    if (RowPages::log2_block(block_frames) < 0) return fail(IQGPU_EINVAL, "%s: block_frames %u is not a power of two in 2^6 .. 2^24", who, block_frames);
    if (rows == 0 || !(fraction >= 0.0 && fraction <= 1.0)) return fail(IQGPU_EINVAL, "%s: no rows, or a fraction outside [0, 1]", who);
    std::vector<float> v;
    try { v.assign(row_sum, row_sum + rows); } catch (const std::bad_alloc &) { return fail(IQGPU_ENOMEM, "%s: out of host memory", who); }
    const size_t k = (size_t)std::floor(fraction * (double)(rows - 1));
    // ascending, a NaN behind every number
    std::nth_element(v.begin(), v.begin() + (std::ptrdiff_t)k, v.end(), [](float a, float b) { return b != b ? a == a : a < b; });
    *mean_power = mean_of(v[k], block_frames);
    return IQGPU_OK;
}
