// sgram.cpp -- host side of the row accumulator (include/iqgpu.h "spectrogram"; kernels sgram.hip): the options and the
// row arithmetic (no device), and the iqgpu_sgram handle -- the stream core and the open row (the total of its closed cells and its
// open cell, two buffers each) -- with push / push_device / read_open / reset.  Independent of any chain.
// Options, tables, segment grid, stream position and carry are the power spectrum's: PsdStream (psd.hpp, psd.cpp).
#include "chain.hpp"
#include "sgram.hpp"

namespace {

constexpr size_t kPushSliceFrames = (size_t)1 << 20;     // of a host push: frames staged per slice (its rows come back per slice)
constexpr uint32_t kMaxRowSegments = (uint32_t)1 << 20;
const char *const kReset = "iqgpu_sgram_reset";

// o's part that is the power spectrum's
iqgpu_psd_opts psd_part(const iqgpu_sgram_opts &o)
{
    iqgpu_psd_opts q{};
    q.nfft = o.nfft; q.hop = o.hop; q.window = o.window; q.gain = o.gain;
    return q;
}

int check_opts(const iqgpu_sgram_opts *o, const char *who)
{
    if (!o) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    const iqgpu_psd_opts q = psd_part(*o);
    const int rc = psd_check_opts(&q, who); if (rc) return rc;
    if (o->row_segments < 1 || o->row_segments > kMaxRowSegments)
        return fail(IQGPU_EINVAL, "%s: row_segments %u is not in 1 .. %u", who, o->row_segments, kMaxRowSegments);
    return IQGPU_OK;
}

} // namespace

struct iqgpu_sgram {
    PsdStream st;
    iqgpu_sgram_opts o{};
    int open_cur = 0;                     // which half of `open` holds the open row (a launch writes the other: sgram.hip)
    DevBuf open, cells, rows_out;
    size_t cell_bins = 0;                 // of cells: [cell_bins] doubles, then [cell_bins] floats
    // open: 2 x { [nfft] total, [nfft] open cell } doubles, then 2 x { [nfft] total peak, [nfft] open-cell peak } floats
    double *tot_sum(int i) const { return (double *)open.p + (size_t)(2 * i) * o.nfft; }
    double *cell_sum(int i) const { return (double *)open.p + (size_t)(2 * i + 1) * o.nfft; }
    float *tot_pk(int i) const { return (float *)((double *)open.p + 4 * (size_t)o.nfft) + (size_t)(2 * i) * o.nfft; }
    float *cell_pk(int i) const { return (float *)((double *)open.p + 4 * (size_t)o.nfft) + (size_t)(2 * i + 1) * o.nfft; }
    size_t open_bytes() const { return (size_t)o.nfft * 4 * (sizeof(double) + sizeof(float)); }
    uint64_t rows_after(size_t n) const { return psd_segments_of(st.q, st.frames + n) / o.row_segments; }
    IQGPU_LOCAL ~iqgpu_sgram() { st.close(); }        // the waits first: the members free themselves behind them
};

namespace {

PsdStream *core(iqgpu_sgram *p) { return p ? &p->st : nullptr; }

// n frames of device memory behind everything pushed so far, on s; the rows they complete into d_sum / d_pk (device, either may be NULL)
int push_frames(iqgpu_sgram *p, const void *d_raw, size_t n, float *d_sum, float *d_pk, hipStream_t s)
{
    PsdStream &st = p->st;
    PsdPush u;
    int rc = st.enter(d_raw, n, s, &u); if (rc) return rc;
    const int64_t R = p->o.row_segments, C = sgram_cells_per_row(R), N = p->o.nfft, m = u.m;
    const int64_t cap = C == 1 ? kSgramDirectCells : kSgramCellBufBins / N;       // cells a launch
    // the cell buffer (R > 32 only): one slot for every cell the longest launch of this push touches (psd.cpp on growing such a buffer)
    if (m > 0 && C > 1) {
        const int64_t touched = sgram_cell_of((int64_t)u.segs - 1, R) - sgram_cell_of((int64_t)st.segments, R) + 1;
        const size_t bins = (size_t)((touched < cap ? touched : cap) * N);
        if (bins > p->cell_bins) {
            rc = p->cells.ensure(bins * (sizeof(double) + sizeof(float))); if (rc) return rc;
            p->cell_bins = bins;
        }
    }
    st.poisoned = true;                                                           // (until finish() has queued the last of the push)
    for (int64_t j = 0; j < m;) {
        const int64_t seg0 = (int64_t)st.segments + j, g0 = sgram_cell_of(seg0, R), r0 = seg0 / R;
        const int64_t room = sgram_cell_end(g0 + cap - 1, R) - seg0;              // whole cells up to the bound
        const int64_t cnt = m - j < room ? m - j : room, seg_end = seg0 + cnt;
        SgramCellsArgs a{};
        st.fill(u, j, cnt, &a);
        a.open_sum_in = p->cell_sum(p->open_cur); a.open_pk_in = p->cell_pk(p->open_cur);
        a.open_sum_out = p->cell_sum(p->open_cur ^ 1); a.open_pk_out = p->cell_pk(p->open_cur ^ 1);
        a.R = R; a.C = C; a.g0 = g0; a.r0 = r0;
        a.cell_sum = (double *)p->cells.p; a.cell_pk = p->cells.p ? (float *)((double *)p->cells.p + p->cell_bins) : nullptr;
        a.row_sum = d_sum; a.row_pk = d_pk;
        HIP_TRY(launch_sgram_cells(a, s));
        if (C > 1) {
            const int64_t g_last = sgram_cell_of(seg_end - 1, R);
            SgramFoldArgs f{};
            f.cell_sum = a.cell_sum; f.cell_pk = a.cell_pk; f.nfft = (int32_t)N;
            f.n_rows = (int32_t)((seg_end - 1) / R - r0 + 1); f.has_tot_in = seg0 % R >= kPsdPageSegments;
            f.R = R; f.C = C; f.g0 = g0; f.r0 = r0; f.n_closed = g_last - g0 + (sgram_cell_end(g_last, R) <= seg_end ? 1 : 0); f.seg_end = seg_end;
            f.tot_sum_in = p->tot_sum(p->open_cur); f.tot_pk_in = p->tot_pk(p->open_cur);
            f.tot_sum_out = p->tot_sum(p->open_cur ^ 1); f.tot_pk_out = p->tot_pk(p->open_cur ^ 1);
            f.row_sum = d_sum; f.row_pk = d_pk;
            HIP_TRY(launch_sgram_fold(f, s));
        }
        p->open_cur ^= 1;                                                         // the open row, if the launch left one, is in the other half
        const int64_t done = seg_end / R - r0;                                    // rows the launch finished
        if (d_sum) d_sum += done * N;
        if (d_pk) d_pk += done * N;
        j += cnt;
    }
    return st.finish(u);
}

// the checks of both pushes, in front of anything queued; *need = the rows the push completes
int begin_push(iqgpu_sgram *p, const void *raw, size_t frames, const float *row_sum, const float *row_peak, size_t cap_rows, size_t *rows,
               size_t *need, const char *who)
{
    if (rows) *rows = 0;
    const int rc = PsdStream::guard(core(p), raw || !frames, who, kReset, false); if (rc) return rc;
    *need = (size_t)(p->rows_after(frames) - p->st.segments / p->o.row_segments);
    if ((row_sum || row_peak) && *need > cap_rows)
        return fail(IQGPU_ECAPACITY, "%s: room for %zu rows, the push completes %zu (iqgpu_sgram_max_rows)", who, cap_rows, *need);
    if (frames) HIP_TRY(hipSetDevice(p->st.device));
    return IQGPU_OK;
}

} // namespace

extern "C" void iqgpu_sgram_opts_init(iqgpu_sgram_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->nfft = 1024; o->hop = 512; o->window = IQGPU_PSD_HANN; o->gain = 1.0f; o->row_segments = 32;
}

extern "C" int iqgpu_sgram_rows(const iqgpu_sgram_opts *o, uint64_t frames, uint64_t *rows)
{
    const int rc = check_opts(o, "iqgpu_sgram_rows"); if (rc) return rc;
    if (!rows) return fail(IQGPU_EINVAL, "iqgpu_sgram_rows: NULL argument");
    *rows = psd_segments_of(psd_part(*o), frames) / o->row_segments;
    return IQGPU_OK;
}

extern "C" int iqgpu_sgram_create(int device, int format, const iqgpu_sgram_opts *o, iqgpu_sgram **out)
{
    const char *who = "iqgpu_sgram_create";
    if (out) *out = nullptr;
    if (!out) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    int rc = check_opts(o, who); if (rc) return rc;
    const iqgpu_psd_opts q = psd_part(*o);
    iqgpu_sgram *p = new (std::nothrow) iqgpu_sgram;
    std::vector<float> tab;                                          // the source of the table upload: until the synchronise below
    rc = PsdStream::open(core(p), device, format, &q, who, tab);
    if (rc == IQGPU_OK) { p->o = *o; rc = p->open.ensure(p->open_bytes()); }
    if (rc == IQGPU_OK) {
        hipError_t e = hipMemsetAsync(p->open.p, 0, p->open_bytes(), p->st.own);
        if (e == hipSuccess) e = hipStreamSynchronize(p->st.own);
        if (e != hipSuccess) rc = fail(IQGPU_EHIP, "%s: %s", who, hipGetErrorString(e));
    }
    if (rc != IQGPU_OK) { delete p; return rc; }
    *out = p;
    return IQGPU_OK;
}

extern "C" void iqgpu_sgram_destroy(iqgpu_sgram *p) { delete p; }

extern "C" int iqgpu_sgram_reset(iqgpu_sgram *p)
{
    if (!p) return fail(IQGPU_EINVAL, "iqgpu_sgram_reset: NULL argument");
    const int rc = p->st.begin_reset(); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(p->open.p, 0, p->open_bytes(), p->st.own));
    HIP_TRY(hipStreamSynchronize(p->st.own));
    p->st.rewind(); p->open_cur = 0;
    return IQGPU_OK;
}

extern "C" size_t iqgpu_sgram_max_rows(const iqgpu_sgram *p, size_t frames)
{
    return p ? (size_t)(p->rows_after(frames) - p->st.segments / p->o.row_segments) : 0;
}

extern "C" int iqgpu_sgram_push_device(iqgpu_sgram *p, const void *d_raw, size_t frames, float *d_row_sum, float *d_row_peak, size_t cap_rows,
                                       size_t *rows, void *hip_stream)
{
    size_t need = 0;
    const int rc = begin_push(p, d_raw, frames, d_row_sum, d_row_peak, cap_rows, rows, &need, "iqgpu_sgram_push_device"); if (rc) return rc;
    if (frames == 0) return IQGPU_OK;
    if (rows) *rows = need;
    return push_frames(p, d_raw, frames, d_row_sum, d_row_peak, (hipStream_t)hip_stream);
}

extern "C" int iqgpu_sgram_push(iqgpu_sgram *p, const void *raw, size_t frames, float *row_sum, float *row_peak, size_t cap_rows, size_t *rows)
{
    size_t need = 0;
    int rc = begin_push(p, raw, frames, row_sum, row_peak, cap_rows, rows, &need, "iqgpu_sgram_push"); if (rc) return rc;
    if (frames == 0) return IQGPU_OK;
    PsdStream &st = p->st;
    const size_t slice = frames < kPushSliceFrames ? frames : kPushSliceFrames, N = p->o.nfft;
    // rows of one slice, whatever the position: the segments that start in a slice, and the one a carry completes
    const size_t slice_rows = (slice / p->o.hop + 1) / p->o.row_segments + 1;
    const int planes = (row_sum ? 1 : 0) + (row_peak ? 1 : 0);
    rc = st.stage.ensure(slice * st.bps); if (rc) return rc;
    if (planes) { rc = p->rows_out.ensure((size_t)planes * slice_rows * N * sizeof(float)); if (rc) return rc; }
    float *d_sum = row_sum ? (float *)p->rows_out.p : nullptr;
    float *d_pk = row_peak ? (float *)p->rows_out.p + (row_sum ? slice_rows * N : 0) : nullptr;
    if (rows) *rows = need;
    HostPlane out[2] = {{(char *)row_sum, d_sum, N * sizeof(float)}, {(char *)row_peak, d_pk, N * sizeof(float)}};
    return push_host_slices(st, st.stage, raw, frames, kPushSliceFrames, slice_rows, out, "iqgpu_sgram_push", "completes",
                            [&](size_t n) { return iqgpu_sgram_max_rows(p, n); },
                            [&](const void *d_raw, size_t n) { return push_frames(p, d_raw, n, d_sum, d_pk, st.own); });
}

extern "C" int iqgpu_sgram_read_open(iqgpu_sgram *p, double *sum_power, float *peak_power, iqgpu_sgram_info *info)
{
    int rc = PsdStream::guard(core(p), true, "iqgpu_sgram_read_open", kReset); if (rc) return rc;
    rc = p->st.settle(); if (rc) return rc;
    const size_t n = p->o.nfft;
    const uint32_t open_segments = (uint32_t)(p->st.segments % p->o.row_segments);
    if (sum_power || peak_power) {
        // the open row's closed cells are in the total, its open cell beside it; what the arithmetic says is empty is not looked at
        const bool has_tot = open_segments >= (uint32_t)kPsdPageSegments, has_cell = open_segments % (uint32_t)kPsdPageSegments != 0;
        std::vector<double> s; std::vector<float> k;
        try { s.assign(2 * n, 0.0); k.assign(2 * n, 0.0f); } catch (const std::bad_alloc &) { return fail(IQGPU_ENOMEM, "iqgpu_sgram_read_open: out of host memory"); }
        if (has_tot) {
            HIP_TRY(hipMemcpy(s.data(), p->tot_sum(p->open_cur), n * sizeof(double), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(k.data(), p->tot_pk(p->open_cur), n * sizeof(float), hipMemcpyDeviceToHost));
        }
        if (has_cell) {
            HIP_TRY(hipMemcpy(s.data() + n, p->cell_sum(p->open_cur), n * sizeof(double), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(k.data() + n, p->cell_pk(p->open_cur), n * sizeof(float), hipMemcpyDeviceToHost));
        }
        for (size_t i = 0; i < n; ++i) {                                 // (iqgpu_psd_read's expressions: total + open)
            if (sum_power) sum_power[i] = has_cell ? s[i] + s[n + i] : s[i];
            if (peak_power) peak_power[i] = has_cell ? fmaxf(k[i], k[n + i]) : k[i];
        }
    }
    if (info) {
        memset(info, 0, sizeof(*info));
        info->frames = p->st.frames; info->segments = p->st.segments; info->rows = p->st.segments / p->o.row_segments; info->open_segments = open_segments;
        info->nfft = p->o.nfft; info->hop = p->o.hop; info->row_segments = p->o.row_segments;
        info->window_sum = p->st.window_sum; info->window_sum_sq = p->st.window_sum_sq;
    }
    return IQGPU_OK;
}
