// psd.cpp -- host side of the power-spectrum accumulator (include/iqgpu.h "power spectrum"; kernels psd.hip): the options,
// the window tables and the segment arithmetic (no device); the stream core PsdStream (psd.hpp) that the row accumulator (sgram.cpp)
// holds too -- stream position, the carry of trailing frames, tables, streams; and the iqgpu_psd handle -- the core, the open page and
// the totals -- with push / push_device / read / reset.  Independent of any chain.
#include "chain.hpp"
#include "psd.hpp"

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr size_t kPushSliceFrames = (size_t)1 << 22;     // of a host push: frames staged per slice
const char *const kReset = "iqgpu_psd_reset";

int log2n_of(uint32_t nfft) { return nfft == 1024 ? 10 : nfft == 2048 ? 11 : nfft == 4096 ? 12 : 0; }

// periodic (DFT-even) forms, evaluated in double, rounded once
float window_at(int window, uint32_t i, uint32_t n)
{
    const double di = (double)i, dn = (double)n;
    switch (window) {
    case IQGPU_PSD_HANN: return (float)(0.5 - 0.5 * std::cos(2.0 * kPi * di / dn));
    case IQGPU_PSD_HAMMING: return (float)(0.54 - 0.46 * std::cos(2.0 * kPi * di / dn));
    case IQGPU_PSD_BLACKMAN_HARRIS:
        return (float)(0.35875 - 0.48829 * std::cos(2.0 * kPi * di / dn) + 0.14128 * std::cos(4.0 * kPi * di / dn) - 0.01168 * std::cos(6.0 * kPi * di / dn));
    default: return 1.0f;
    }
}

void fill_window(const iqgpu_psd_opts &o, float *w, double *sum, double *sum_sq)
{
    double s = 0.0, q = 0.0;
    for (uint32_t i = 0; i < o.nfft; ++i) {
        w[i] = window_at(o.window, i, o.nfft);
        s += (double)w[i]; q += (double)w[i] * (double)w[i];
    }
    if (sum) *sum = s;
    if (sum_sq) *sum_sq = q;
}

// the device tables: [nfft] window, then [nfft] twiddles exp(-2 pi i k / nfft) as (cos, sin) pairs -- double, rounded once
void fill_tables(const iqgpu_psd_opts &o, float *tab, double *sum, double *sum_sq)
{
    fill_window(o, tab, sum, sum_sq);
    for (uint32_t k = 0; k < o.nfft; ++k) {
        const double a = -2.0 * kPi * (double)k / (double)o.nfft;
        tab[o.nfft + 2 * k] = (float)std::cos(a); tab[o.nfft + 2 * k + 1] = (float)std::sin(a);
    }
}

} // namespace

// what sgram.cpp calls too (psd.hpp), so that the two accumulators cannot drift apart
int iqgpu::psd_check_opts(const iqgpu_psd_opts *o, const char *who)
{
    if (!o) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    if (!log2n_of(o->nfft)) return fail(IQGPU_EINVAL, "%s: nfft %u is not 1024, 2048 or 4096", who, o->nfft);
    if (o->hop != o->nfft && o->hop != o->nfft / 2 && o->hop != o->nfft / 4)
        return fail(IQGPU_EINVAL, "%s: hop %u is not nfft, nfft / 2 or nfft / 4 of nfft %u", who, o->hop, o->nfft);
    if (o->window < IQGPU_PSD_RECT || o->window > IQGPU_PSD_BLACKMAN_HARRIS) return fail(IQGPU_EINVAL, "%s: unknown window %d", who, o->window);
    if (!std::isfinite(o->gain)) return fail(IQGPU_EINVAL, "%s: gain is not finite", who);
    return IQGPU_OK;
}

uint64_t iqgpu::psd_segments_of(const iqgpu_psd_opts &o, uint64_t frames) { return frames < o.nfft ? 0 : (frames - o.nfft) / o.hop + 1; }

// ---- the stream core (psd.hpp) ----
int PsdStream::open(PsdStream *st, int device, int format, const iqgpu_psd_opts *o, const char *who, std::vector<float> &tab)
{
    int rc = psd_check_opts(o, who); if (rc) return rc;
    try { tab.resize(3 * (size_t)o->nfft); } catch (const std::bad_alloc &) { st = nullptr; }
    rc = AccumCore::open(st, device, format, who); if (rc) return rc;
    st->log2n = log2n_of(o->nfft); st->q = *o;
    fill_tables(*o, tab.data(), &st->window_sum, &st->window_sum_sq);
    rc = st->tables.ensure(tab.size() * sizeof(float));
    for (int i = 0; i < 2 && rc == IQGPU_OK; ++i) rc = st->carry[i].ensure((size_t)o->nfft * st->bps);
    if (rc) return rc;
    const hipError_t e = hipMemcpyAsync(st->tables.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, st->own);
    return e == hipSuccess ? IQGPU_OK : fail(IQGPU_EHIP, "%s: %s", who, hipGetErrorString(e));
}

int PsdStream::enter(const void *d_raw, size_t n, hipStream_t s, PsdPush *u)
{
    const int rc = note_stream(s); if (rc) return rc;
    u->raw = d_raw; u->n = n; u->s = s;
    u->frames = frames + n; u->segs = psd_segments_of(q, u->frames); u->m = (int64_t)(u->segs - segments);
    return IQGPU_OK;
}

int PsdStream::finish(const PsdPush &u)
{
    // the trailing frames the next segment starts with, into the other buffer (the launches of the push read this one)
    const size_t left = (size_t)(u.frames - u.segs * q.hop);
    PsdCarryArgs c{};
    c.carry = (const unsigned char *)carry[cur].p; c.raw = (const unsigned char *)u.raw;
    c.split_bytes = (int64_t)(carry_n * bps); c.first = (int64_t)((carry_n + u.n - left) * bps);
    c.bytes = (int32_t)(left * bps); c.dst = (unsigned char *)carry[cur ^ 1].p;
    HIP_TRY(launch_psd_carry(c, u.s));
    cur ^= 1; carry_n = left; frames = u.frames; segments = u.segs;
    poisoned = false;
    return IQGPU_OK;
}

struct iqgpu_psd {
    PsdStream st;
    int open_cur = 0;                     // which of the two open-page buffers holds the open page (the page kernel writes the other: psd.hip)
    Event staged;                         // a host push: the slice has left the caller's memory
    DevBuf sums, pages;
    size_t page_bins = 0;                 // of pages: [page_bins] doubles, then [page_bins] floats
    // sums: [nfft] total, 2 x [nfft] open (double), then [nfft] peak, 2 x [nfft] open peak (float)
    double *total_sum() const { return (double *)sums.p; }
    double *open_sum(int i) const { return (double *)sums.p + (size_t)(1 + i) * st.q.nfft; }
    float *total_pk() const { return (float *)((double *)sums.p + 3 * (size_t)st.q.nfft); }
    float *open_pk(int i) const { return total_pk() + (size_t)(1 + i) * st.q.nfft; }
    size_t sums_bytes() const { return (size_t)st.q.nfft * (3 * sizeof(double) + 3 * sizeof(float)); }
    IQGPU_LOCAL ~iqgpu_psd() { st.close(); }          // the waits first: the members free themselves behind them
};

namespace {

PsdStream *core(iqgpu_psd *p) { return p ? &p->st : nullptr; }

// n frames of device memory behind everything pushed so far, on s
int push_frames(iqgpu_psd *p, const void *d_raw, size_t n, hipStream_t s)
{
    PsdStream &st = p->st;
    PsdPush u;
    int rc = st.enter(d_raw, n, s, &u); if (rc) return rc;
    const int64_t N = st.q.nfft, G = kPsdPageSegments, cap = G * (kPsdPageBufBins / N), m = u.m;
    // the page buffer: one slot for every page the longest launch of this push touches, the whole bound at most (sized before anything is
    // queued).  Growing it frees the old one while kernels of earlier pushes may still be queued on the caller's stream: that is safe because
    // hipFree waits for the device, and it makes the first long push of a handle wait once (iqgpu_psd_push's staging buffer: the same)
    const int64_t touched = m / G + 2;
    const size_t bins = (size_t)(touched * N < kPsdPageBufBins ? touched * N : kPsdPageBufBins);
    if (m > 0 && bins > p->page_bins) {
        rc = p->pages.ensure(bins * (sizeof(double) + sizeof(float))); if (rc) return rc;
        p->page_bins = bins;
    }
    st.poisoned = true;                                                           // (until finish() has queued the last of the push)
    for (int64_t j = 0; j < m;) {
        const int64_t seg0 = (int64_t)st.segments + j;
        const int64_t cnt = m - j < cap - seg0 % G ? m - j : cap - seg0 % G;      // whole pages up to the page buffer's bound
        PsdPagesArgs a{};
        st.fill(u, j, cnt, &a);
        a.open_sum_in = p->open_sum(p->open_cur); a.open_pk_in = p->open_pk(p->open_cur);
        a.open_sum_out = p->open_sum(p->open_cur ^ 1); a.open_pk_out = p->open_pk(p->open_cur ^ 1);
        a.page_sum = (double *)p->pages.p; a.page_pk = (float *)((double *)p->pages.p + p->page_bins);
        HIP_TRY(launch_psd_pages(a, s));
        PsdFoldArgs f{};
        f.page_sum = a.page_sum; f.page_pk = a.page_pk; f.n_pages = (int32_t)((seg0 + cnt) / G - seg0 / G); f.nfft = (int32_t)N;
        f.total_sum = p->total_sum(); f.total_pk = p->total_pk();
        HIP_TRY(launch_psd_fold(f, s));
        if ((seg0 + cnt) % G != 0) p->open_cur ^= 1;                              // the launch left an open page, in the other buffer
        j += cnt;
    }
    return st.finish(u);
}

} // namespace

extern "C" void iqgpu_psd_opts_init(iqgpu_psd_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->nfft = 1024; o->hop = 512; o->window = IQGPU_PSD_HANN; o->gain = 1.0f;
}

extern "C" int iqgpu_psd_window(const iqgpu_psd_opts *o, float *w, size_t cap, double *sum, double *sum_sq)
{
    const int rc = psd_check_opts(o, "iqgpu_psd_window"); if (rc) return rc;
    if (!w) return fail(IQGPU_EINVAL, "iqgpu_psd_window: NULL argument");
    if (cap < o->nfft) return fail(IQGPU_EINVAL, "iqgpu_psd_window: room for %zu values, the window has %u", cap, o->nfft);
    fill_window(*o, w, sum, sum_sq);
    return IQGPU_OK;
}

extern "C" int iqgpu_psd_segments(const iqgpu_psd_opts *o, uint64_t frames, uint64_t *segments)
{
    const int rc = psd_check_opts(o, "iqgpu_psd_segments"); if (rc) return rc;
    if (!segments) return fail(IQGPU_EINVAL, "iqgpu_psd_segments: NULL argument");
    *segments = psd_segments_of(*o, frames);
    return IQGPU_OK;
}

extern "C" void iqgpu_psd_geometry(size_t *segments_per_page)
{
    if (segments_per_page) *segments_per_page = (size_t)kPsdPageSegments;
}

extern "C" int iqgpu_psd_create(int device, int format, const iqgpu_psd_opts *o, iqgpu_psd **out)
{
    const char *who = "iqgpu_psd_create";
    if (out) *out = nullptr;
    if (!out) return fail(IQGPU_EINVAL, "%s: NULL argument", who);
    iqgpu_psd *p = new (std::nothrow) iqgpu_psd;
    std::vector<float> tab;                                          // the source of the table upload: until the synchronise below
    int rc = PsdStream::open(core(p), device, format, o, who, tab);
    if (rc == IQGPU_OK) rc = p->sums.ensure(p->sums_bytes());
    if (rc == IQGPU_OK) {
        hipError_t e = p->staged.create(hipEventDisableTiming);
        if (e == hipSuccess) e = hipMemsetAsync(p->sums.p, 0, p->sums_bytes(), p->st.own);
        if (e == hipSuccess) e = hipStreamSynchronize(p->st.own);
        if (e != hipSuccess) rc = fail(IQGPU_EHIP, "%s: %s", who, hipGetErrorString(e));
    }
    if (rc != IQGPU_OK) { delete p; return rc; }
    *out = p;
    return IQGPU_OK;
}

extern "C" void iqgpu_psd_destroy(iqgpu_psd *p) { delete p; }

extern "C" int iqgpu_psd_reset(iqgpu_psd *p)
{
    if (!p) return fail(IQGPU_EINVAL, "iqgpu_psd_reset: NULL argument");
    const int rc = p->st.begin_reset(); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(p->sums.p, 0, p->sums_bytes(), p->st.own));
    HIP_TRY(hipStreamSynchronize(p->st.own));
    p->st.rewind(); p->open_cur = 0;
    return IQGPU_OK;
}

extern "C" int iqgpu_psd_push_device(iqgpu_psd *p, const void *d_raw, size_t frames, void *hip_stream)
{
    if (p && frames == 0) return IQGPU_OK;
    const int rc = PsdStream::guard(core(p), d_raw, "iqgpu_psd_push_device", kReset); if (rc) return rc;
    return push_frames(p, d_raw, frames, (hipStream_t)hip_stream);
}

extern "C" int iqgpu_psd_push(iqgpu_psd *p, const void *raw, size_t frames)
{
    if (p && frames == 0) return IQGPU_OK;
    int rc = PsdStream::guard(core(p), raw, "iqgpu_psd_push", kReset); if (rc) return rc;
    PsdStream &st = p->st;
    rc = st.stage.ensure((frames < kPushSliceFrames ? frames : kPushSliceFrames) * st.bps); if (rc) return rc;
    for (size_t at = 0; at < frames;) {
        const size_t n = frames - at < kPushSliceFrames ? frames - at : kPushSliceFrames;
        // (the one staging buffer: the copy is ordered behind the kernels of the slice in front on the handle's stream)
        HIP_TRY(hipMemcpyAsync(st.stage.p, (const char *)raw + at * st.bps, n * st.bps, hipMemcpyHostToDevice, st.own));
        HIP_TRY(hipEventRecord(p->staged, st.own));
        rc = push_frames(p, st.stage.p, n, st.own); if (rc) return rc;
        HIP_TRY(hipEventSynchronize(p->staged));                     // the caller's memory is free when the call returns
        at += n;
    }
    return IQGPU_OK;
}

extern "C" int iqgpu_psd_read(iqgpu_psd *p, double *sum_power, float *peak_power, iqgpu_psd_info *info)
{
    int rc = PsdStream::guard(core(p), true, "iqgpu_psd_read", kReset); if (rc) return rc;
    rc = p->st.settle(); if (rc) return rc;
    const size_t n = p->st.q.nfft;
    if (sum_power || peak_power) {
        std::vector<double> s; std::vector<float> k;
        try { s.resize(2 * n); k.resize(2 * n); } catch (const std::bad_alloc &) { return fail(IQGPU_ENOMEM, "iqgpu_psd_read: out of host memory"); }
        HIP_TRY(hipMemcpy(s.data(), p->total_sum(), n * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(s.data() + n, p->open_sum(p->open_cur), n * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(k.data(), p->total_pk(), n * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(k.data() + n, p->open_pk(p->open_cur), n * sizeof(float), hipMemcpyDeviceToHost));
        const bool open = p->st.segments % (uint64_t)kPsdPageSegments != 0;      // else the open arrays hold a page already folded
        for (size_t i = 0; i < n; ++i) {
            if (sum_power) sum_power[i] = open ? s[i] + s[n + i] : s[i];
            if (peak_power) peak_power[i] = open ? fmaxf(k[i], k[n + i]) : k[i];
        }
    }
    if (info) {
        memset(info, 0, sizeof(*info));
        info->frames = p->st.frames; info->segments = p->st.segments; info->nfft = p->st.q.nfft; info->hop = p->st.q.hop;
        info->window_sum = p->st.window_sum; info->window_sum_sq = p->st.window_sum_sq;
    }
    return IQGPU_OK;
}
